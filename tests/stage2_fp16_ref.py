"""The contract of stage 2's precision mode "fp16" (include/atlasfit.h: AF_FILTER_FP16) as a torch restatement in any
working dtype (a helper; not collected).  In fp64 it is the "contract twin" of tests/test_gpu_stage2_fp16.py.

q, conv_sum and conv are tests/raft_fp16_ref.py's: q(x) = x.half().to(x.dtype) marks every place where the mode rounds.

  convolution   y = q(conv(q(x), q(w)) + q(b)); v = q(act(y)) with act none / ReLU / LeakyReLU(0.2) / tanh; then q(v + residual);
                products and the sum in the working dtype; reflection padding moves values, so it commutes with q
  bilinear x2   q(F.interpolate(..., align_corners=True)) on fp16 values: one rounding
  LSTM finish   i = q(sigmoid(in)), o = q(sigmoid(out)), g = q(tanh(cell gate)), cell = q(i g), hidden = q(o tanh(cell))
                (autocast keeps cell and hidden in fp32, prev_state being fp32 zeros; hidden's only consumer is a convolution that
                rounds as it gathers, so the operand bits are the same)
  final         q(pred + Y); frame 0: final = pred
  moves         replicate pad, the 12-channel pack, maxpool, nearest x2
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from raft_fp16_ref import q, conv_sum, conv  # noqa: E402

ACT_NAMES = ("none", "relu", "leaky", "tanh")      # af_conv2d's act codes 0..3


def conv2d(x, w, b, stride=1, pad_mode=0, act=0, res=None):
    """One convolution of the mode on NCHW tensors: padding k // 2 (pad_mode 0 zeros, 1 reflection), act an af_conv2d code."""
    k = w.shape[-1]
    pad = k // 2
    if pad_mode:
        x, pad = F.pad(x, [k // 2] * 4, mode="reflect"), 0
    if ACT_NAMES[act] == "leaky":
        v = q(F.leaky_relu(conv_sum(x, w, b, stride, pad), 0.2))
    else:
        v = conv(x, w, b, stride, pad, ACT_NAMES[act])
    return v if res is None else q(v + res)


def unet_half(sd, x, acts):
    def block(x, p):
        return conv2d(conv2d(x, sd[p + "conv1.weight"], None, act=1), sd[p + "conv2.weight"], None, act=1)
    enc, h = [], x
    for i in range(1, 5):
        h = block(h, "encoder%d.enc%d" % (i, i))
        acts["enc%d" % i] = h
        enc.append(h)
        h = F.max_pool2d(h, 2, 2)
    h = block(h, "bottleneck.bottleneck")
    acts["bottleneck"] = h
    for n in (4, 3, 2, 1):
        u = q(F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=True))
        u = conv2d(u, sd["upconv%d.1.weight" % n], sd["upconv%d.1.bias" % n])
        h = block(torch.cat((u, enc[n - 1]), 1), "decoder%d.dec%d" % (n, n))
        acts["dec%d" % n] = h
    return conv2d(h, sd["conv.weight"], sd["conv.bias"])


def local_half(sd, X, acts):
    def cl(x, name, stride=1, act=2, res=None):
        return conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride, 1, act, res)
    E1a, E1b = cl(X[:, :6], "conv1a.conv2d"), cl(X[:, 6:], "conv1b.conv2d")
    E2a, E2b = cl(E1a, "conv2a.conv2d", 2), cl(E1b, "conv2b.conv2d", 2)
    E3 = cl(torch.cat((E2a, E2b), 1), "conv3.conv2d", 2)
    RB = E3
    for b in range(5):
        RB = cl(cl(RB, "ResBlocks.%d.conv1.conv2d" % b), "ResBlocks.%d.conv2.conv2d" % b, act=0, res=RB)
    # the Gates conv reads cat(RB, hidden = 0): only its first 128 input channels meet non-zero operands
    gates = conv2d(RB, sd["convlstm.Gates.weight"][:, :128], sd["convlstm.Gates.bias"])
    gi, _, go, gc = gates.chunk(4, 1)
    cell = q(q(torch.sigmoid(gi)) * q(torch.tanh(gc)))
    hidden = q(q(torch.sigmoid(go)) * torch.tanh(cell))
    D2 = cl(F.interpolate(hidden, scale_factor=2, mode="nearest"), "deconv1.conv2d")
    D1 = cl(F.interpolate(torch.cat((D2, E2a), 1), scale_factor=2, mode="nearest"), "deconv2.conv2d")
    Y = cl(torch.cat((D1, E1a), 1), "deconv3.conv2d", act=3)
    acts.update(E1a=E1a, E1b=E1b, E2a=E2a, E2b=E2b, E3=E3, RB=RB, hidden=hidden, D2=D2, D1=D1, Y=Y)
    return Y


def loop(fsd, lsd, contents, styles, dtype):
    """The frame loop under the contract: contents / styles padded NCHW fp32 tensors (u8 / 255); per frame a dict of the named
    intermediates af_filter_debug_activation knows (those that exist on that frame), HWC float64 numpy."""
    fsd = {k: v.to(dtype) for k, v in fsd.items()}
    lsd = {k: v.to(dtype) for k, v in lsd.items() if v.is_floating_point()}
    out, o1, p1 = [], None, None
    with torch.no_grad():
        for t, (c, s) in enumerate(zip(contents, styles)):
            acts = {"input": torch.cat((c, s), 1).to(dtype)}      # fp32 values: the first convolutions round them as they gather
            pred = unet_half(fsd, acts["input"], acts)
            if t == 0:
                o1 = p1 = final = pred
            else:
                final = q(pred + local_half(lsd, torch.cat((pred, o1, pred, p1), 1), acts))
                p1, o1 = pred, final
            acts.update(pred=pred, final=final)
            out.append({k: v[0].permute(1, 2, 0).double().numpy() for k, v in acts.items()})
    return out


# ---- the single-convolution sweep of tests/test_gpu_stage2_fp16.py (and its CPU companion in tests/test_stage2_fp16_host.py) ----------
SWEEP = [                                # (cin, cout, k, stride, pad_mode, h, w)
    (12, 32, 7, 1, 1, 9, 11),            # K = 588, which no chunk divides; a partial M tile with reflection
    (128, 128, 3, 2, 1, 13, 10),         # stride 2 on odd sizes
    (64, 3, 7, 1, 1, 12, 45),            # Cout = 3 at BN 32; more than four M tiles
    (6, 32, 3, 1, 0, 8, 17),             # K = 54
    (32, 3, 1, 1, 0, 3, 43),             # K equal to one chunk; M = 129
    (128, 512, 3, 1, 0, 5, 7),           # BN 128, the gates shape
    (512, 512, 3, 1, 0, 4, 6),           # K = 4608
]


def draw_conv(shape, xscale=1.0, wscale=1.0, half=True, residual=False):
    """Seeded operands of a sweep shape, NCHW: x, weight, bias, residual (or None); half: already fp16 values."""
    cin, cout, k, stride, _, h, w = shape
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + k)
    x = torch.randn((1, cin, h, w), generator=gen) * xscale
    wt = (torch.rand((cout, cin, k, k), generator=gen) * 2 - 1) * float((6.0 / (cin * k * k)) ** 0.5) * wscale
    b = (torch.rand((cout,), generator=gen) * 2 - 1) * 0.05 * wscale
    r = torch.randn((1, cout, (h - 1) // stride + 1, (w - 1) // stride + 1), generator=gen) if residual else None
    if half:
        x, wt, b, r = x.half().float(), wt.half().float(), b.half().float(), None if r is None else r.half().float()
    return x, wt, b, r


def torch_half_conv(x, w, b, stride, pad_mode, act, res=None):
    """torch's own half convolution on the CPU with the mode's epilogue as half tensors (the yardstick of the 2x rule), as float64."""
    k = w.shape[-1]
    xh = F.pad(x.half(), [k // 2] * 4, mode="reflect") if pad_mode else F.pad(x.half(), [k // 2] * 4)
    y = F.conv2d(xh, w.half(), None if b is None else b.half(), stride)
    y = [lambda v: v, F.relu, lambda v: F.leaky_relu(v, 0.2), torch.tanh][act](y)
    if res is not None:
        y = y + res.half()
    assert y.dtype == torch.float16
    return y.double()
