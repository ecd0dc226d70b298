"""The contract of the native RAFT path's precision mode "fp16" (include/atlasfit.h: AF_RAFT_FP16) as a torch
restatement in any working dtype (a helper; not collected).  In fp64 it is the "contract twin" of tests/test_gpu_raft_fp16.py.

q(x) = x.half().to(x.dtype) marks every place where the mode rounds; everything else is tools/make_golden_raft.py's restatement:

  convolution   y = q(conv(q(x), q(w)) + q(b)), then q(act(y * oscale)); products and the sum in the working dtype
  GRU           z, r = q(sigmoid(y)); r * h rounded once; q = q(tanh(y)); h' = q((1 - z) h + z q)
  norms         q(relu(norm(x))) and q(relu(res + relu(norm(x)))): one rounding at the store
  fp32 (here: the working dtype)   the correlation volume from the fp16-valued feature maps, pooling, lookup, coords1 += delta,
                flow = coords1 - coords0 (rounded only where a convolution gathers it), the convex upsampling
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_golden_raft as G  # noqa: E402

ACTS = {"none": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


def q(x):
    """Round to fp16 (nearest even, subnormals kept, overflow to inf) and come back to x's dtype."""
    return x.half().to(x.dtype)


def conv_sum(x, w, b, stride=1, pad=0):
    """y of the contract: fp16(sum + bias16), operands rounded on the way in."""
    return q(F.conv2d(q(x), q(w), None if b is None else q(b), stride, pad))


def conv(x, w, b, stride=1, pad=0, act="none", oscale=1.0):
    return q(ACTS[act](conv_sum(x, w, b, stride, pad) * oscale))


def gru_half(net, x, wz, bz, wr, br, wq, bq, pad):
    hx = torch.cat([net, x], 1)
    z = q(torch.sigmoid(conv_sum(hx, wz, bz, 1, pad)))
    r = q(torch.sigmoid(conv_sum(hx, wr, br, 1, pad)))
    qq = q(torch.tanh(conv_sum(torch.cat([q(r * net), x], 1), wq, bq, 1, pad)))
    return q((1 - z) * net + z * qq)


def norm_store(v, relu, res=None):
    """The normalise pass's store: v is the normalised tensor."""
    if relu:
        v = torch.relu(v)
    if res is not None:
        v = torch.relu(res + v)
    return q(v)


def _encoder(sd, p, x, norm):
    def nrm(v, name):
        if norm == "instance":
            return F.instance_norm(v, eps=1e-5)
        return F.batch_norm(v, sd[p + name + ".running_mean"], sd[p + name + ".running_var"], sd[p + name + ".weight"], sd[p + name + ".bias"], False, 0.0, 1e-5)

    def cv(v, name, stride=1, pad=0):
        return conv(v, sd[p + name + ".weight"], sd[p + name + ".bias"], stride, pad)
    x = norm_store(nrm(cv(x, "conv1", 2, 3), "norm1"), True)
    for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
        for b in (0, 1):
            n = "%s.%d." % (layer, b)
            s = stride if b == 0 else 1
            y = norm_store(nrm(cv(x, n + "conv1", s, 1), n + "norm1"), True)
            y = nrm(cv(y, n + "conv2", 1, 1), n + "norm2")
            if s != 1:
                x = norm_store(nrm(cv(x, n + "downsample.0", s, 0), n + "norm3"), False)
            x = norm_store(y, True, x)
    return conv_sum(x, sd[p + "conv2.weight"], sd[p + "conv2.bias"])


def update_step(sd, net, inp, corr, flow, want_mask=True):
    p = "update_block."

    def cv(v, name, pad, act="relu", oscale=1.0):
        return conv(v, sd[p + name + ".weight"], sd[p + name + ".bias"], 1, pad, act, oscale)
    cor = cv(cv(corr, "encoder.convc1", 0), "encoder.convc2", 1)
    flo = cv(cv(flow, "encoder.convf1", 3), "encoder.convf2", 1)
    motion = torch.cat([cv(torch.cat([cor, flo], 1), "encoder.conv", 1), flow], 1)      # the flow channels stay fp32: rounded where gathered
    x = torch.cat([inp, motion], 1)
    for n, pad in (("1", (0, 2)), ("2", (2, 0))):
        w = [sd[p + "gru.conv%s%s.%s" % (g, n, t)] for g in "zrq" for t in ("weight", "bias")]
        net = gru_half(net, x, *w, pad)
    delta = cv(cv(net, "flow_head.conv1", 1), "flow_head.conv2", 1, "none")
    mask = cv(cv(net, "mask.0", 1), "mask.2", 0, "none", 0.25) if want_mask else None
    return net, mask, delta, motion


def raft_forward(sd, im1, im2, iters=20, acts=None, state=None):
    """make_golden_raft.raft_forward under the contract: same arguments, same returns, same named intermediates."""
    with torch.no_grad():
        a, b = 2 * (im1 / 255.0) - 1.0, 2 * (im2 / 255.0) - 1.0
        f1, f2 = _encoder(sd, "fnet.", a, "instance"), _encoder(sd, "fnet.", b, "instance")
        c = _encoder(sd, "cnet.", a, "batch")
        net, inp = q(torch.tanh(c[:, :128])), q(torch.relu(c[:, 128:]))
        pyr = G.corr_pyramid(G.corr_volume(f1, f2))
        h, w = f1.shape[-2:]
        coords0 = G.coords_grid(h, w, a.dtype)
        coords1 = coords0.clone()
        if acts is not None:
            acts.update(fmap1=f1, fmap2=f2, net0=net, inp=inp)
        if state is not None:
            net, coords1 = q(state[0]), state[1]
        mask = None
        for it in range(iters):
            corr = G.corr_lookup(pyr, coords1)
            flow = coords1 - coords0
            net, mask, delta, motion = update_step(sd, net, inp, corr, flow, want_mask=(it == iters - 1))
            coords1 = coords1 + delta
            if acts is not None and it == iters - 1:
                acts.update(motion=motion, net=net, delta=delta, mask=mask, coords1=coords1)
        return coords1 - coords0, G.upsample_flow(coords1 - coords0, mask)
