"""Stage 2 on the GPU (include/atlasfit.h: af_filter_*, af_conv2d) against tests/golden/stage2.npz, which
tools/make_golden_stage2.py computed with the reference's own UNet and TransformNet modules (fp32 and an fp64 twin).

Rule (the project's usual one): for every compared tensor, max and rms of |hip - fp64| are each at most twice the same statistic of
|torch fp32 - fp64| on the CPU.  The per-layer checks use the functional restatement below (`unet_ref`, `local_ref`), whose fp64
output is first checked against the fixture's twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage2.npz")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_stage2 import synthetic_state_dicts, pad_other, LO_SCALE  # noqa: E402


def _shapes(table):
    return [tuple(int(v) for v in r if v >= 0) for r in table]


@pytest.fixture(scope="module")
def g2():
    g = dict(np.load(GOLDEN))
    for w in ("pred", "final"):
        g[w + "64"] = g[w + "64_hi"].astype(np.float64) + g[w + "64_lo"].astype(np.float64) / LO_SCALE
    fsd = {str(k): torch.zeros(s) for k, s in zip(g["filter_keys"], _shapes(g["filter_shapes"]))}
    lsd = {str(k): torch.zeros(s) for k, s in zip(g["local_keys"], _shapes(g["local_shapes"]))}
    for k in lsd:
        if k.endswith("running_var"):
            lsd[k] += 1.0
        if k.endswith("num_batches_tracked"):
            lsd[k] = torch.zeros((), dtype=torch.int64)
    synthetic_state_dicts(fsd, lsd)
    g["fsd"], g["lsd"] = fsd, lsd
    return g


@pytest.fixture(scope="module")
def nf(g2):
    import aiod_amd
    f = aiod_amd.NeuralFilter(40, 70)
    f.load_state_dicts(g2["fsd"], g2["lsd"])
    yield f
    f.close()


# ---- functional restatement of network_filter.py / network_local.py (NCHW, any dtype) ---------------------------------------
def unet_ref(sd, x, acts):
    def block(x, p):
        x = F.relu(F.conv2d(x, sd[p + "conv1.weight"], padding=1))
        return F.relu(F.conv2d(x, sd[p + "conv2.weight"], padding=1))
    enc = []
    h = x
    for i in range(1, 5):
        h = block(h, "encoder%d.enc%d" % (i, i))
        acts["enc%d" % i] = h
        enc.append(h)
        h = F.max_pool2d(h, 2, 2)
    h = block(h, "bottleneck.bottleneck")
    acts["bottleneck"] = h
    for n in (4, 3, 2, 1):
        u = F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=True)
        u = F.conv2d(u, sd["upconv%d.1.weight" % n], sd["upconv%d.1.bias" % n], padding=1)
        h = block(torch.cat((u, enc[n - 1]), 1), "decoder%d.dec%d" % (n, n))
        acts["dec%d" % n] = h
    return F.conv2d(h, sd["conv.weight"], sd["conv.bias"])


def local_ref(sd, X, acts):
    lk = lambda v: F.leaky_relu(v, 0.2)     # noqa: E731

    def cl(x, name, stride=1):
        w = sd[name + ".weight"]
        k = w.shape[-1]
        return F.conv2d(F.pad(x, [k // 2] * 4, mode="reflect"), w, sd[name + ".bias"], stride)
    E1a = lk(cl(X[:, :6], "conv1a.conv2d"))
    E1b = lk(cl(X[:, 6:], "conv1b.conv2d"))
    E2a = lk(cl(E1a, "conv2a.conv2d", 2))
    E2b = lk(cl(E1b, "conv2b.conv2d", 2))
    E3 = lk(cl(torch.cat((E2a, E2b), 1), "conv3.conv2d", 2))
    RB = E3
    for b in range(5):
        RB = cl(lk(cl(RB, "ResBlocks.%d.conv1.conv2d" % b)), "ResBlocks.%d.conv2.conv2d" % b) + RB
    gates = F.conv2d(torch.cat((RB, torch.zeros_like(RB)), 1), sd["convlstm.Gates.weight"], sd["convlstm.Gates.bias"], padding=1)
    gi, gr, go, gc = gates.chunk(4, 1)
    cell = torch.sigmoid(gr) * torch.zeros_like(gr) + torch.sigmoid(gi) * torch.tanh(gc)
    hidden = torch.sigmoid(go) * torch.tanh(cell)
    D2 = lk(cl(F.interpolate(hidden, scale_factor=2, mode="nearest"), "deconv1.conv2d"))
    D1 = lk(cl(F.interpolate(torch.cat((D2, E2a), 1), scale_factor=2, mode="nearest"), "deconv2.conv2d"))
    Y = torch.tanh(cl(torch.cat((D1, E1a), 1), "deconv3.conv2d"))
    acts.update(E1a=E1a, E1b=E1b, E2a=E2a, E2b=E2b, E3=E3, RB=RB, hidden=hidden, D2=D2, D1=D1, Y=Y)
    return Y


def ref_loop(g2, dtype, nframes):
    """The frame loop on the restatement; per frame (pred, final, activations), all HWC float64 numpy."""
    fsd = {k: v.to(dtype) for k, v in g2["fsd"].items()}
    lsd = {k: v.to(dtype) for k, v in g2["lsd"].items() if v.is_floating_point()}
    out, o1, p1 = [], None, None
    with torch.no_grad():
        for t in range(nframes):
            c = pad_other(torch.from_numpy(g2["content"][t] / 255.0).permute(2, 0, 1)[None].float().to(dtype))
            s = pad_other(torch.from_numpy(g2["style"][t] / 255.0).permute(2, 0, 1)[None].float().to(dtype))
            acts = {"input": torch.cat((c, s), 1)}
            pred = unet_ref(fsd, acts["input"], acts)
            if t == 0:
                o1 = p1 = final = pred
            else:
                final = pred + local_ref(lsd, torch.cat((pred, o1, pred, p1), 1), acts)
                p1, o1 = pred, final
            acts.update(pred=pred, final=final)
            out.append({k: v[0].permute(1, 2, 0).double().numpy() for k, v in acts.items()})
    return out


def _frames(g2, t):
    return g2["content"][t] / 255.0, g2["style"][t] / 255.0


def _stats(d):
    d = np.abs(np.asarray(d, np.float64)).ravel()
    return d.max(), np.sqrt((d ** 2).mean())


def _within(hip, ref32, ref64, what):
    hm, hr = _stats(hip - ref64)
    rm, rr = _stats(ref32 - ref64)
    assert hm <= 2 * rm and hr <= 2 * rr, "%s: hip max %.3g rms %.3g, torch fp32 max %.3g rms %.3g" % (what, hm, hr, rm, rr)
    return hm, hr, rm, rr


def test_end_to_end_against_fixture(g2, nf):
    nf.reset()
    n = g2["pred64"].shape[0]
    for t in range(n):
        pred, final = nf.frame(*_frames(g2, t))
        assert pred.shape == (64, 96, 3) and final.shape == (64, 96, 3)
        for w, v in (("pred", pred), ("final", final)):
            hm, hr = _stats(v - g2[w + "64"][t])
            rm, rr = g2[w + "_err32"][t]
            print("frame %d %s: hip max %.3g rms %.3g | torch fp32 max %.3g rms %.3g" % (t, w, hm, hr, rm, rr))
            assert hm <= 2 * rm and hr <= 2 * rr, (t, w, hm, hr, rm, rr)


def test_frame0_final_is_pred_and_reset_reproduces(g2, nf):
    nf.reset()
    first = [tuple(a.copy() for a in nf.frame(*_frames(g2, t))) for t in range(3)]
    assert np.array_equal(first[0][0], first[0][1])                 # frame 0: final == pred, bit for bit
    assert not np.array_equal(first[1][0], first[1][1])
    nf.reset()
    again = [nf.frame(*_frames(g2, t)) for t in range(3)]
    for a, b in zip(first, again):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # device tensors in and out: the same numbers
    nf.reset()
    for t in range(2):
        c, s = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in _frames(g2, t))
        p, f = nf.frame(c, s)
        assert p.is_cuda and np.array_equal(p.cpu().numpy(), first[t][0]) and np.array_equal(f.cpu().numpy(), first[t][1])


def test_per_layer_against_restatement(g2, nf):
    r64 = ref_loop(g2, torch.float64, 2)
    for w in ("pred", "final"):        # the restatement is the reference's modules: its fp64 output is the fixture's twin
        for t in range(2):
            assert np.abs(r64[t][w] - g2[w + "64"][t]).max() < 1e-9, (w, t)
    r32 = ref_loop(g2, torch.float32, 2)
    nf.reset()
    for t in range(2):
        nf.frame(*_frames(g2, t))
    import aiod_amd
    for name in aiod_amd.stage2.ACTIVATIONS:
        hip = nf.activation(name)
        assert hip.shape == r64[1][name].shape, name
        hm, hr, rm, rr = _within(hip, r32[1][name], r64[1][name], name)
        print("%-10s hip max %.3g rms %.3g | torch fp32 max %.3g rms %.3g" % (name, hm, hr, rm, rr))
    nf.reset()
    nf.frame(*_frames(g2, 0))
    with pytest.raises(aiod_amd.AtlasFitError):       # the refinement net did not run on a frame 0
        nf.activation("E1a")


# every distinct layer shape of both nets (cin, cout, k, stride, pad_mode, act, bias, residual, h, w), plus odd sizes
CONV_CASES = [
    (6, 32, 3, 1, 0, 1, False, False, 64, 96), (32, 32, 3, 1, 0, 1, False, False, 64, 96), (32, 64, 3, 1, 0, 1, False, False, 32, 48),
    (64, 64, 3, 1, 0, 1, False, False, 32, 48), (64, 128, 3, 1, 0, 1, False, False, 16, 24), (128, 128, 3, 1, 0, 1, False, False, 16, 24),
    (128, 256, 3, 1, 0, 1, False, False, 8, 12), (256, 256, 3, 1, 0, 1, False, False, 8, 12), (256, 512, 3, 1, 0, 1, False, False, 4, 6),
    (512, 512, 3, 1, 0, 1, False, False, 4, 6), (512, 256, 3, 1, 0, 0, True, False, 8, 12), (256, 128, 3, 1, 0, 0, True, False, 16, 24),
    (128, 64, 3, 1, 0, 0, True, False, 32, 48), (64, 32, 3, 1, 0, 0, True, False, 64, 96), (32, 3, 1, 1, 0, 0, True, False, 64, 96),
    (6, 32, 7, 1, 1, 2, True, False, 64, 96), (32, 64, 3, 2, 1, 2, True, False, 64, 96), (128, 128, 3, 2, 1, 2, True, False, 32, 48),
    (128, 128, 3, 1, 1, 2, True, False, 16, 24), (128, 128, 3, 1, 1, 0, True, True, 16, 24), (128, 512, 3, 1, 0, 0, True, False, 16, 24),
    (128, 64, 3, 1, 1, 2, True, False, 32, 48), (128, 32, 3, 1, 1, 2, True, False, 64, 96), (64, 3, 7, 1, 1, 3, True, False, 64, 96),
    (12, 32, 7, 1, 1, 2, True, False, 37, 53), (6, 17, 3, 2, 1, 1, True, False, 33, 21), (12, 40, 3, 2, 0, 3, False, True, 29, 31),
    (7, 5, 1, 2, 0, 0, True, False, 9, 11), (33, 70, 7, 2, 1, 2, True, True, 23, 19),
]


def _torch_conv(x, w, b, stride, pad_mode, act, res):
    k = w.shape[-1]
    x = x.permute(2, 0, 1)[None]
    x = F.pad(x, [k // 2] * 4, mode="reflect") if pad_mode else F.pad(x, [k // 2] * 4)
    y = F.conv2d(x, w, b, stride)
    y = [lambda v: v, F.relu, lambda v: F.leaky_relu(v, 0.2), torch.tanh][act](y)
    y = y[0].permute(1, 2, 0)
    return y + res if res is not None else y


def test_conv2d_sweep():
    import aiod_amd
    g = torch.Generator().manual_seed(7)
    worst = []
    for i, (cin, cout, k, stride, pm, act, has_b, has_r, h, w) in enumerate(CONV_CASES):
        x = torch.rand(h, w, cin, generator=g, dtype=torch.float64) * 2 - 1
        wt = (torch.rand(cout, cin, k, k, generator=g, dtype=torch.float64) * 2 - 1) * np.sqrt(6.0 / (cin * k * k))
        b = (torch.rand(cout, generator=g, dtype=torch.float64) - 0.5) * 0.1 if has_b else None
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        r = torch.rand(ho, wo, cout, generator=g, dtype=torch.float64) if has_r else None
        f32 = lambda t: None if t is None else t.float()      # noqa: E731
        args = [f32(x), f32(wt), f32(b), f32(r)]
        ref64 = _torch_conv(*[None if a is None else a.double() for a in args[:3]], stride, pm, act, None if r is None else args[3].double()).numpy()
        ref32 = _torch_conv(args[0], args[1], args[2], stride, pm, act, args[3]).double().numpy()
        hip = aiod_amd.stage2.conv2d(args[0].numpy(), args[1].numpy(), None if b is None else args[2].numpy(), stride, pm, act,
                                     None if r is None else args[3].numpy())
        assert hip.shape == ref64.shape, (i, hip.shape, ref64.shape)
        worst.append(_within(hip, ref32, ref64, "case %d %s" % (i, CONV_CASES[i])))
        if i in (0, 19):          # device pointers: the same numbers
            dev = [None if a is None else a.cuda() for a in args]
            hd = aiod_amd.stage2.conv2d(dev[0], dev[1], dev[2], stride, pm, act, dev[3])
            assert np.array_equal(hd.cpu().numpy(), hip), i
    print("conv2d sweep: worst hip/torch max ratio %.2f" % max(a[0] / max(a[2], 1e-30) for a in worst))


def test_conv2d_and_handle_errors():
    import aiod_amd
    x = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(aiod_amd.AtlasFitError, match="arguments"):
        aiod_amd.stage2.conv2d(x, np.zeros((4, 4, 5, 5), np.float32))          # k = 5
    with pytest.raises(aiod_amd.AtlasFitError, match="reflection"):
        aiod_amd.stage2.conv2d(np.zeros((3, 3, 4), np.float32), np.zeros((4, 4, 7, 7), np.float32), pad_mode=1)
    f = aiod_amd.NeuralFilter(40, 70)
    with pytest.raises(aiod_amd.AtlasFitError) as e:       # parameters not set
        f.frame(np.zeros((40, 70, 3)), np.zeros((40, 70, 3)))
    assert e.value.code == -5
    f.close()


def test_loader_errors_are_named(g2):
    import aiod_amd
    f = aiod_amd.NeuralFilter(40, 70)
    bad = dict(g2["fsd"]); del bad["upconv3.1.bias"]
    with pytest.raises(aiod_amd.StateDictError, match="missing key 'upconv3.1.bias'"):
        f.load_state_dicts(bad, g2["lsd"])
    bad = dict(g2["lsd"]); bad["extra.weight"] = torch.zeros(1)
    with pytest.raises(aiod_amd.StateDictError, match="unexpected key 'extra.weight'"):
        f.load_state_dicts(g2["fsd"], bad)
    bad = dict(g2["lsd"]); bad["deconv3.conv2d.weight"] = torch.zeros(3, 64, 3, 3)
    with pytest.raises(aiod_amd.StateDictError, match="'deconv3.conv2d.weight' has shape"):
        f.load_state_dicts(g2["fsd"], bad)
    f.close()


def test_cli_on_synthetic_tree(g2, tmp_path):
    from PIL import Image
    from oracle.cv_oracle import cv_resize_linear
    vid, n, (h, w) = "clip", 3, (40, 70)
    (tmp_path / "data" / "test" / vid).mkdir(parents=True)
    (tmp_path / "results" / vid / "stage_1" / "output").mkdir(parents=True)
    styles = []
    for t in range(n):
        Image.fromarray(g2["content"][t]).save(tmp_path / "data" / "test" / vid / ("%05d.png" % t))
        st = np.asarray(Image.fromarray(g2["style"][t]).resize((84, 48), Image.NEAREST))      # a stage-1 frame of another size
        styles.append(st)
        Image.fromarray(st).save(tmp_path / "results" / vid / "stage_1" / "output" / ("%05d.png" % t))
    torch.save(g2["fsd"], tmp_path / "f.pth")
    torch.save(g2["lsd"], tmp_path / "l.pth")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "all-in-one-deflicker_amd", "neural_filter.py"), "--video_name", vid,
                        "--ckpt_filter", "f.pth", "--ckpt_local", "l.pth", "--gpu", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    base = tmp_path / "results" / vid
    dirs = {"concat": base / "neural_filter" / "concat", "pred": base / "neural_filter" / "output", "final": base / "final" / "output"}
    for d in dirs.values():
        assert sorted(os.listdir(d)) == ["%05d.png" % t for t in range(n)]
    # the torch restatement of the script: load_image, InputPadder, the loop, tensor2img + cv2.resize, save_img
    fsd, lsd = g2["fsd"], {k: v for k, v in g2["lsd"].items() if v.is_floating_point()}
    o1 = p1 = None
    diff, total = 0, 0
    with torch.no_grad():
        for t in range(n):
            c = torch.from_numpy(g2["content"][t] / 255.0).permute(2, 0, 1)[None].float()
            s = cv_resize_linear(styles[t] / 255.0, w, h)
            s = torch.from_numpy(np.asarray(s)).permute(2, 0, 1)[None].float()
            c, s = pad_other(c), pad_other(s)
            pred = unet_ref(fsd, torch.cat((c, s), 1), {})
            if t == 0:
                o1 = p1 = final = pred
            else:
                final = pred + local_ref(lsd, torch.cat((pred, o1, pred, p1), 1), {})
                p1, o1 = pred, final
            back = [np.asarray(cv_resize_linear(v[0].permute(1, 2, 0).numpy(), w, h), np.float32) for v in (c, s, pred, final)]
            q = lambda a: (np.clip(a, 0, 1) * np.float32(255.0)).astype(np.uint8)       # noqa: E731
            expect = {"concat": q(np.concatenate(back[:3], 1)), "pred": q(back[2]), "final": q(back[3])}
            for k, d in dirs.items():
                got = np.asarray(Image.open(d / ("%05d.png" % t)))
                assert got.shape == expect[k].shape, (k, got.shape)
                dd = np.abs(got.astype(int) - expect[k].astype(int))
                assert dd.max() <= 1, (k, t, dd.max())
                diff += int((dd > 0).sum()); total += dd.size
    assert expect["concat"].shape == (h, 3 * w, 3)
    print("CLI: %d of %d uint8 values differ by one level (%.2e)" % (diff, total, diff / total))
