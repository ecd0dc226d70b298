"""The native RAFT path's precision mode "fp16" on the GPU (include/atlasfit.h: AF_RAFT_FP16, af_raft_set_precision, the *_prec building
blocks; csrc/conv_gemm_h.h, k_rconv_h): the arithmetic the reference runs on a GPU, both encoders and the update block under fp16
autocast.

Yardsticks.  The "contract twin" is tests/raft_fp16_ref.py in fp64: the mode's rounding contract with exact sums.
A single layer is held against it tightly: the kernel accumulates exact products in fp32, so it can differ from the twin only where the
fp32 sum and the fp64 sum round to different fp16 values, on well below 1 % of the outputs (on the CPU, fp32-accumulated rounding
differs from the twin on 0.10 - 0.21 % of these shapes' outputs, torch's own half convolution on 0.10 - 0.39 %).  Near-zero outputs
that differ do so by several of their own ulps, so the bound on the difference is absolute: twice torch's half convolution on the same
operands, or one fp16 ulp at the largest output.  The end-to-end tensors are held against the fp64 twin of tests/golden/raft.npz with
the project's usual rule, at most twice the error of the reference's own modules under fp16 autocast (tests/golden/raft_amp.npz,
tools/make_golden_raft_amp.py): two correct implementations of the contract differ by 1.7e-2 px after 20 iterations, so nothing
tighter is meaningful there."""
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_raft as G  # noqa: E402
import raft_fp16_ref as R16  # noqa: E402

H, W, HP, WP, H8, W8 = 130, 197, 136, 200, 17, 25
P = H8 * W8
ACT_CODE = {"none": 0, "relu": 1, "tanh": 3, "sigmoid": 4}


def stats(a, ref64):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(ref64, np.float64)).ravel()
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pc(t):
    """(1, C, h, w) tensor -> (h * w, C) float64 numpy."""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).double().numpy()


def is_fp16_valued(a):
    a = np.asarray(a, np.float32)
    return np.array_equal(a.astype(np.float16).astype(np.float32), a)


# ---- 1 - 3: single convolutions ----------------------------------------------------------------------------------------------
CONV_SHAPES = [                          # (cin, cout, kh, kw, stride, h, w) at batch 2
    (7, 5, 1, 1, 2, 9, 11),              # K < one chunk, one partial M tile, BN 32
    (12, 40, 3, 3, 1, 29, 31),           # BN 64, last M tile partial
    (33, 70, 7, 7, 2, 23, 19),           # K = 1617, not a multiple of any chunk; BN 128 with padded columns
    (384, 128, 1, 5, 1, 17, 25),         # the GRU shapes
    (384, 128, 5, 1, 1, 17, 25),
    (324, 256, 1, 1, 1, 17, 25),
    (3, 64, 7, 7, 2, 40, 56),
]


def draw_conv(shape, xscale=1.0, wscale=1.0, half=True):
    cin, cout, kh, kw, stride, h, w = shape
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + kh)
    x = torch.randn((2, cin, h, w), generator=gen) * xscale
    wt = (torch.rand((cout, cin, kh, kw), generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (cin * kh * kw))) * wscale
    b = (torch.rand((cout,), generator=gen) * 2 - 1) * 0.05 * wscale
    if half:
        x, wt, b = x.half().float(), wt.half().float(), b.half().float()
    return x, wt, b


def conv_case(name, shape, act, x, wt, b):
    """The three conditions of a single convolution; prints every figure before it asserts.  Returns the GPU's output."""
    from aiod_amd.raft import conv2d
    stride, pad = shape[4], (shape[2] // 2, shape[3] // 2)
    twin = nhwc(R16.conv(x.double(), wt.double(), b.double(), stride, pad, act)).numpy()
    th = nhwc(R16.ACTS[act](F.conv2d(x.half(), wt.half(), b.half(), stride, pad))).double().numpy()      # torch's own half convolution
    y = conv2d(nhwc(x).numpy(), wt.numpy(), b.numpy(), stride, ACT_CODE[act], precision="fp16")
    assert y.shape == twin.shape and np.isfinite(y).all() and is_fp16_valued(y)
    frac = float((y.astype(np.float64) != twin).mean())
    hm, hr = stats(y, twin)
    tm, tr = stats(th, twin)
    ulp = float(np.spacing(np.float16(np.abs(twin).max())))
    print("%-40s differ %.4f %% | hip max %.3e rms %.3e | torch half max %.3e rms %.3e (differ %.4f %%) | ulp at max %.3e"
          % (name, 100 * frac, hm, hr, tm, tr, 100 * float((th != twin).mean()), ulp))
    assert frac <= 0.01, "%s: %.3f %% of the outputs differ from the twin's fp16 value" % (name, 100 * frac)
    assert hm <= max(2.0 * tm, ulp), "%s: max |hip - twin| %.3e > max(2 x %.3e, %.3e)" % (name, hm, tm, ulp)
    assert hr <= 2.0 * tr, "%s: rms |hip - twin| %.3e > 2 x %.3e" % (name, hr, tr)
    return y


@pytest.mark.parametrize("act", ["none", "relu", "tanh", "sigmoid"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_against_the_contract_twin(shape, act):
    conv_case("conv %s %s" % (shape, act), shape, act, *draw_conv(shape))


def test_conv_subnormal_operands():
    shape = CONV_SHAPES[1]
    x, wt, b = draw_conv(shape, xscale=2.0 ** -6, wscale=2.0 ** -18)
    assert 0 < wt.abs().max() < 2.0 ** -14                      # every weight is an fp16 subnormal
    y = conv_case("conv subnormal %s" % (shape,), shape, "none", x, wt, b)
    assert np.abs(y).max() > 0 and np.abs(y).max() < 2.0 ** -14      # subnormal outputs, not flushed


def test_conv_rounds_fp32_operands_to_nearest_even():
    from aiod_amd.raft import conv2d
    shape = CONV_SHAPES[2]
    x, wt, b = draw_conv(shape, half=False)
    x[0, 0, 0, :4] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -25])      # ties: to even, and half the smallest subnormal
    assert not is_fp16_valued(x.numpy()) and not is_fp16_valued(wt.numpy()) and not is_fp16_valued(b.numpy())
    args = (shape[4], ACT_CODE["tanh"])
    y = conv2d(nhwc(x).numpy(), wt.numpy(), b.numpy(), *args, precision="fp16")
    yr = conv2d(nhwc(x.half().float()).numpy(), wt.half().float().numpy(), b.half().float().numpy(), *args, precision="fp16")
    assert np.abs(y).max() > 0 and np.array_equal(y.view(np.uint32), yr.view(np.uint32))
    y32 = conv2d(nhwc(x).numpy(), wt.numpy(), b.numpy(), *args)
    assert not np.array_equal(y, y32)                           # and the default is another arithmetic


# ---- 4: building blocks --------------------------------------------------------------------------------------------------------
def check2x(name, hip, ref64, torch_stat):
    """The project's rule; prints every figure before it asserts."""
    hm, hr = stats(hip, ref64)
    tm, tr = float(torch_stat[0]), float(torch_stat[1])
    print("%-26s hip max %.3e rms %.3e | yardstick max %.3e rms %.3e | ratio %.2f %.2f" % (name, hm, hr, tm, tr, hm / max(tm, 1e-300), hr / max(tr, 1e-300)))
    assert np.isfinite(np.asarray(hip)).all(), name
    assert hm <= 2.0 * tm, "%s: max |hip - twin| %.3e > 2 x %.3e" % (name, hm, tm)
    assert hr <= 2.0 * tr, "%s: rms |hip - twin| %.3e > 2 x %.3e" % (name, hr, tr)


def cpu_autocast():
    return torch.autocast("cpu", dtype=torch.float16)


@pytest.mark.parametrize("vertical", [0, 1])
def test_gru_half_fp16(vertical):
    from aiod_amd.raft import gru_half
    gen = torch.Generator().manual_seed(17 + vertical)
    k = (5, 1) if vertical else (1, 5)
    pad = (2, 0) if vertical else (0, 2)
    net = torch.tanh(torch.randn((2, 128, 17, 25), generator=gen)).half().float()
    x = torch.randn((2, 256, 17, 25), generator=gen).half().float()
    ws = [((torch.rand((128, 384) + k, generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (384 * 5)))).half().float() for _ in range(3)]
    bs = [((torch.rand((128,), generator=gen) * 2 - 1) * 0.05).half().float() for _ in range(3)]
    wb = [v for pair in zip(ws, bs) for v in pair]
    twin = nhwc(R16.gru_half(net.double(), x.double(), *[v.double() for v in wb], pad)).numpy()
    with torch.no_grad(), cpu_autocast():                       # the reference's SepConvGRU half on fp16 tensors
        n, xx = net.half(), x.half()
        hx = torch.cat([n, xx], 1)
        z = torch.sigmoid(F.conv2d(hx, ws[0], bs[0], 1, pad))
        r = torch.sigmoid(F.conv2d(hx, ws[1], bs[1], 1, pad))
        qq = torch.tanh(F.conv2d(torch.cat([r * n, xx], 1), ws[2], bs[2], 1, pad))
        ta = ((1 - z) * n + z * qq)
    assert ta.dtype == torch.float16
    y = gru_half(nhwc(net).numpy(), nhwc(x).numpy(), *[v.numpy() for v in wb], vertical, precision="fp16")
    assert is_fp16_valued(y)
    check2x("gru half fp16 vertical=%d" % vertical, y, twin, stats(nhwc(ta).double().numpy(), twin))


@pytest.mark.parametrize("c,relu,res", [(64, True, False), (96, False, False), (128, True, True), (64, True, True)])
def test_instance_norm_fp16(c, relu, res):
    from aiod_amd.raft import instance_norm
    gen = torch.Generator().manual_seed(c + 1)
    x = (torch.randn((1, c, 68, 100), generator=gen) * 3 + torch.randn((1, c, 1, 1), generator=gen)).half().float()
    r = torch.randn((1, c, 68, 100), generator=gen).half().float() if res else None
    twin = nhwc(R16.norm_store(F.instance_norm(x.double(), eps=1e-5), relu, None if r is None else r.double())).numpy()[0]
    with torch.no_grad(), cpu_autocast():                       # what the next autocast convolution would receive: the result as fp16
        t = F.instance_norm(x.half(), eps=1e-5)
        if relu:
            t = torch.relu(t)
        if res:
            t = torch.relu(r.half() + t)
        t = t.half()
    y = instance_norm(nhwc(x).numpy()[0], relu, None if r is None else nhwc(r).numpy()[0], precision="fp16")
    assert is_fp16_valued(y)
    check2x("instance norm fp16 c=%d" % c, y, twin, stats(nhwc(t).double().numpy()[0], twin))


# ---- 5 - 7: the network ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "raft.npz")))
    amp = np.load(os.path.join(ROOT, "tests", "golden", "raft_amp.npz"))
    for k in ("up12", "up21", "lo12", "lo21"):
        d[k] = d[k + "_hi"].astype(np.float64) + d[k + "_lo"].astype(np.float64) / G.LO_SCALE
    sd = {}
    for k, r in zip(d["keys"], d["shapes"]):
        shape = tuple(int(v) for v in r if v >= 0)
        sd[str(k)] = torch.zeros(shape, dtype=torch.int64 if str(k).endswith("num_batches_tracked") else torch.float32)
    G.synthetic_state_dict(sd)
    d["sd"] = sd
    d["sd64"] = {k: v.double() for k, v in sd.items()}
    d["err32"] = {str(n): e for n, e in zip(d["names"], d["err32"])}
    d["err16"] = {str(n): e for n, e in zip(amp["names"], amp["err16"])}
    d["im"] = [G.pad_sintel(G.to_nchw(d["im1"])), G.pad_sintel(G.to_nchw(d["im2"]))]
    return d


@pytest.fixture(scope="module")
def twin(g):
    """The fp64 restatement: intermediates of iteration 1 of direction 1 -> 2, held against the fixture's stored 1/8 flow."""
    torch.set_num_threads(8)
    acts = {}
    lo, _ = G.raft_forward(g["sd64"], g["im"][0].double(), g["im"][1].double(), iters=1, acts=acts)
    assert np.abs(lo[0].permute(1, 2, 0).numpy() - g["lo12"][0]).max() < 1e-9
    return acts


@pytest.fixture(scope="module")
def raft16(g):
    import aiod_amd
    r = aiod_amd.RAFT(H, W, capacity=2, precision="fp16")
    r.load_state_dict({"module." + k: v for k, v in g["sd"].items()})
    r.encode(0, g["im1"])
    r.encode(1, g["im2"])
    yield r
    r.close()


@pytest.fixture(scope="module")
def flows16(raft16):
    """The saved flows of both directions in fp16, computed once."""
    return raft16.flow_slots([(0, 1), (1, 0)], iters=20)


def test_end_to_end_against_the_reference_autocast_error(g, raft16, twin):
    failed = []

    def check(name, hip, ref64, key):
        hm, hr = stats(hip, ref64)
        em, er = g["err16"][key]
        ok = bool(np.isfinite(np.asarray(hip)).all()) and hm <= 2.0 * em and hr <= 2.0 * er
        print("%-14s hip max %.3e rms %.3e | reference autocast max %.3e rms %.3e | ratio %.2f %.2f%s" % (name, hm, hr, em, er, hm / em, hr / er, "" if ok else "  FAIL"))
        if not ok:
            failed.append(name)
    up, lo = raft16.flow_slots([(0, 1)], iters=1, want_lo=True)
    for name in ("fmap1", "fmap2", "net0", "inp", "corr_l0", "corr_l1", "corr_l2", "corr_l3", "motion", "net", "delta", "mask"):
        check(name, raft16.activation(name), pc(twin[name]), name)
    check("corr_vol", raft16.activation("corr_vol0"), twin["corr_vol"][0].reshape(P, -1).numpy(), "corr_vol")
    for k, iters in enumerate(G.ITERS):
        up, lo = raft16.flow_slots([(0, 1), (1, 0)], iters=iters, want_lo=True)
        check("lo12 after %d" % iters, lo[0], g["lo12"][k], "lo12_%d" % iters)
        check("lo21 after %d" % iters, lo[1], g["lo21"][k], "lo21_%d" % iters)
    assert up.shape == (2, HP, WP, 2)
    check("up12", up[0], g["up12"], "up12")
    check("up21", up[1], g["up21"], "up21")
    # the teacher-forced step: the twin's state after 11 iterations, the hidden state rounded to fp16 (as the call itself rounds it)
    st = G.teacher_state(g["sd64"], g["im"][0], g["im"][1])
    st16 = (st[0].half().float(), st[1])
    n64, d64 = G.teacher_step(g["sd64"], g["im"][0], g["im"][1], st16)
    net, delta = raft16.step(0, 1, pc(st[0]).astype(np.float32), pc(st[1]).astype(np.float32))
    net_r, delta_r = raft16.step(0, 1, pc(st16[0]).astype(np.float32), pc(st16[1]).astype(np.float32))
    assert np.array_equal(net, net_r) and np.array_equal(delta, delta_r)          # the upload rounds the state
    check("step net", net, pc(n64), "step_net")
    check("step delta", delta, pc(d64), "step_delta")
    assert not failed, failed


def test_the_mode_is_real_and_deterministic(g, raft16, flows16):
    import aiod_amd
    r32 = aiod_amd.RAFT(H, W, capacity=2)
    try:
        r32.load_state_dict(g["sd"])
        r32.encode(0, g["im1"]); r32.encode(1, g["im2"])
        up32 = r32.flow_slots([(0, 1), (1, 0)], iters=20)
    finally:
        r32.close()
    for i, name in enumerate(("up12", "up21")):
        d = float(np.abs(flows16[i] - up32[i]).max())
        print("%s: max |fp16 - fp32| %.3e, err32 max %.3e" % (name, d, g["err32"][name][0]))
        assert d > 10.0 * g["err32"][name][0]
    assert np.isfinite(flows16).all()
    np.testing.assert_array_equal(raft16.flow_slots([(0, 1), (1, 0)], iters=20), flows16)         # two runs
    raft16.encode(2, g["im1"]); raft16.encode(3, g["im2"])                                        # cached against freshly encoded frames
    np.testing.assert_array_equal(raft16.flow_slots([(2, 3), (3, 2)], iters=20), flows16)
    one = aiod_amd.RAFT(H, W, capacity=1, precision="fp16")                                       # capacity 1: one direction per launch
    try:
        one.load_state_dict(g["sd"])
        got = list(one.clip([g["im1"], g["im2"]]))
    finally:
        one.close()
    np.testing.assert_array_equal(got[0][1], flows16[0])
    np.testing.assert_array_equal(got[0][2], flows16[1])


def test_fp16_activations_are_fp16_values(raft16):
    raft16.flow_slots([(0, 1)], iters=3)
    for name in ("fmap1", "fmap2", "net0", "inp", "net", "delta", "mask"):
        a = raft16.activation(name)
        assert np.abs(a).max() > 0 and is_fp16_valued(a), name
    motion = raft16.activation("motion")
    assert is_fp16_valued(motion[:, :126])
    # the last two channels are the flow, fp32 in the reference too (torch.cat promotes); its consumers round it as they gather it
    assert np.abs(motion[:, 126:]).max() > 0 and not is_fp16_valued(motion[:, 126:])


def test_switching_precision_on_one_handle(g):
    import aiod_amd
    from aiod_amd.atlasfit import AtlasFitError
    r = aiod_amd.RAFT(H, W, capacity=1)
    try:
        r.load_state_dict(g["sd"])
        prec = ctypes.c_int(-1)
        assert r.lib.af_raft_get_precision(r.r, ctypes.byref(prec)) == 0 and prec.value == 0 and r.precision == "fp32"
        first = r.flow(g["im1"], g["im2"])
        r.set_precision("fp16")
        assert r.lib.af_raft_get_precision(r.r, ctypes.byref(prec)) == 0 and prec.value == 1 and r.precision == "fp16"
        with pytest.raises(AtlasFitError, match="a slot has no encoded frame") as e:      # the slots were invalidated
            r.flow_slots([(0, 1)])
        assert e.value.code == -5
        half = r.flow(g["im1"], g["im2"])
        assert not np.array_equal(half, first)
        r.set_precision("fp32")
        with pytest.raises(AtlasFitError, match="a slot has no encoded frame"):
            r.flow_slots([(0, 1)])
        np.testing.assert_array_equal(r.flow(g["im1"], g["im2"]), first)
        assert r.lib.af_raft_set_precision(r.r, 2) == -1                                   # AF_EINVAL, with a message
        assert b"precision must be" in r.lib.af_last_error(None)
        assert r.lib.af_raft_get_precision(r.r, ctypes.byref(prec)) == 0 and prec.value == 0
        np.testing.assert_array_equal(r.flow_slots([(0, 1)])[0], first)                    # a refused value changes nothing
        with pytest.raises(ValueError):
            r.set_precision("bf16")
    finally:
        r.close()
    x = np.zeros((1, 4, 4, 3), np.float32)
    y = np.zeros((1, 4, 4, 2), np.float32)
    w = np.zeros((2, 3, 1, 1), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert r.lib.af_raft_conv2d_prec(2, 0, p(x), 1, 4, 4, 3, p(w), None, 2, 1, 1, 1, 0, p(y)) == -1
    assert b"af_raft_conv2d_prec: precision must be" in r.lib.af_last_error(None)


# ---- 8: pipelines ----------------------------------------------------------------------------------------------------------------
DOWN, SEED = 4, 11                       # tests/test_gpu_deflicker.py's clip, config and seed
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(str(c) for c in cmd) + "\n" + r.stdout[-2000:] + r.stderr[-3000:]
    return r


def _npy_bytes(a):
    buf = io.BytesIO()
    np.save(buf, np.asarray(a, np.float32))
    return buf.getvalue()


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    import aiod_amd
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("fp16_pipeline")
    weights = PB.synthetic_weights()
    paths = PB.write_weights(str(d / "weights"), weights)
    with open(d / "short.json", "w") as f:
        json.dump(dict(REFERENCE_CONFIG, **SHORT), f)
    frames = PB.synthetic_clip(3, H, W, seed=5)                   # the fixture clip of tests/test_gpu_deflicker.py, its first frames
    r = aiod_amd.RAFT(H, W, capacity=2, precision="fp16")
    try:
        r.load_state_dict(weights[0])
        expect = [(f12.copy(), f21.copy()) for _, f12, f21 in r.clip(frames)]
    finally:
        r.close()
    return {"dir": d, "paths": paths, "cfg": str(d / "short.json"), "frames": frames, "expect": expect, "down": DOWN, "seed": SEED}


def _flow_files(folder, n):
    names = ["%05d.png" % i for i in range(n)]
    return [(folder / ("%s_%s.npy" % (names[i], names[i + 1])), folder / ("%s_%s.npy" % (names[i + 1], names[i]))) for i in range(n - 1)]


def test_precompute_cli_writes_the_fp16_flows(clip, tmp_path):
    import pipeline_bench as PB
    PB.write_clip(str(tmp_path / "data" / "test" / "clip"), clip["frames"])
    _run([sys.executable, os.path.join(PB.PKG, "preprocess_optical_flow.py"), "--vid-path", os.path.join("data", "test", "clip"), "--model", clip["paths"][0],
          "--gpu", "0", "--flow_precision", "fp16"], tmp_path)
    folder = tmp_path / "data" / "test" / "clip_flow"
    assert len(os.listdir(folder)) == 2 * (len(clip["frames"]) - 1)
    for (p12, p21), (f12, f21) in zip(_flow_files(folder, len(clip["frames"])), clip["expect"]):
        assert p12.read_bytes() == _npy_bytes(f12) and p21.read_bytes() == _npy_bytes(f21)


@pytest.mark.parametrize("precision", ["fp16", None])
def test_deflicker_cli_flow_precision(clip, tmp_path, precision):
    import pipeline_bench as PB
    PB.write_clip(str(tmp_path / "data" / "test" / "clip"), clip["frames"])
    out = tmp_path / "out"
    extra = ["--keep_intermediates"] + (["--flow_precision", precision] if precision else [])
    _run(PB.in_process_command(str(tmp_path / "data" / "test" / "clip"), str(out), clip["cfg"], clip["down"], clip["seed"], clip["paths"], extra=extra), tmp_path)
    rec = json.load(open(out / "deflicker.json"))
    assert rec["flow_precision"] == (precision or "fp32")
    folder = tmp_path / "data" / "test" / "clip_flow"
    same = [p12.read_bytes() == _npy_bytes(f12) and p21.read_bytes() == _npy_bytes(f21)
            for (p12, p21), (f12, f21) in zip(_flow_files(folder, len(clip["frames"])), clip["expect"])]
    assert len(same) == len(clip["frames"]) - 1
    assert all(same) if precision == "fp16" else not any(same)      # exactly the fp16 flows with the flag, other flows without it
