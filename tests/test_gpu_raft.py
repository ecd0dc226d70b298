"""The native RAFT forward on the GPU (include/atlasfit.h: af_raft_*) against tests/golden/raft.npz, which tools/make_golden_raft.py
computed with the reference's own RAFT modules on the CPU (fp32 and an fp64 twin).

Rule (the project's usual one): for every compared tensor, max and rms of |hip - fp64 twin| are each at most twice the same statistic
of |torch fp32 - fp64 twin|.  For the end-to-end tensors the torch statistic is the one recorded in the fixture (the reference's
modules); for the stand-alone building blocks it is measured here with torch on the CPU on the same inputs.  The twins of the named
intermediates are too large to store: they come from the generator's functional restatement in fp64, which `twin` first holds
against the fixture's stored flows."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft.npz")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_raft as G  # noqa: E402

H, W, HP, WP, H8, W8 = 130, 197, 136, 200, 17, 25
P = H8 * W8


def stats(a, ref64):
    d = np.abs(np.asarray(a, np.float64) - ref64).ravel()
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


def check(name, hip, ref64, torch_stat):
    """The rule; prints every figure before it asserts."""
    hm, hr = stats(hip, ref64)
    tm, tr = float(torch_stat[0]), float(torch_stat[1])
    print("%-22s hip max %.3e rms %.3e | torch fp32 max %.3e rms %.3e | ratio %.2f %.2f" % (name, hm, hr, tm, tr, hm / max(tm, 1e-300), hr / max(tr, 1e-300)))
    assert np.isfinite(np.asarray(hip)).all(), name
    assert hm <= 2.0 * tm, "%s: max |hip - fp64| %.3e > 2 x %.3e" % (name, hm, tm)
    assert hr <= 2.0 * tr, "%s: rms |hip - fp64| %.3e > 2 x %.3e" % (name, hr, tr)


def pc(t):
    """(1, C, h, w) tensor -> (h * w, C) float64 numpy."""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).double().numpy()


@pytest.fixture(scope="module")
def g():
    d = dict(np.load(GOLDEN))
    for k in ("up12", "up21", "lo12", "lo21"):
        d[k] = d[k + "_hi"].astype(np.float64) + d[k + "_lo"].astype(np.float64) / G.LO_SCALE
    sd = {}
    for k, r in zip(d["keys"], d["shapes"]):
        shape = tuple(int(v) for v in r if v >= 0)
        sd[str(k)] = torch.zeros(shape, dtype=torch.int64 if str(k).endswith("num_batches_tracked") else torch.float32)
    G.synthetic_state_dict(sd)
    d["sd"] = sd
    d["sd64"] = {k: v.double() for k, v in sd.items()}
    d["err"] = {str(n): e for n, e in zip(d["names"], d["err32"])}
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
def raft(g):
    import aiod_amd
    r = aiod_amd.RAFT(H, W, capacity=2)
    r.load_state_dict({"module." + k: v for k, v in g["sd"].items()})
    r.encode(0, g["im1"])
    r.encode(1, g["im2"])
    yield r
    r.close()


# ---- building blocks, stand-alone against torch -------------------------------------------------------------------------
RECT_CASES = [(1, 5, 384, 128, 4), (5, 1, 384, 128, 3), (1, 5, 20, 40, 0), (5, 1, 33, 2, 1), (3, 3, 16, 96, 4)]      # (kh, kw, cin, cout, act); tools/conv_paths_digest.py reads them


@pytest.mark.parametrize("kh,kw,cin,cout,act", RECT_CASES)
def test_rect_conv(kh, kw, cin, cout, act):
    from aiod_amd.raft import conv2d
    gen = torch.Generator().manual_seed(100 * kh + kw + cin)
    x = torch.randn((2, cin, 19, 27), generator=gen)
    wt = (torch.rand((cout, cin, kh, kw), generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (cin * kh * kw)))
    b = (torch.rand((cout,), generator=gen) * 2 - 1) * 0.05
    fn = {0: lambda v: v, 1: torch.relu, 3: torch.tanh, 4: torch.sigmoid}[act]
    y32 = fn(F.conv2d(x, wt, b, 1, (kh // 2, kw // 2)))
    y64 = fn(F.conv2d(x.double(), wt.double(), b.double(), 1, (kh // 2, kw // 2))).permute(0, 2, 3, 1).numpy()
    y = conv2d(x.permute(0, 2, 3, 1).numpy(), wt.numpy(), b.numpy(), act=act)
    check("conv %dx%d act %d" % (kh, kw, act), y, y64, stats(y32.permute(0, 2, 3, 1).numpy(), y64))


@pytest.mark.parametrize("cin,cout,k,stride,act,h,w", [
    (7, 5, 1, 2, 0, 9, 11),             # M = 30 in one partial tile, K = 7 < 16, BN 32
    (12, 40, 3, 1, 1, 29, 31),          # BN 64, last M tile partial
    (33, 70, 7, 2, 3, 23, 19),          # BN 128 with 58 padded columns, K = 1617, not a multiple of 16
    (128, 128, 3, 1, 1, 16, 24),        # exact tiles
])
def test_one_core_stage2_and_raft_routes_bitwise(cin, cout, k, stride, act, h, w):
    """k_conv and k_rconv are two instantiations of one tile function (csrc/conv_gemm.h): a square zero-padded convolution gives the
    same bits through either (both form sum + bias; RAFT's output scale is exactly 1)."""
    import aiod_amd
    g = torch.Generator().manual_seed(1000 * cin + cout)
    x = (torch.rand(h, w, cin, generator=g, dtype=torch.float64) * 2 - 1).float().numpy()
    wt = ((torch.rand(cout, cin, k, k, generator=g, dtype=torch.float64) * 2 - 1) * np.sqrt(6.0 / (cin * k * k))).float().numpy()
    b = ((torch.rand(cout, generator=g, dtype=torch.float64) - 0.5) * 0.1).float().numpy()
    y2 = aiod_amd.stage2.conv2d(x, wt, b, stride, 0, act)
    yr = aiod_amd.raft.conv2d(x[None], wt, b, stride, act)[0]
    assert y2.shape == yr.shape == ((h - 1) // stride + 1, (w - 1) // stride + 1, cout)
    assert np.isfinite(y2).all() and np.abs(y2).max() > 0
    assert np.array_equal(y2, yr)


@pytest.mark.parametrize("vertical", [0, 1])
def test_gru_half(vertical):
    from aiod_amd.raft import gru_half
    gen = torch.Generator().manual_seed(7 + vertical)
    k = (5, 1) if vertical else (1, 5)
    pad = (2, 0) if vertical else (0, 2)
    net = torch.tanh(torch.randn((2, 128, 17, 25), generator=gen))
    x = torch.randn((2, 256, 17, 25), generator=gen)
    ws = [(torch.rand((128, 384) + k, generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (384 * 5))) for _ in range(3)]
    bs = [(torch.rand((128,), generator=gen) * 2 - 1) * 0.05 for _ in range(3)]

    def ref(dt):
        n, xx = net.to(dt), x.to(dt)
        w_, b_ = [v.to(dt) for v in ws], [v.to(dt) for v in bs]
        hx = torch.cat([n, xx], 1)
        z = torch.sigmoid(F.conv2d(hx, w_[0], b_[0], 1, pad))
        r = torch.sigmoid(F.conv2d(hx, w_[1], b_[1], 1, pad))
        q = torch.tanh(F.conv2d(torch.cat([r * n, xx], 1), w_[2], b_[2], 1, pad))
        return ((1 - z) * n + z * q).permute(0, 2, 3, 1).double().numpy()
    y64 = ref(torch.float64)
    y = gru_half(net.permute(0, 2, 3, 1).numpy(), x.permute(0, 2, 3, 1).numpy(), ws[0].numpy(), bs[0].numpy(), ws[1].numpy(), bs[1].numpy(),
                 ws[2].numpy(), bs[2].numpy(), vertical)
    check("gru half vertical=%d" % vertical, y, y64, stats(ref(torch.float32), y64))


@pytest.mark.parametrize("c,relu,res", [(64, True, False), (96, False, False), (128, True, True), (64, True, True)])
def test_instance_norm(c, relu, res):
    from aiod_amd.raft import instance_norm
    gen = torch.Generator().manual_seed(c)
    x = torch.randn((1, c, 68, 100), generator=gen) * 3 + torch.randn((1, c, 1, 1), generator=gen)
    r = torch.randn((1, c, 68, 100), generator=gen) if res else None

    def ref(dt):
        y = F.instance_norm(x.to(dt), eps=1e-5)
        if relu:
            y = torch.relu(y)
        if res:
            y = torch.relu(r.to(dt) + y)
        return y[0].permute(1, 2, 0).double().numpy()
    y64 = ref(torch.float64)
    y = instance_norm(x[0].permute(1, 2, 0).numpy(), relu, None if r is None else r[0].permute(1, 2, 0).numpy())
    check("instance norm c=%d" % c, y, y64, stats(ref(torch.float32), y64))


# ---- correlation: volume, pyramid, lookup -------------------------------------------------------------------------------
def test_corr_volume_and_pyramid(g, raft, twin):
    raft.lookup(0, 1, G.coords_grid(H8, W8, torch.float32)[0].permute(1, 2, 0).numpy())
    vol64 = twin["corr_vol"][0]                                   # (P, h, w)
    check("corr volume", raft.activation("corr_vol0"), vol64.reshape(P, -1).numpy(), g["err"]["corr_vol"])
    # the pooling alone: each level from the level the GPU itself wrote, torch fp32 on the same input as the yardstick
    for l in (1, 2, 3):
        src = torch.from_numpy(raft.activation("corr_vol%d" % (l - 1))).reshape(P, 1, H8 >> (l - 1), W8 >> (l - 1))
        p64 = F.avg_pool2d(src.double(), 2, stride=2).reshape(P, -1).numpy()
        p32 = F.avg_pool2d(src, 2, stride=2).reshape(P, -1).numpy()
        hip = raft.activation("corr_vol%d" % l)
        assert hip.shape[1] == (H8 >> l) * (W8 >> l)
        check("pyramid level %d" % l, hip, p64, stats(p32, p64))


def _lookup_case(raft, coords, name):
    """The lookup alone: HIP against torch on the pyramid the GPU itself built."""
    out = raft.lookup(0, 1, coords)
    pyr32 = [torch.from_numpy(raft.activation("corr_vol%d" % l)).reshape(P, 1, H8 >> l, W8 >> l) for l in range(4)]
    c = torch.from_numpy(coords.reshape(H8, W8, 2)).permute(2, 0, 1)[None]
    r64 = pc(G.corr_lookup([v.double() for v in pyr32], c.double()))
    r32 = pc(G.corr_lookup(pyr32, c))
    for l in range(4):
        sl = slice(81 * l, 81 * (l + 1))
        check("%s level %d" % (name, l), out[:, sl], r64[:, sl], stats(r32[:, sl], r64[:, sl]))
        np.testing.assert_array_equal(raft.activation("corr_l%d" % l), out[:, sl])


def test_lookup_fractional(raft):
    rng = np.random.default_rng(5)
    base = G.coords_grid(H8, W8, torch.float32)[0].permute(1, 2, 0).numpy()
    _lookup_case(raft, (base + rng.uniform(-3, 3, base.shape)).astype(np.float32), "lookup fractional")


def test_lookup_integer_positions(raft):
    base = G.coords_grid(H8, W8, torch.float32)[0].permute(1, 2, 0).numpy()
    rng = np.random.default_rng(6)
    _lookup_case(raft, (base + rng.integers(-2, 3, base.shape)).astype(np.float32), "lookup integer")


def test_lookup_outside_the_map(raft):
    rng = np.random.default_rng(7)
    c = rng.uniform(-40, 70, (H8, W8, 2)).astype(np.float32)         # most taps of most levels fall outside: zeros
    c[0, 0] = (-1.0, -1.0); c[0, 1] = (W8 - 1.0, H8 - 1.0); c[0, 2] = (W8, H8); c[0, 3] = (-5.0, 3.25); c[0, 4] = (1e6, -1e6)
    _lookup_case(raft, c, "lookup outside")


# ---- the network --------------------------------------------------------------------------------------------------------
def test_iteration_one_intermediates(g, raft, twin):
    up, lo = raft.flow_slots([(0, 1)], iters=1, want_lo=True)
    for name in ("fmap1", "fmap2", "net0", "inp", "corr_l0", "corr_l1", "corr_l2", "corr_l3", "motion", "net", "delta", "mask"):
        check(name, raft.activation(name), pc(twin[name]), g["err"][name])
    check("lo12 after 1", lo[0], g["lo12"][0], g["err"]["lo12_1"])


def test_teacher_forced_step(g, raft):
    st = G.teacher_state(g["sd64"], g["im"][0], g["im"][1])
    n64, d64 = G.teacher_step(g["sd64"], g["im"][0], g["im"][1], st)
    net, delta = raft.step(0, 1, pc(st[0]).astype(np.float32), pc(st[1]).astype(np.float32))
    check("step net", net, pc(n64), g["err"]["step_net"])
    check("step delta", delta, pc(d64), g["err"]["step_delta"])


@pytest.mark.parametrize("k,iters", list(enumerate(G.ITERS)))
def test_low_resolution_flow(g, raft, k, iters):
    up, lo = raft.flow_slots([(0, 1), (1, 0)], iters=iters, want_lo=True)
    check("lo12 after %d" % iters, lo[0], g["lo12"][k], g["err"]["lo12_%d" % iters])
    check("lo21 after %d" % iters, lo[1], g["lo21"][k], g["err"]["lo21_%d" % iters])
    if iters == 20:
        assert up.shape == (2, HP, WP, 2)
        check("up12", up[0], g["up12"], g["err"]["up12"])
        check("up21", up[1], g["up21"], g["err"]["up21"])


def test_bitwise_cached_fresh_repeat_and_capacity(g, raft):
    import aiod_amd
    both = raft.flow_slots([(0, 1), (1, 0)], iters=20)
    again = raft.flow_slots([(0, 1), (1, 0)], iters=20)
    np.testing.assert_array_equal(both, again)                        # two runs
    raft.encode(2, g["im1"]); raft.encode(3, g["im2"])                # freshly encoded frames in other slots
    np.testing.assert_array_equal(raft.flow_slots([(2, 3), (3, 2)], iters=20), both)
    np.testing.assert_array_equal(raft.flow(g["im1"], g["im2"]), both[0])
    one = aiod_amd.RAFT(H, W, capacity=1)                             # batch capacity 1: one direction per launch
    try:
        one.load_state_dict(g["sd"])
        got = list(one.clip([g["im1"], g["im2"]]))
    finally:
        one.close()
    assert len(got) == 1 and got[0][0] == 0
    np.testing.assert_array_equal(got[0][1], both[0])
    np.testing.assert_array_equal(got[0][2], both[1])
    clip = list(raft.clip([g["im1"], g["im2"], g["im1"]]))            # capacity 2, frames encoded once
    np.testing.assert_array_equal(clip[0][1], both[0]); np.testing.assert_array_equal(clip[0][2], both[1])
    np.testing.assert_array_equal(clip[1][1], both[1]); np.testing.assert_array_equal(clip[1][2], both[0])


def test_device_pointers_bitwise_equal_host_pointers(g, raft):
    """af_raft_encode / af_raft_flow with on_device = 1 (CUDA tensors in, CUDA tensors out) against the host-pointer calls."""
    host_up, host_lo = raft.flow_slots([(0, 1), (1, 0)], iters=4, want_lo=True)
    dev = torch.device("cuda:0")
    raft.encode(2, torch.from_numpy(g["im1"].astype(np.float32)).to(dev))
    raft.encode(3, torch.from_numpy(g["im2"].astype(np.float32)).to(dev))
    up, lo = raft.flow_slots([(2, 3), (3, 2)], iters=4, want_lo=True, on_device=True)
    assert up.is_cuda and lo.is_cuda and tuple(up.shape) == (2, HP, WP, 2) and tuple(lo.shape) == (2, H8, W8, 2)
    np.testing.assert_array_equal(up.cpu().numpy(), host_up)
    np.testing.assert_array_equal(lo.cpu().numpy(), host_lo)
    only_up = raft.flow_slots([(0, 1)], iters=4, on_device=True)             # the optional 1/8 output left out
    np.testing.assert_array_equal(only_up.cpu().numpy()[0], host_up[0])


def test_size_limit_and_state_errors(g):
    import aiod_amd
    from aiod_amd.atlasfit import AtlasFitError
    for h, w in ((64, 96), (120, 300), (300, 113)):
        with pytest.raises(AtlasFitError) as e:
            aiod_amd.RAFT(h, w)
        assert e.value.code == -1 and "128" in str(e.value)
    r = aiod_amd.RAFT(121, 128, capacity=1)                           # pads to exactly 128 x 128: accepted
    try:
        assert (r.Hp, r.Wp) == (128, 128)
        with pytest.raises(AtlasFitError) as e:
            r.encode(0, np.zeros((121, 128, 3), np.float32))
        assert e.value.code == -5
        with pytest.raises(AtlasFitError) as e:
            r.flow_slots([(0, 1)])
        assert e.value.code == -5
        r.load_state_dict(g["sd"])
        with pytest.raises(AtlasFitError) as e:                       # parameters set, but no frame encoded
            r.flow_slots([(0, 1)])
        assert e.value.code == -5
        with pytest.raises(AtlasFitError) as e:
            r.flow_slots([(0, 1), (1, 0)])                            # over the capacity
        assert e.value.code == -1
    finally:
        r.close()
