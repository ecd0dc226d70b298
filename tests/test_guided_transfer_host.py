"""Host-side checks of the proxy route (no GPU): the numpy restatement of the residual guided transfer (tests/guided_transfer_ref.py) that
the GPU tests hold the kernels to, against its definition and its fp64 twin, and `Deflicker(proxy_long_edge=...)` with the stub engines of
tests/test_deflicker_host.py (imported, not edited), the CLI flags and the refusals that need no device.

The bounds against the twin.  Output: the restatement and the twin round values that differ by far less than one level (the planes differ
by ~1e-7 and ~1e-5, below), so their bytes differ by at most 1, and only where the real value lies next to a rounding boundary.  Planes:
measured here on the GPU tests' inputs (MEASUREMENTS.md Part X): max |abar - abar64| = 2.4986e-07, max |bbar - bbar64| = 3.5991e-05, both
on the random-byte case; the asserted bounds are twice those."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_transfer_ref as R  # noqa: E402
import test_deflicker_host as TD  # noqa: E402      (the stub engines of the one-process pipeline)

MEASURED_A, MEASURED_B = 2.4985526603238384e-07, 3.599137346554926e-05
BOUND_A, BOUND_B = 2 * MEASURED_A, 2 * MEASURED_B


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in R.CASES:
        full, i, p, r = R.make_case(name)
        out[name] = (full, i, p, r, R.coeffs(i, p, r, R.EPS), R.coeffs64(i, p, r, R.EPS))
    return out


# ---- the restatement against its definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 8, 32])
def test_identity_returns_the_frame(r):
    full, i, _, _ = R.make_case("ratio")
    a, b = R.coeffs(i, i, r, R.EPS)
    assert not a.any() and not b.any()
    assert np.array_equal(R.apply(full, a, b), full)


@pytest.mark.parametrize("c", [-37, 1, 60])
@pytest.mark.parametrize("r", [1, 8, 32])
def test_constant_offset_is_carried_exactly(r, c):
    rng = np.random.RandomState(r + 100 + c)
    full = rng.randint(70, 186, (75, 106, 3)).astype(np.uint8)           # nothing clips: 70 - 37 >= 0, 185 + 60 <= 255
    i = R.area_shrink(full, 37, 53)
    p = (i.astype(np.int64) + c).astype(np.uint8)
    a, b = R.coeffs(i, p, r, R.EPS)
    assert not a.any() and np.array_equal(b, np.full(b.shape, c, np.float32))
    assert np.array_equal(R.apply(full, a, b).astype(np.int64), full.astype(np.int64) + c)


def test_an_edge_is_followed_better_than_bilinear_upsampling():
    """A two-region guide, 50 | 200, the edge between proxy columns 15 and 16 (full columns 31 and 32 at ratio 2); the residual is +10
    left of it and -10 right of it.  The exact full-size answer is F + 10 | F - 10.  Plain bilinear upsampling of d smears the step over
    the full-size pixels next to the edge; the guided transfer follows the guide."""
    h, w, H, W = 24, 32, 48, 64
    i = np.full((h, w, 3), 50, np.uint8)
    i[:, 16:] = 200
    d = np.where(np.arange(w) < 16, 10, -10)[None, :, None]
    p = (i.astype(np.int64) + d).astype(np.uint8)
    full = np.full((H, W, 3), 50, np.uint8)
    full[:, 32:] = 200
    exact = full.astype(np.int64) + np.where(np.arange(W) < 32, 10, -10)[None, :, None]
    guided = R.transfer(full, i, p, 8, R.EPS).astype(np.int64)
    zero = np.zeros((h, w, 3), np.float32)
    plain = R.apply(full, zero, np.broadcast_to(d, (h, w, 3)).astype(np.float32)).astype(np.int64)      # a = 0, b = d: bilinear d
    edge = slice(30, 34)
    err_guided, err_plain = np.abs(guided - exact)[:, edge].max(), np.abs(plain - exact)[:, edge].max()
    print("edge error: guided %d, bilinear %d" % (err_guided, err_plain))
    assert err_plain > 0 and err_guided < err_plain
    assert np.abs(guided - exact).max() <= np.abs(plain - exact).max()


def test_restatement_is_within_one_level_of_the_fp64_twin(cases):
    for name, (full, i, p, r, (a, b), _) in cases.items():
        out, twin = R.apply(full, a, b), R.transfer64(full, i, p, r, R.EPS)
        assert np.abs(out.astype(np.int64) - twin.astype(np.int64)).max() <= 1, name


def test_coefficient_planes_against_the_fp64_twin(cases):
    worst_a = worst_b = 0.0
    for name, (_, _, _, _, (a, b), (a64, b64)) in cases.items():
        assert a.dtype == np.float32 and b.dtype == np.float32
        worst_a, worst_b = max(worst_a, np.abs(a - a64).max()), max(worst_b, np.abs(b - b64).max())
    print("max |abar - abar64| = %.4e (bound %.4e), max |bbar - bbar64| = %.4e (bound %.4e)" % (worst_a, BOUND_A, worst_b, BOUND_B))
    assert worst_a <= BOUND_A and worst_b <= BOUND_B


def test_the_largest_sums_fit_int32():
    """I = 255, P = 0 at r = 32 on a proxy that holds a whole window: S_II = 4225 * 255^2, the figure the kernel's int32 planes are sized by."""
    _, i, p, r = R.make_case("extreme")
    assert r == 32 and i.shape[0] >= 65 and i.shape[1] >= 65
    a, b, n = R.raw_coeffs(i, p, r, R.EPS)      # asserts every sum < 2^31
    assert n.max() == 4225 and 4225 * 255 * 255 == 274730625 < 2 ** 31
    assert not a.any() and np.array_equal(b, np.full(b.shape, -255, np.float32))


# ---- python-side refusals that need no device --------------------------------------------------------------------------------------
def test_python_refusals():
    import aiod_amd
    from aiod_amd import guided as G
    img = np.zeros((4, 6, 3), np.uint8)
    assert G.DEFAULT_RADIUS == 8 and G.DEFAULT_EPS == aiod_amd.DEFAULT_EPS > 0
    for name in ("guided_transfer", "guided_transfer_device", "guided_coeffs", "guided_coeffs_device"):
        assert getattr(aiod_amd, name) is getattr(G, name)
    for bad in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match="radius must be an integer in 1..32"):
            G.guided_transfer(img, img, img, radius=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, "x"):
        with pytest.raises(ValueError, match="eps must be"):
            G.guided_coeffs(img, img, eps=bad)
    with pytest.raises(ValueError, match="proxy_in is 6x4, proxy_out 5x4"):
        G.guided_transfer(img, img, img[:, :5])
    with pytest.raises(ValueError, match=r"the proxy \(6x4\) is larger than the full frame \(6x3\)"):
        G.guided_transfer(img[:3], img, img)
    with pytest.raises(ValueError, match=r"full must be \(H, W, 3\) uint8"):
        G.guided_transfer(img.astype(np.float32), img, img)
    with pytest.raises(ValueError, match="must be CUDA tensors"):
        G.guided_transfer_device(img, img, img)


def test_abi_refusals_come_before_the_device():
    """The handle-free wrappers refuse bad arguments by name before any HIP call, so this runs without a GPU."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    import aiod_amd
    lib = aiod_amd.load_library()
    u8 = np.zeros((4, 6, 3), np.uint8)
    f32 = [np.zeros((4, 6, 3), np.float32) for _ in range(2)]
    big = np.zeros((8, 12, 3), np.uint8)
    out = np.zeros((8, 12, 3), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def coeffs(h=4, w=6, r=8, eps=64.0, i=u8, a=f32[0], b=f32[1]):
        return lib.af_guided_coeffs(0, ptr(i) if i is not None else None, ptr(u8), h, w, r, eps, ptr(a), ptr(b), None, 0)

    def apply(H=8, W=12, h=4, w=6, full=big, o=out):
        return lib.af_guided_apply(0, ptr(full) if full is not None else None, H, W, ptr(f32[0]), ptr(f32[1]), h, w, ptr(o), 0)

    for call, msg in ((lambda: coeffs(i=None), "af_guided_coeffs: null pointer"),
                      (lambda: coeffs(r=0), "af_guided_coeffs: r must be 1..32"),
                      (lambda: coeffs(r=33), "af_guided_coeffs: r must be 1..32"),
                      (lambda: coeffs(eps=0.0), "af_guided_coeffs: eps must be finite and > 0"),
                      (lambda: coeffs(eps=float("nan")), "af_guided_coeffs: eps must be finite and > 0"),
                      (lambda: coeffs(eps=float("inf")), "af_guided_coeffs: eps must be finite and > 0"),
                      (lambda: coeffs(h=0), "af_guided_coeffs: h must be 1..16384"),
                      (lambda: coeffs(w=16385), "af_guided_coeffs: w must be 1..16384"),
                      (lambda: coeffs(b=f32[0]), "af_guided_coeffs: a_out aliases b_out"),
                      (lambda: apply(full=None), "af_guided_apply: null pointer"),
                      (lambda: apply(H=0), "af_guided_apply: H must be 1..16384"),
                      (lambda: apply(W=16385), "af_guided_apply: W must be 1..16384"),
                      (lambda: apply(h=0), "af_guided_apply: h must be 1..16384"),
                      (lambda: apply(H=3), "af_guided_apply: the proxy is larger than the full frame"),
                      (lambda: apply(W=5), "af_guided_apply: the proxy is larger than the full frame"),
                      (lambda: apply(o=big), "af_guided_apply: the output aliases an input")):
        assert call() == -1, msg                                                    # AF_EINVAL
        assert lib.af_last_error(None).decode() == msg


# ---- the pipeline with stub engines ------------------------------------------------------------------------------------------------
class _Engines(TD._StubEngines):
    """The host stubs plus the proxy route's two calls; the stub transfer marks a frame: its full-size ident plus 100 where the three
    inputs belong together."""

    def shrink(self, frame, h, w):
        assert frame.dtype == np.uint8
        self.log.append(("shrink", TD._ident(frame), tuple(frame.shape[:2]), h, w))
        return np.full((h, w, 3), TD._ident(frame), np.uint8)

    def guided_transfer(self, full, proxy_in, proxy_out, radius, eps):
        self.log.append(("transfer", TD._ident(full), tuple(full.shape[:2]), TD._ident(proxy_in), tuple(proxy_in.shape[:2]),
                         TD._ident(proxy_out), tuple(proxy_out.shape[:2]), radius, eps))
        return np.full(full.shape, TD._ident(full) + 100, np.uint8)

    def inputs(self, frames, flows12, flows21, resy, resx):
        self.log.append(("inputs", [tuple(f.shape[:2]) for f in frames], resy, resx))
        return super().inputs(frames, flows12, flows21, resy, resx)

    def warp_error(self, img1, img2, f12, f21, align_corners):
        self.log.append(("warp_error", tuple(img1.shape[:2]), tuple(img2.shape[:2])))
        return 0.5


def test_proxy_route_runs_the_stages_on_the_shrunk_frames():
    import aiod_amd
    E = _Engines()
    d = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, engines=E, proxy_long_edge=20, proxy_radius=5, proxy_eps=9.0)
    sunk = []
    res = d.run(TD._frames(4, 16, 40), keep=("final", "stage1"), sink=lambda name, i, a: sunk.append((name, i, a.shape)), warp_error=True)
    log = E.log
    names = [e[0] for e in log]
    # every frame shrunk once, from the full size, by the rule of max_long_edge (40 / 20: 8 x 20), before anything else
    assert [e for e in log if e[0] == "shrink"] == [("shrink", i, (16, 40), 8, 20) for i in range(4)]
    assert max(i for i, e in enumerate(names) if e == "shrink") < names.index("raft_open")
    # the inner stages see proxy-size frames only
    assert [e for e in log if e[0] == "raft_open"] == [("raft_open", 8, 20)]
    assert [e[1] for e in log if e[0] == "encode"] == list(range(4))
    assert [e for e in log if e[0] == "atlas_open"] == [("atlas_open", 5, 2, 4)]
    assert [e for e in log if e[0] == "inputs"] == [("inputs", [(8, 20)] * 4, 2, 5)]
    assert [e for e in log if e[0] == "filter_open"] == [("filter_open", 8, 20)]
    assert [e[1:] for e in log if e[0] == "filter"] == [(i, i) for i in range(4)]
    # each proxy-size final to its own full-size frame, with the knobs given, after the filter is closed
    assert [e for e in log if e[0] == "transfer"] == [("transfer", i, (16, 40), i, (8, 20), i, (8, 20), 5, 9.0) for i in range(4)]
    assert names.index("filter_close") < names.index("transfer")
    # final is full-size, everything else the proxy's
    assert res["final"].shape == (4, 16, 40, 3) and [int(f[0, 0, 0]) for f in res["final"]] == [100, 101, 102, 103]
    assert res["stage1"].shape == (4, 2, 5, 3)
    assert [s for s in sunk if s[0] == "final"] == [("final", i, (16, 40, 3)) for i in range(4)]
    assert res["proxy"] == {"size": [8, 20], "radius": 5, "eps": 9.0} and res["flow_size"] == [8, 20]
    assert set(res["seconds"]) == {"proxy", "decode + flow", "stage 1", "stage 2", "transfer", "warp error", "total"}
    assert list(res["seconds"])[0] == "proxy" and list(res["seconds"]).index("transfer") == list(res["seconds"]).index("stage 2") + 1
    # E_warp: of the proxy-size input and finals, recorded with its size
    assert [e for e in log if e[0] == "warp_error"] == [("warp_error", (8, 20), (8, 20))] * 6
    assert res["warp_error"]["size"] == [8, 20]


def test_proxy_route_takes_an_iterator_and_the_defaults():
    import aiod_amd
    from aiod_amd import guided as G
    E = _Engines()
    d = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, seed=7, engines=E, proxy_long_edge=20)
    res = d.run(iter(TD._frames(3, 16, 40)))
    assert res["final"].shape == (3, 16, 40, 3) and res["proxy"] == {"size": [8, 20], "radius": G.DEFAULT_RADIUS, "eps": G.DEFAULT_EPS}
    assert set(res["seconds"]) == {"proxy", "decode + flow", "stage 1", "stage 2", "transfer", "total"}
    assert [e[-2:] for e in E.log if e[0] == "transfer"] == [(G.DEFAULT_RADIUS, G.DEFAULT_EPS)] * 3


@pytest.mark.parametrize("as_iterator", [False, True])
@pytest.mark.parametrize("edge", [40, 41, 2000])
def test_a_clip_at_or_below_the_threshold_makes_the_defaults_calls(edge, as_iterator):
    import aiod_amd
    logs, results = [], []
    for kw in ({}, {"proxy_long_edge": edge}):
        E = _Engines()
        frames = TD._frames(4, 16, 40)
        res = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, engines=E, **kw).run(iter(frames) if as_iterator else frames)
        logs.append(E.log)
        results.append(res)
    assert logs[0] == logs[1] and "shrink" not in [e[0] for e in logs[0]] and "transfer" not in [e[0] for e in logs[0]]
    assert set(results[0]) == set(results[1]) and "proxy" not in results[1]
    assert set(results[1]["seconds"]) == {"decode + flow", "stage 1", "stage 2", "total"}
    assert np.array_equal(results[0]["final"], results[1]["final"])


def test_the_unchanged_stub_still_serves_the_default():
    import aiod_amd
    E = TD._StubEngines()                                    # no shrink, no guided_transfer
    res = aiod_amd.Deflicker(None, None, None, config=TD.SMALL, seed=7, engines=E).run(TD._frames(3))
    assert "proxy" not in res and set(res["seconds"]) == {"decode + flow", "stage 1", "stage 2", "total"}
    with pytest.raises(ValueError, match="proxy_long_edge needs an engine with shrink and guided_transfer"):
        aiod_amd.Deflicker(None, None, None, config=TD.SMALL, engines=E, proxy_long_edge=20)


def test_deflicker_argument_refusals():
    import aiod_amd
    E = _Engines()
    mk = lambda **kw: aiod_amd.Deflicker(None, None, None, config=TD.SMALL, engines=E, **kw)      # noqa: E731
    for bad in (0, -5, 1.5, "20", True):
        with pytest.raises(ValueError, match="proxy_long_edge must be None or a positive integer"):
            mk(proxy_long_edge=bad)
    with pytest.raises(ValueError, match="they need proxy_long_edge"):
        mk(proxy_radius=4)
    with pytest.raises(ValueError, match="they need proxy_long_edge"):
        mk(proxy_eps=1.0)
    with pytest.raises(ValueError, match="Deflicker: proxy: radius must be an integer in 1..32"):
        mk(proxy_long_edge=20, proxy_radius=33)
    with pytest.raises(ValueError, match="Deflicker: proxy: eps must be finite and > 0"):
        mk(proxy_long_edge=20, proxy_eps=0.0)
    with pytest.raises(ValueError, match="frame 0 is 4000x1: shrinking it to proxy_long_edge 2000"):
        mk(proxy_long_edge=2000).run([np.zeros((1, 4000, 3), np.uint8)] * 2)
    assert E.log == []


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from aiod_amd import deflicker
    o = deflicker.parse_args(["--frames_dir", "x"])
    assert o.proxy_long_edge is None and o.proxy_radius is None and o.proxy_eps is None
    o = deflicker.parse_args(["--frames_dir", "x", "--proxy_long_edge", "1920", "--proxy_radius", "4", "--proxy_eps", "25"])
    assert o.proxy_long_edge == 1920 and o.proxy_radius == 4 and o.proxy_eps == 25.0
    for argv in (["--proxy_radius", "4"], ["--proxy_eps", "2"], ["--proxy_long_edge", "0"]):
        with pytest.raises(SystemExit):
            deflicker.parse_args(["--frames_dir", "x"] + argv)
    R2 = TD._load("af_run_pipeline_proxy", os.path.join(TD.PKG, "run_pipeline.py"))
    base = ["--video_frame_folder", "data/test/clip"]
    cmds = R2.build_commands(R2.parse_opts(base + ["--in_process", "--proxy_long_edge", "1920", "--proxy_eps", "25.0"]))
    assert cmds[-1][1].endswith(" --proxy_long_edge 1920 --proxy_eps 25.0")
    plain = R2.build_commands(R2.parse_opts(base + ["--in_process"]))
    assert "proxy" not in plain[-1][1] and cmds[-1][1].startswith(plain[-1][1])
    for argv in (["--proxy_long_edge", "1920"], ["--in_process", "--proxy_radius", "4"]):
        with pytest.raises(SystemExit):
            R2.parse_opts(base + argv)


def test_cli_writes_the_proxy_record(tmp_path):
    from PIL import Image
    from aiod_amd import deflicker
    clip = tmp_path / "clip"
    clip.mkdir()
    for i, f in enumerate(TD._frames(3, 16, 40)):
        Image.fromarray(f).save(str(clip / ("%05d.png" % i)))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(TD.SMALL))
    for extra, proxied in ((["--proxy_long_edge", "20", "--proxy_radius", "3"], True), (["--proxy_long_edge", "40"], False), ([], False)):
        out = tmp_path / ("out%d" % len(extra))
        assert deflicker.main(["--frames_dir", str(clip), "--out", str(out), "--config", str(cfg), "--seed", "1"] + extra, engines=_Engines()) == 0
        rec = json.loads((out / "deflicker.json").read_text())
        assert ("proxy" in rec) == proxied
        assert ({"proxy", "transfer"} <= set(rec["seconds"])) == proxied and bool(set(rec["seconds"]) & {"proxy", "transfer"}) == proxied
        if proxied:
            assert rec["proxy"]["size"] == [8, 20] and rec["proxy"]["radius"] == 3 and rec["proxy"]["eps"] == 64.0
        finals = sorted((out / "final" / "output").iterdir())
        assert len(finals) == 3 and np.asarray(Image.open(finals[1])).shape == (16, 40, 3)      # full-size PNGs either way
