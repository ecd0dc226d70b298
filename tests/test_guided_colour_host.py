"""Host-side checks of the guided transfer with a colour guide (no GPU): the numpy restatement the GPU tests hold the
kernels to (tests/guided_colour_ref.py) against its fp64 twin and its identities, the reason for the feature on a cross-channel
correction, the arguments and the CLI flags, and `Deflicker(proxy_guide=...)` with stub engines.

The bound of the restatement against the twin (`_bound`) is derived, not measured.  With u = 2^-24, w1 = 2r + 1, a* and b* the largest
magnitudes of the unsmoothed planes, F = 255:
  - a sampled plane entry carries the rounding of x or b to fp32 (u), the fp32 box mean (w1 - 1 additions along a row, w1 - 1 down the
    rows, one divide: (2 w1 - 1) u) and three fp32 interpolations of three operations each on differences of at most twice the magnitude
    (at most 24 u): (2 w1 + 24) u times a* or b*;
  - the apply multiplies three such entries by f <= F and adds the fourth: (2 w1 + 24) u (3 F a* + b*), then rounds three products
    (u a* F each), three sums (u (3 a* F + b*) each) and f + t (u (F + 3 a* F + b*));
  - the fp64 solve without pivoting and numpy.linalg.solve each err by a few 2^-53 cond in x, cond <= (trace Sigma + 3 e) / e since every
    eigenvalue is at least e; an error dx in x moves A f by 3 F dx and b by 3 F dx: 8 * 2^-53 cond a* 6 F.
The largest difference measured on the cases is 7.85e-5 (the random bytes), where the bound is 4.3e-3; the largest bound is 4.9e-3 (w7)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_transfer_ref as G  # noqa: E402
import guided_colour_ref as R  # noqa: E402
import test_deflicker_host as TD  # noqa: E402      (the stub engines of the one-process pipeline)
import test_deep_video_host as TV  # noqa: E402      (and those of the deep route)

U32 = 2.0 ** -24


def _bound(i, p, r, eps):
    A, b, (d0, d1, d2, e) = R.raw_coeffs(i, p, r, eps, pivots=True)
    a_s, b_s = float(np.abs(A).max()), float(np.abs(b).max())
    w1, F = 2 * r + 1, 255.0
    n, s_c, _, s_cc, _ = R.sums(i, p, r)
    trace = sum((n * s_cc[..., q] - s_c[..., c] ** 2).astype(np.float64) for q, c in ((0, 0), (3, 1), (5, 2)))
    cond = float(((trace + 3 * e) / e).max())
    planes = (2 * w1 + 24) * U32 * (3 * F * a_s + b_s)
    steps = U32 * (3 * a_s * F + 3 * (3 * a_s * F + b_s) + (F + 3 * a_s * F + b_s))
    solve = 8 * 2.0 ** -53 * cond * a_s * 6 * F
    return planes + steps + solve


@pytest.fixture(scope="module")
def cases():
    """name -> (full, proxy_in, proxy_out, r, eps): the shapes of guided_transfer_ref.CASES, the grey guide and the colour matrix."""
    out = {}
    for name in G.CASES:
        out[name] = G.make_case(name) + (G.EPS,)
    grey = R.make_grey()
    for eps, tag in ((64.0, "64"), (R.EPS_FLOOR, "floor")):
        for r in (1, 8, 32):
            out["grey_%s_r%d" % (tag, r)] = grey + (r, eps)
    out["matrix"] = R.make_matrix()[:3] + (8, 64.0)
    return out


ALL = G.CASES + tuple("grey_%s_r%d" % (t, r) for t in ("64", "floor") for r in (1, 8, 32)) + ("matrix",)


# ---- 1. the restatement against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_restatement_against_the_fp64_twin(cases, name):
    full, i, p, r, eps = cases[name]
    A, b = R.coeffs(i, p, r, eps)
    assert A.dtype == np.float32 and A.shape == i.shape[:2] + (9,) and b.shape == i.shape[:2] + (3,)
    u, v = R.unrounded(full, A, b), R.transfer64(full, i, p, r, eps, unrounded=True)
    bound, diff = _bound(i, p, r, eps), float(np.abs(u - v).max())
    print(name, "restatement - twin before rounding: %.3e, bound %.3e" % (diff, bound))
    assert diff <= bound < 0.01
    o, o64 = R.apply(full, A, b), R.transfer64(full, i, p, r, eps)
    differ = o != o64
    assert np.abs(o.astype(np.int64) - o64.astype(np.int64)).max() <= 1
    frac = np.abs(v - np.floor(v) - 0.5)                       # the twin's distance from a half-integer
    assert np.all(frac[differ] <= bound), (name, int(differ.sum()))


# ---- 2. the identities of the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 8, 32])
def test_identity_returns_the_frame(r):
    full, i, _, _ = G.make_case("ratio")
    A, b = R.coeffs(i, i, r, G.EPS)
    assert not A.any() and not b.any()
    assert np.array_equal(R.apply(full, A, b), full)


@pytest.mark.parametrize("c", [-37, 60, (5, -9, 21)])
def test_constant_offset_is_carried_exactly(c):
    rng = np.random.RandomState(3)
    f = rng.randint(70, 186, (75, 106, 3)).astype(np.uint8)
    s = G.area_shrink(f, 37, 53)
    c = np.broadcast_to(np.array(c, np.int64), (3,))
    A, b = R.coeffs(s, (s.astype(np.int64) + c).astype(np.uint8), 8, G.EPS)
    assert not A.any()                                        # kappa is exactly 0 in integers
    assert np.array_equal(b, np.broadcast_to(c.astype(np.float32), b.shape))      # and b exactly c
    assert np.array_equal(R.apply(f, A, b).astype(np.int64), f.astype(np.int64) + c)


def test_diagonal_planes_give_the_per_channel_bytes():
    """A = diag(a): the added terms are exact zeros, so the colour apply is the per-channel apply byte for byte, at 8 and at 16 bits."""
    import depth_transfer_ref as D
    full, i, p, r = G.make_case("ratio")
    a, b = G.coeffs(i, p, r, G.EPS)
    A = np.zeros(a.shape[:2] + (9,), np.float32)
    A[..., 0], A[..., 4], A[..., 8] = a[..., 0], a[..., 1], a[..., 2]
    assert np.array_equal(R.apply(full, A, b), G.apply(full, a, b))
    for bits in (8, 10, 16):
        deep = D.deepen(full, bits, 5)
        assert np.array_equal(R.apply16(deep, bits, A, b), D.apply16(deep, bits, a, b))


# ---- 3. the grey guide -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [64.0, R.EPS_FLOOR])
@pytest.mark.parametrize("r", [1, 8, 32])
def test_grey_guide_is_the_per_channel_filter_at_a_third_of_eps(r, eps):
    """Sigma = s 11^T: (s 11^T + e I)^-1 kappa with kappa = k 1 is k / (3 s + e) 1, so the three equal guide channels share the gain of the
    per-channel filter at eps / 3.  Also: the restatement's solve stays finite with every pivot at least e."""
    full, i, p = R.make_grey()
    assert np.array_equal(i[..., 0], i[..., 1]) and np.array_equal(i[..., 0], i[..., 2])
    colour = R.transfer64(full, i, p, r, eps, unrounded=True)
    # eps / 3 in fp64: the per-channel twin reads eps through fp32, so it is restated here with the exact third
    i64, d64 = i.astype(np.int64), p.astype(np.int64) - i.astype(np.int64)
    n = R.window_n(48, 64, r)[:, :, None].astype(np.float64)
    s_i, s_d, s_ii, s_id = (G._box_int(v, r).astype(np.float64) for v in (i64, d64, i64 * i64, i64 * d64))
    a = (n * s_id - s_i * s_d) / ((n * s_ii - s_i * s_i) + np.float64(np.float32(eps)) / 3.0 * n * n)
    b = (s_d - a * s_i) / n

    def mean(v):
        pad = np.zeros((48 + 2 * r, 64 + 2 * r, 3))
        pad[r:r + 48, r:r + 64] = v
        return sum(pad[r + dy:r + dy + 48, r + dx:r + dx + 64] for dy in range(-r, r + 1) for dx in range(-r, r + 1)) / n
    f = full.astype(np.float64)
    channel = f + (G._bilinear(mean(a), 96, 128, np.float64) * f + G._bilinear(mean(b), 96, 128, np.float64))
    diff = float(np.abs(colour - channel).max())
    print("grey r=%d eps=%g: colour twin - per-channel twin at eps / 3: %.3e" % (r, eps, diff))
    assert diff <= 1e-6
    A, _, (d0, d1, d2, e) = R.raw_coeffs(i, p, r, eps, pivots=True)
    assert np.isfinite(A).all() and (d0 >= e).all() and (d1 >= e).all() and (d2 >= e).all()


# ---- 4. the reason for the feature ---------------------------------------------------------------------------------------------------
def test_a_colour_matrix_is_carried_by_the_colour_guide():
    full, i, p, exact = R.make_matrix()
    assert full.shape == (96, 128, 3) and i.shape == (48, 64, 3)
    assert abs(R.MATRIX - np.eye(3)).max() <= 0.06 and np.abs(R.MATRIX - np.diag(np.diag(R.MATRIX))).max() >= 0.03      # mild, and it mixes
    colour = R.transfer64(full, i, p, 8, 64.0, unrounded=True) - exact
    channel = G.transfer64(full, i, p, 8, 64.0, unrounded=True) - exact
    rms_c, rms_p = float(np.sqrt((colour ** 2).mean())), float(np.sqrt((channel ** 2).mean()))
    print("matrix: colour rms %.3f max %.3f; per-channel rms %.3f max %.3f" % (rms_c, np.abs(colour).max(), rms_p, np.abs(channel).max()))
    assert rms_c <= rms_p / 4
    assert np.abs(colour).max() < 2.0


# ---- 5. arguments ------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    import aiod_amd
    from aiod_amd import guided as Gd
    img = np.zeros((4, 6, 3), np.uint8)
    deep = np.zeros((4, 6, 3), np.uint16)
    for name in ("guided_coeffs_colour", "guided_transfer_colour", "depth_transfer_colour", "guided_apply_colour", "guided_apply_colour16"):
        for name in (name, name + "_device"):
            assert getattr(aiod_amd, name) is getattr(Gd, name) and getattr(Gd, name).__doc__.strip()
    from aiod_amd.deflicker import DeviceEngines
    E = DeviceEngines(None, None, None)      # the engines name the guide: refused before any work, no device touched
    for bad in ("color", "rgb", None, 1, ""):
        for call in (lambda: E.guided_transfer(img, img, img, 8, 64.0, guide=bad), lambda: E.depth_transfer(deep, 10, img, img, 8, 64.0, guide=bad),
                     lambda: Gd.check_guided(8, 64.0, guide=bad)):
            with pytest.raises(ValueError, match="guide must be one of channel, colour"):
                call()
    for bad in (2.0 ** -21, 1e-7, 9e-7):
        for call in (lambda: Gd.guided_transfer_colour(img, img, img, eps=bad), lambda: Gd.guided_coeffs_colour(img, img, eps=bad),
                     lambda: Gd.depth_transfer_colour(deep, 10, img, img, eps=bad), lambda: Gd.guided_transfer_colour_device(img, img, img, eps=bad)):
            with pytest.raises(ValueError, match=r"eps must be at least 2\^-20 with the colour guide"):
                call()
        assert Gd.check_guided(8, bad) == (8, float(np.float32(bad)))      # the per-channel rule is its own: eps > 0
    assert Gd.check_guided(8, 2.0 ** -20, guide="colour") == (8, 2.0 ** -20)
    with pytest.raises(ValueError, match=r"A must be \(h, w, 9\) float32"):
        Gd.guided_apply_colour(img, np.zeros((4, 6, 3), np.float32), np.zeros((4, 6, 3), np.float32))
    with pytest.raises(ValueError, match=r"b must be \(h, w, 3\) float32"):
        Gd.guided_apply_colour16(deep, 10, np.zeros((4, 6, 9), np.float32), np.zeros((4, 6, 9), np.float32))
    with pytest.raises(ValueError, match="must be CUDA tensors"):
        Gd.guided_transfer_colour_device(img, img, img)


def test_abi_refusals_come_before_the_device():
    """The three entries refuse bad arguments by name before any HIP call, so this runs without a GPU; the outputs are untouched."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    import aiod_amd
    lib = aiod_amd.load_library()
    u8 = np.zeros((4, 6, 3), np.uint8)
    A, b = np.full((4, 6, 9), 7, np.float32), np.full((4, 6, 3), 7, np.float32)
    big, out = np.zeros((8, 12, 3), np.uint8), np.full((8, 12, 3), 7, np.uint8)
    big16, out16 = np.zeros((8, 12, 3), np.uint16), np.full((8, 12, 3), 7, np.uint16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def coeffs(h=4, w=6, r=8, eps=64.0, i=u8, bo=b):
        return lib.af_guided_coeffs_colour(0, ptr(i) if i is not None else None, ptr(u8), h, w, r, eps, ptr(A), ptr(bo), None, 0)

    def apply(H=8, W=12, h=4, w=6, full=big, o=out):
        return lib.af_guided_apply_colour(0, ptr(full) if full is not None else None, H, W, ptr(A), ptr(b), h, w, ptr(o), 0)

    def apply16(H=8, W=12, bits=10, full=big16, o=out16):
        return lib.af_guided_apply_colour16(0, ptr(full), H, W, bits, ptr(A), ptr(b), 4, 6, ptr(o), 0)

    for call, msg in ((lambda: coeffs(i=None), "af_guided_coeffs_colour: null pointer"),
                      (lambda: coeffs(r=0), "af_guided_coeffs_colour: r must be 1..32"),
                      (lambda: coeffs(r=33), "af_guided_coeffs_colour: r must be 1..32"),
                      (lambda: coeffs(eps=0.0), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(eps=2.0 ** -21), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(eps=float("nan")), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(eps=float("inf")), "af_guided_coeffs_colour: eps must be finite and >= 2^-20"),
                      (lambda: coeffs(h=0), "af_guided_coeffs_colour: h must be 1..16384"),
                      (lambda: coeffs(w=16385), "af_guided_coeffs_colour: w must be 1..16384"),
                      (lambda: coeffs(bo=A), "af_guided_coeffs_colour: a_out aliases b_out"),
                      (lambda: apply(full=None), "af_guided_apply_colour: null pointer"),
                      (lambda: apply(H=0), "af_guided_apply_colour: H must be 1..16384"),
                      (lambda: apply(W=16385), "af_guided_apply_colour: W must be 1..16384"),
                      (lambda: apply(h=0), "af_guided_apply_colour: h must be 1..16384"),
                      (lambda: apply(H=3), "af_guided_apply_colour: the proxy is larger than the full frame"),
                      (lambda: apply(o=big), "af_guided_apply_colour: the output aliases an input"),
                      (lambda: apply16(bits=7), "af_guided_apply_colour16: bits must be 8..16"),
                      (lambda: apply16(bits=17), "af_guided_apply_colour16: bits must be 8..16"),
                      (lambda: apply16(H=3), "af_guided_apply_colour16: the proxy is larger than the full frame"),
                      (lambda: apply16(o=big16), "af_guided_apply_colour16: the output aliases an input")):
        assert call() == -1, msg                                                    # AF_EINVAL
        assert lib.af_last_error(None).decode() == msg
    assert (A == 7).all() and (b == 7).all() and (out == 7).all() and (out16 == 7).all()


def test_deflicker_argument_refusals():
    import aiod_amd
    E = _Engines()
    mk = lambda **kw: aiod_amd.Deflicker(None, None, None, config=TD.SMALL, engines=E, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="proxy_guide belongs to the proxy route: it needs proxy_long_edge"):
        mk(proxy_guide="colour")
    with pytest.raises(ValueError, match="proxy_guide belongs to the proxy route: it needs proxy_long_edge"):
        mk(proxy_guide="channel")
    for bad in ("color", 3, ""):
        with pytest.raises(ValueError, match="Deflicker: proxy: guide must be one of channel, colour"):
            mk(proxy_long_edge=20, proxy_guide=bad)
    with pytest.raises(ValueError, match=r"Deflicker: proxy: eps must be at least 2\^-20 with the colour guide"):
        mk(proxy_long_edge=20, proxy_eps=1e-7, proxy_guide="colour")
    assert mk(proxy_long_edge=20, proxy_eps=1e-7).proxy_guide == "channel" and mk(proxy_long_edge=20, proxy_guide="colour").proxy_guide == "colour"
    assert E.log == []


def test_cli_flags():
    from aiod_amd import deflicker
    o = deflicker.parse_args(["--frames_dir", "x"])
    assert o.proxy_guide is None
    o = deflicker.parse_args(["--frames_dir", "x", "--proxy_long_edge", "1920", "--proxy_guide", "colour"])
    assert o.proxy_long_edge == 1920 and o.proxy_guide == "colour"
    for argv in (["--proxy_guide", "colour"], ["--proxy_long_edge", "1920", "--proxy_guide", "rgb"]):
        with pytest.raises(SystemExit):
            deflicker.parse_args(["--frames_dir", "x"] + argv)
    R2 = TD._load("af_run_pipeline_guide", os.path.join(TD.PKG, "run_pipeline.py"))
    base = ["--video_frame_folder", "data/test/clip"]
    cmds = R2.build_commands(R2.parse_opts(base + ["--in_process", "--proxy_long_edge", "1920", "--proxy_guide", "colour"]))
    assert cmds[-1][1].endswith(" --proxy_long_edge 1920 --proxy_guide colour")
    plain = R2.build_commands(R2.parse_opts(base + ["--in_process", "--proxy_long_edge", "1920"]))
    assert "proxy_guide" not in plain[-1][1] and cmds[-1][1].startswith(plain[-1][1])
    for argv in (["--proxy_long_edge", "1920", "--proxy_guide", "colour"], ["--in_process", "--proxy_guide", "colour"]):
        with pytest.raises(SystemExit):
            R2.parse_opts(base + argv)
    opts = R2.parse_opts(base + ["--in_process", "--proxy_long_edge", "1920", "--proxy_guide", "colour"])
    opts.in_process = False
    with pytest.raises(ValueError, match="--proxy_guide are options of the one-process pipeline: they need --in_process"):
        R2.build_commands(opts)


# ---- 6. the pipeline with stub engines ---------------------------------------------------------------------------------------------
class _Engines(TD._StubEngines):
    """The host stubs plus the proxy route's calls; both transfers take `guide` and log it."""

    def shrink(self, frame, h, w):
        self.log.append(("shrink", TD._ident(frame), h, w))
        return np.full((h, w, 3), TD._ident(frame), np.uint8)

    def guided_transfer(self, full, proxy_in, proxy_out, radius, eps, guide="absent"):
        self.log.append(("transfer", TD._ident(full), radius, eps, guide))
        return np.full(full.shape, TD._ident(full) + 100, np.uint8)


class _OldEngines(TD._StubEngines):
    """An engine from before the colour guide: five positional arguments, no keyword."""

    def shrink(self, frame, h, w):
        return np.full((h, w, 3), TD._ident(frame), np.uint8)

    def guided_transfer(self, full, proxy_in, proxy_out, radius, eps):
        self.log.append(("transfer", TD._ident(full), radius, eps))
        return np.full(full.shape, TD._ident(full) + 100, np.uint8)


def _run(E, **kw):
    import aiod_amd
    return aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, engines=E, proxy_long_edge=20, **kw).run(TD._frames(3, 16, 40))


def test_default_guide_makes_the_calls_and_records_of_before():
    E, old = _Engines(), _OldEngines()
    res, res_old = _run(E, proxy_radius=5, proxy_eps=9.0), _run(old, proxy_radius=5, proxy_eps=9.0)
    assert [e for e in E.log if e[0] == "transfer"] == [("transfer", i, 5, 9.0, "absent") for i in range(3)]      # no keyword reaches the engine
    assert [e for e in old.log if e[0] == "transfer"] == [("transfer", i, 5, 9.0) for i in range(3)]
    assert res["proxy"] == res_old["proxy"] == {"size": [8, 20], "radius": 5, "eps": 9.0}
    explicit = _run(_Engines(), proxy_radius=5, proxy_eps=9.0, proxy_guide="channel")
    assert explicit["proxy"] == res["proxy"] and np.array_equal(explicit["final"], res["final"])
    assert list(explicit) == list(res)


def test_colour_guide_reaches_the_engine_and_the_record():
    E = _Engines()
    res = _run(E, proxy_radius=5, proxy_eps=9.0, proxy_guide="colour")
    assert [e for e in E.log if e[0] == "transfer"] == [("transfer", i, 5, 9.0, "colour") for i in range(3)]
    assert res["proxy"] == {"size": [8, 20], "radius": 5, "eps": 9.0, "guide": "colour"}
    assert res["final"].shape == (3, 16, 40, 3) and [int(f[0, 0, 0]) for f in res["final"]] == [100, 101, 102]
    with pytest.raises(TypeError):                            # an engine without the keyword cannot serve the colour guide, and says so
        _run(_OldEngines(), proxy_guide="colour")


def test_cli_writes_the_guide_into_the_record(tmp_path):
    from PIL import Image
    from aiod_amd import deflicker
    clip = tmp_path / "clip"
    clip.mkdir()
    for i, f in enumerate(TD._frames(3, 16, 40)):
        Image.fromarray(f).save(str(clip / ("%05d.png" % i)))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(TD.SMALL))
    for extra, want in ((["--proxy_guide", "colour"], {"size": [8, 20], "radius": 8, "eps": 64.0, "guide": "colour"}),
                        ([], {"size": [8, 20], "radius": 8, "eps": 64.0})):
        out = tmp_path / ("out%d" % len(extra))
        E = _Engines()
        assert deflicker.main(["--frames_dir", str(clip), "--out", str(out), "--config", str(cfg), "--seed", "1", "--proxy_long_edge", "20"] + extra, engines=E) == 0
        assert json.loads((out / "deflicker.json").read_text())["proxy"] == want
        assert {e[-1] for e in E.log if e[0] == "transfer"} == {"colour" if extra else "absent"}


def test_deep_route_passes_the_guide_to_depth_transfer():
    """The deep route (bits=...) on the stubs of tests/test_deep_video_host.py, whose depth_transfer takes the six positional arguments of
    before: the default guide still reaches it, guide="colour" goes through the keyword, and the `depth` record carries it."""
    import aiod_amd

    class Deep(TV._DeepEngines):
        shrink, guided_transfer = _Engines.shrink, _Engines.guided_transfer      # proxy_long_edge asks for them; nothing here is shrunk

    class DeepColour(Deep):
        def depth_transfer(self, full16, bits, proxy_in, proxy_out, radius, eps, guide="absent"):
            self.log.append(("guide", guide))
            return super().depth_transfer(full16, bits, proxy_in, proxy_out, radius, eps)

    frames = TV._deep_grey_clip()[:3]
    mk = lambda E, **kw: aiod_amd.Deflicker(None, None, None, config=TD.SMALL, seed=1, engines=E, proxy_long_edge=2000, **kw).run(frames, bits=10)      # noqa: E731
    plain, same = mk(Deep()), mk(DeepColour())
    assert plain["depth"] == same["depth"] == {"bits": 10, "radius": aiod_amd.DEFAULT_RADIUS, "eps": aiod_amd.DEFAULT_EPS} and "proxy" not in plain
    E = DeepColour()
    res = mk(E, proxy_guide="colour")
    assert [e for e in E.log if e[0] == "guide"] == [("guide", "colour")] * 3
    assert res["depth"] == {"bits": 10, "radius": aiod_amd.DEFAULT_RADIUS, "eps": aiod_amd.DEFAULT_EPS, "guide": "colour"} and "proxy" not in res
    assert np.array_equal(res["final"], plain["final"])
