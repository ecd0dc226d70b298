"""Host-side checks of the deep-video route (no GPU): the numpy restatements the GPU tests hold the kernels to
(tests/y4m16_ref.py, tests/depth_transfer_ref.py) against what exists (tests/y4m_ref.py, tests/guided_transfer_ref.py at 8 bits), against
their fp64 twins within derived bounds and against their definitions; the container above 8 bits per sample; and deflicker.py
--video_depth keep / Deflicker.run(bits=...) with the stub engines of tests/test_y4m_host.py (imported, not edited).

The bound against the fp64 transfer twin.  The restatement and the twin round real values v32 and v64; they differ by at most one level,
and only where v64 lies within delta = |v32 - v64| of a rounding boundary (a "near-tie").  delta(D) is derived, not measured:
  planes      |abar - abar64| <= BOUND_A, |bbar - bbar64| <= BOUND_B: the asserted bounds of tests/test_guided_transfer_host.py (asserted on
              this file's inputs too), times the operands: BOUND_A * M + BOUND_B * (M / 255);
  sampling    the bilinear taps in fp32: three operations each on a plane value, relative 2^-24 each: 3 * 2^-24 * (A * M + B * M / 255)
              with A = 2, B = 256 bounding |abar| and |bbar| (asserted);
  last step   s = (float)(M / 255) (relative 2^-24, times B * M / 255) and the four operations p, q, t, f + t, each half an ulp of a
              value below 4 M: 4 * 2^-24 * 4 M.
At D = 10 that is 0.0024 of a level: a sample is a near-tie with probability 2 delta, so the twin's own near-ties are below 1 % of the
samples (asserted: the condition of the cap), and the samples that differ are among them (asserted: the cap).  At D = 12 and 16 delta is
0.0096 and 0.1529 of a level: the subset property is asserted and the shares are printed, no 1 % is claimed."""
import io
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")
sys.path.insert(0, HERE)
import y4m_ref as R8  # noqa: E402
import y4m16_ref as R  # noqa: E402
import guided_transfer_ref as G  # noqa: E402
import depth_transfer_ref as DT  # noqa: E402
import test_deflicker_host as TH  # noqa: E402
import test_y4m_host as TY  # noqa: E402      (the stub engines of the video route)

CASES = [(layout, matrix, full) for layout in R.LAYOUTS for matrix in R.MATRICES for full in (False, True)]
SIZES = ((1, 1), (2, 2), (5, 3), (33, 18))      # (w, h)
BOUND_A, BOUND_B = 2 * 2.4985526603238384e-07, 2 * 3.599137346554926e-05      # tests/test_guided_transfer_host.py


# ---- the restatement at 8 bits is the existing one -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,matrix,full", CASES)
def test_restatement_at_8_bits_is_y4m_ref(layout, matrix, full):
    assert R.int_matrices(matrix, full, 8) == R8.int_matrices(matrix, full) and R.qbits(8) == R8.BITS
    for w, h in SIZES:
        for name, payload in R8.inputs(h, w, layout):
            got = R.yuv_to_rgb(payload.astype(np.uint16), h, w, layout, matrix, full, 8)
            assert got.dtype == np.uint16 and np.array_equal(got, R8.yuv_to_rgb(payload, h, w, layout, matrix, full)), ("read", w, h, name)
        for name, img in R8.rgb_inputs(h, w):
            got = R.rgb_to_yuv(img.astype(np.uint16), layout, matrix, full, 8)
            assert got.dtype == np.uint16 and np.array_equal(got, R8.rgb_to_yuv(img, layout, matrix, full)), ("write", w, h, name)


def test_constants_per_depth():
    for bits in R.DEPTHS:
        y0, sy, sc, c = R.scales(False, bits)
        assert (y0, c) == (16 << (bits - 8), 1 << (bits - 1)) and sy == Fraction(219 << (bits - 8), (1 << bits) - 1) and sc == Fraction(224 << (bits - 8), (1 << bits) - 1)
        assert R.scales(True, bits) == (0, 1, 1, 1 << (bits - 1)) and R.qbits(bits) == bits + 6
        for matrix in R.MATRICES:
            for full in (False, True):
                (ky, ku, kv), inv = R.int_matrices(matrix, full, bits)
                assert sum(ky) == round(R.scales(full, bits)[1] * (1 << (bits + 6))) and sum(ku) == 0 and sum(kv) == 0
                assert max(abs(v) for v in ky + ku + kv + list(inv)) < 2 ** 31      # the kernel holds them in ints
                # the host builds them in fp64 by the same expressions, rounded with nearbyint: no entry sits near enough to a tie to differ
                fwd, rinv = R.real_matrices(matrix, full, bits)
                for v in [x for row in fwd for x in row] + list(rinv):
                    frac = (v * (1 << (bits + 6))) % 1
                    assert abs(frac - Fraction(1, 2)) > Fraction(1, 10 ** 6), (bits, matrix, full, float(v))


def test_grey_is_carried_exactly_in_full_range():
    for bits in (9, 10, 12, 14, 16):
        m = R.maxv(bits)
        for v in (0, 1, m // 2, m - 1, m):
            img = np.full((4, 6, 3), v, np.uint16)
            for layout in R.LAYOUTS:
                p = R.rgb_to_yuv(img, layout, "bt709", True, bits)
                assert (p[:24] == v).all() and (p[24:] == 1 << (bits - 1)).all()
                assert np.array_equal(R.yuv_to_rgb(p, 4, 6, layout, "bt709", True, bits), img)


def test_a_sample_above_the_maximum_reads_as_the_maximum():
    for layout in ("444", "420jpeg"):
        (_, above), = [x for x in R.inputs(5, 7, layout, 10, above=True) if x[0] == "above"]
        assert above.max() > 1023
        assert np.array_equal(R.yuv_to_rgb(above, 5, 7, layout, "bt601", False, 10), R.yuv_to_rgb(np.minimum(above, 1023), 5, 7, layout, "bt601", False, 10))
        (_, img), = [x for x in R.rgb_inputs(5, 7, 10, above=True) if x[0] == "above"]
        assert np.array_equal(R.rgb_to_yuv(img, layout, "bt601", False, 10), R.rgb_to_yuv(np.minimum(img, 1023), layout, "bt601", False, 10))


# ---- distance from the exact fp64 formula ----------------------------------------------------------------------------------------
def test_bounds_at_8_bits_are_the_documented_ones():
    """The derivation from the tables is tighter than y4m_ref's closed form (which takes 2^-(BITS + 1) for every coefficient)."""
    for matrix in R.MATRICES:
        for full in (False, True):
            assert 0.5 < R.read_bound(matrix, full, 8) <= R8.READ_BOUND and 0.5 < R.write_bound(matrix, full, 8) <= 0.5 + 3 * 255 * 1.05 * 2.0 ** -14


@pytest.mark.parametrize("bits", R.DEPTHS)
def test_restatement_within_the_derived_bound_of_exact(bits):
    worst_r = worst_w = 0.0
    slack = 64 * R.maxv(bits) * 2.0 ** -52                   # the twin's own fp64 roundoff: a few dozen operations on values up to M
    for layout, matrix, full in CASES:
        rb, wb = R.read_bound(matrix, full, bits), R.write_bound(matrix, full, bits)
        assert 0.5 < rb < 0.54 and 0.5 < wb < 0.54          # Q grows with the depth: the coefficient term stays a few hundredths of a level
        for w, h in ((5, 3), (33, 18)):
            for name, payload in R.inputs(h, w, layout, bits, above=True):
                got = R.yuv_to_rgb(payload, h, w, layout, matrix, full, bits).astype(np.float64)
                err = np.abs(got - R.yuv_to_rgb_exact(payload, h, w, layout, matrix, full, bits)).max()
                worst_r = max(worst_r, err)
                assert err <= rb + slack, ("read", bits, layout, matrix, full, w, h, name, err, rb)
            for name, img in R.rgb_inputs(h, w, bits, above=True):
                got = R.rgb_to_yuv(img, layout, matrix, full, bits).astype(np.float64)
                err = np.abs(got - R.rgb_to_yuv_exact(img, layout, matrix, full, bits)).max()
                worst_w = max(worst_w, err)
                assert err <= wb + slack, ("write", bits, layout, matrix, full, w, h, name, err, wb)
    print("bits %d: max |restatement - exact| reading %.4f, writing %.4f" % (bits, worst_r, worst_w))


# ---- depth reduce ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [9, 10, 12, 14, 16])
def test_reduce_depth_is_round_255_v_over_m(bits):
    m = R.maxv(bits)
    v = np.arange(m + 1, dtype=np.uint16)
    got = R.reduce_depth(v, bits)
    want = np.array([round(Fraction(255 * int(x), m)) for x in v], np.uint8)      # Fraction rounds half to even; no half occurs (asserted)
    assert all((2 * 255 * int(x)) % m != 0 or (2 * 255 * int(x) // m) % 2 == 0 for x in v[::max(1, m // 4096)])
    assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(DT.reduce_depth(v, bits), want)
    assert got[0] == 0 and got[-1] == 255
    if bits < 16:
        assert (R.reduce_depth(np.arange(m + 1, 65536, dtype=np.uint16), bits) == 255).all()      # above M reads as M


def test_reduce_depth_is_the_identity_at_8_bits():
    assert np.array_equal(R.reduce_depth(np.arange(256, dtype=np.uint16), 8), np.arange(256, dtype=np.uint8))


# ---- depth transfer --------------------------------------------------------------------------------------------------------------
def test_apply16_at_8_bits_is_the_existing_apply():
    assert DT.scale(8) == np.float32(1) and DT.scale(16) == np.float32(257)
    for name in ("ratio", "same", "one", "random", "wide"):
        full, i, p, r = G.make_case(name)
        a, b = G.coeffs(i, p, r, G.EPS)
        assert np.array_equal(DT.apply16(full.astype(np.uint16), 8, a, b), G.apply(full, a, b)), name


def _deep_case(shape_full, shape_proxy, bits, seed):
    rng = np.random.default_rng(seed)
    full = rng.integers(0, DT.maxv(bits) + 1, shape_full + (3,)).astype(np.uint16)
    i = rng.integers(0, 256, shape_proxy + (3,), dtype=np.uint8)
    p = rng.integers(0, 256, shape_proxy + (3,), dtype=np.uint8)
    return full, i, p


@pytest.mark.parametrize("bits", [9, 10, 12, 14, 16])
def test_identity_returns_the_deep_frame(bits):
    for sf, sp in (((24, 20), (24, 20)), ((20, 15), (9, 7))):
        full, i, _ = _deep_case(sf, sp, bits, 3)
        assert np.array_equal(DT.transfer16(full, bits, i, i, 2, G.EPS), full)
        assert np.array_equal(DT.transfer16(full, bits, i, i, 8, G.EPS), full)


@pytest.mark.parametrize("c", [-37, 1, 60])
def test_constant_offset_becomes_257_c_at_16_bits(c):
    rng = np.random.default_rng(40 + c)
    full = rng.integers(37 * 257, 65536 - 60 * 257, (20, 15, 3)).astype(np.uint16)      # nothing clips
    for shape in ((20, 15), (9, 7)):
        i = rng.integers(70, 186, shape + (3,)).astype(np.uint8)
        p = (i.astype(np.int64) + c).astype(np.uint8)
        a, b = G.coeffs(i, p, 2, G.EPS)
        assert not a.any() and np.array_equal(b, np.full(b.shape, c, np.float32))
        assert np.array_equal(DT.apply16(full, 16, a, b).astype(np.int64), full.astype(np.int64) + 257 * c)


def _delta(bits):
    m = float(DT.maxv(bits))
    a_max, b_max = 2.0, 256.0
    return BOUND_A * m + BOUND_B * m / 255 + 3 * 2.0 ** -24 * (a_max * m + b_max * m / 255) + 2.0 ** -24 * b_max * m / 255 + 4 * 2.0 ** -24 * 4 * m


@pytest.mark.parametrize("bits", [10, 12, 16])
def test_restatement_is_within_one_level_of_the_fp64_twin(bits):
    delta = _delta(bits)
    assert (bits, round(delta, 4)) in ((10, 0.0024), (12, 0.0096), (16, 0.1529))
    for sf, sp in (((24, 20), (24, 20)), ((20, 15), (9, 7))):
        full, i, p = _deep_case(sf, sp, bits, 11)
        a, b = G.coeffs(i, p, 2, G.EPS)
        a64, b64 = G.coeffs64(i, p, 2, G.EPS)
        assert np.abs(a - a64).max() <= BOUND_A and np.abs(b - b64).max() <= BOUND_B and np.abs(a).max() <= 2 and np.abs(b).max() <= 256
        out = DT.apply16(full, bits, a, b).astype(np.int64)
        twin = DT.transfer16_64(full, bits, i, p, 2, G.EPS).astype(np.int64)
        real = DT.transfer16_64(full, bits, i, p, 2, G.EPS, unrounded=True)
        near = np.abs(np.abs(real - np.floor(real)) - 0.5) <= delta                      # the twin's own near-ties
        clip = (real <= delta) | (real >= DT.maxv(bits) - delta)                        # and the two clamp boundaries
        differ = out != twin
        print("bits %d, %dx%d over %dx%d: %.3f %% of the samples differ from the twin, %.3f %% of the twin's are near-ties (delta %.4f)"
              % (bits, sp[1], sp[0], sf[1], sf[0], 100 * differ.mean(), 100 * near.mean(), delta))
        assert np.abs(out - twin).max() <= 1
        assert not (differ & ~(near | clip)).any()                                       # the cap: only near-ties may differ
        if bits == 10:
            assert near.mean() < 0.01                                                    # the condition: these inputs have few of them


# ---- the container ---------------------------------------------------------------------------------------------------------------
def _stream(head, payloads):
    return head.encode() + b"\n" + b"".join(b"FRAME\n" + bytes(p) for p in payloads)


def test_deep_tags_parse_only_when_asked():
    from aiod_amd import Y4MError, Y4MReader
    from aiod_amd.y4m import frame_bytes
    head = "YUV4MPEG2 W5 H3 F25:1 Ip A1:1 "
    for tag, layout in (("420p", "420jpeg"), ("422p", "422"), ("444p", "444")):
        for n in (9, 10, 12, 14, 16):
            r = Y4MReader(io.BytesIO(_stream(head + "C%s%d XYSCSS=%s%d" % (tag, n, tag.upper(), n), [])), deep=True)
            assert (r.layout, r.bits, r.frame_bytes) == (layout, n, 2 * R8.frame_bytes(3, 5, layout)) and r.info()["bits"] == n
    for n in (9, 10, 12, 16):
        r = Y4MReader(io.BytesIO(_stream(head + "Cmono%d" % n, [])), deep=True)
        assert (r.layout, r.bits, r.frame_bytes) == ("mono", n, 30)
    for tag in ("Cmono14", ):
        with pytest.raises(Y4MError, match="header tag '%s': deep layout not handled" % tag):
            Y4MReader(io.BytesIO(_stream(head + tag, [])), deep=True)
    with pytest.raises(Y4MError, match="header tag 'C420p11': chroma layout not handled"):
        Y4MReader(io.BytesIO(_stream(head + "C420p11", [])), deep=True)
    # without the argument: refused as before, the old sentence first, the new flag named after it
    with pytest.raises(Y4MError, match="header tag 'C420p10': only 8 bits per sample are handled; add `-pix_fmt yuv420p` to the ffmpeg command, or .*--video_depth keep"):
        Y4MReader(io.BytesIO(_stream(head + "C420p10", [])))
    r = Y4MReader(io.BytesIO(_stream(head + "C420jpeg", [bytes(27)])), deep=True)      # an 8-bit stream: what it always was
    assert r.bits == 8 and next(r).dtype == np.uint8
    r8 = Y4MReader(io.BytesIO(_stream(head + "C420jpeg", [])))
    assert r8.bits == 8 and "bits" not in r8.info()
    for layout in R.LAYOUTS:
        for w, h in ((1, 1), (5, 3), (197, 130)):
            assert frame_bytes(h, w, layout, 8) == frame_bytes(h, w, layout) == R8.frame_bytes(h, w, layout)
            for bits in (9, 10, 16):
                assert frame_bytes(h, w, layout, bits) == 2 * R8.frame_bytes(h, w, layout)
    with pytest.raises(ValueError, match="bits must be an integer in 8..16"):
        frame_bytes(3, 5, "444", 17)


def test_deep_round_trip_and_the_header_ffmpeg_writes():
    from aiod_amd import Y4MError, Y4MReader, Y4MWriter
    rng = np.random.default_rng(5)
    n = R8.frame_bytes(3, 5, "420jpeg")
    payloads = [rng.integers(0, 1024, n).astype(np.uint16) for _ in range(3)]
    buf = io.BytesIO()
    wr = Y4MWriter(buf, 5, 3, Fraction(25), "420jpeg", False, aspect=Fraction(1), bits=10)
    for p in payloads:
        wr.write(p)
    with pytest.raises(ValueError, match="frame 3 is 27 uint8 samples"):
        wr.write(np.zeros(n, np.uint8))
    with pytest.raises(ValueError, match="frame 3 is 26 uint16 samples"):
        wr.write(np.zeros(n - 1, np.uint16))
    raw = buf.getvalue()
    head = b"YUV4MPEG2 W5 H3 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\n"      # ffmpeg -pix_fmt yuv420p10le -f yuv4mpegpipe
    assert raw.startswith(head + b"FRAME\n") and len(raw) == len(head) + 3 * (6 + 2 * n)
    assert raw[len(head) + 6:len(head) + 6 + 2 * n] == payloads[0].astype("<u2").tobytes()      # little-endian samples
    r = Y4MReader(io.BytesIO(raw), deep=True)
    got = list(r)
    assert (r.bits, r.layout, r.full_range, r.frames_read) == (10, "420jpeg", False, 3)
    assert all(g.dtype == np.uint16 and np.array_equal(g, p) for g, p in zip(got, payloads))
    r = Y4MReader(io.BytesIO(raw[:-5]), deep=True)
    next(r), next(r)
    with pytest.raises(Y4MError, match="truncated frame 2: 49 of 54 bytes"):
        next(r)
    buf = io.BytesIO()
    Y4MWriter(buf, 4, 2, "25", "mono", True, bits=12).close()
    assert buf.getvalue() == b"YUV4MPEG2 W4 H2 F25:1 Ip A0:0 Cmono12 XCOLORRANGE=FULL\n"
    buf = io.BytesIO()
    Y4MWriter(buf, 4, 2, "25", "444", True, bits=16).close()
    assert buf.getvalue() == b"YUV4MPEG2 W4 H2 F25:1 Ip A0:0 C444p16 XYSCSS=444P16 XCOLORRANGE=FULL\n"
    with pytest.raises(ValueError, match="420mpeg2 has no tag above 8 bits"):
        Y4MWriter(io.BytesIO(), 4, 2, "25", "420mpeg2", False, bits=10)
    with pytest.raises(ValueError, match="no mono tag at 14 bits"):
        Y4MWriter(io.BytesIO(), 4, 2, "25", "mono", False, bits=14)
    with pytest.raises(ValueError, match="bits must be an integer in 8..16"):
        Y4MWriter(io.BytesIO(), 4, 2, "25", "444", False, bits=7)
    buf = io.BytesIO()
    Y4MWriter(buf, 4, 2, "25", "mono", False, bits=8).close()                               # bits = 8: today's header
    assert buf.getvalue() == b"YUV4MPEG2 W4 H2 F25:1 Ip A0:0 Cmono XCOLORRANGE=LIMITED\n"


def test_abi_declares_the_deep_symbols():
    import re
    import aiod_amd
    hdr = open(os.path.join(ROOT, "include", "atlasfit.h")).read()
    declared = set(re.findall(r"\b(af_[a-z_0-9]+)\s*\(", hdr))
    for name in ("af_yuv_to_rgb16", "af_rgb_to_yuv16", "af_depth_reduce", "af_guided_apply16"):
        assert name in declared and name in aiod_amd.atlasfit.ABI_SYMBOLS and hasattr(aiod_amd.load_library(), name)
    for name in ("yuv_to_rgb16", "rgb16_to_yuv", "yuv_to_rgb16_device", "rgb16_to_yuv_device", "reduce_depth", "reduce_depth_device", "guided_apply16",
                 "guided_apply16_device", "depth_transfer", "depth_transfer_device"):
        assert callable(getattr(aiod_amd, name)), name
    for name in ("frame16", "reduce_depth", "depth_transfer", "yuv_to_rgb16", "rgb16_to_yuv"):
        assert hasattr(aiod_amd.deflicker.DeviceEngines, name), name
    src = open(os.path.join(PKG, "build.py")).read()
    assert '"yuv16.hip"' in src


def test_refusals_before_the_device_is_touched():
    """AF_EINVAL by name from a process without a GPU: nothing reached the device."""
    import ctypes as C
    import aiod_amd
    lib = aiod_amd.load_library()
    u16, u8, f32 = np.zeros(4096, np.uint16), np.zeros(4096, np.uint8), np.zeros(4096, np.float32)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)      # noqa: E731
    conv = lambda fn, **k: getattr(lib, fn)(0, k.get("src", p(u16)), k.get("h", 4), k.get("w", 4), k.get("layout", 2), k.get("matrix", 0), 0,      # noqa: E731
                                           k.get("bits", 10), k.get("dst", p(u16, 2048)), 0)
    for fn in ("af_yuv_to_rgb16", "af_rgb_to_yuv16"):
        for kw, msg in ((dict(src=None), "null pointer"), (dict(h=0), "h must be 1..16384"), (dict(w=16385), "w must be 1..16384"), (dict(layout=5), "unknown layout"),
                        (dict(matrix=2), "unknown matrix"), (dict(bits=7), "bits must be 8..16"), (dict(bits=17), "bits must be 8..16"),
                        (dict(src=p(u16, 1)), "uint16 pointers must be 2-byte aligned"), (dict(dst=p(u16, 2049)), "uint16 pointers must be 2-byte aligned")):
            assert conv(fn, **kw) == -1 and lib.af_last_error(None).decode() == "%s: %s" % (fn, msg), (fn, kw)
    red = lambda **k: lib.af_depth_reduce(0, k.get("src", p(u16)), k.get("count", 16), k.get("bits", 10), k.get("dst", p(u8)), 0)      # noqa: E731
    for kw, msg in ((dict(dst=None), "null pointer"), (dict(count=0), "count must be 1..2^32"), (dict(count=2 ** 32 + 1), "count must be 1..2^32"),
                    (dict(bits=17), "bits must be 8..16"), (dict(src=p(u16, 1)), "uint16 pointers must be 2-byte aligned"), (dict(dst=p(u16, 4)), "the output aliases the input")):
        assert red(**kw) == -1 and lib.af_last_error(None).decode() == "af_depth_reduce: " + msg, kw
    app = lambda **k: lib.af_guided_apply16(0, k.get("full", p(u16)), k.get("H", 4), k.get("W", 6), k.get("bits", 10), p(f32), p(f32, 2048), k.get("h", 2), 3,      # noqa: E731
                                            k.get("out", p(u16, 2048)), 0)
    for kw, msg in ((dict(full=None), "null pointer"), (dict(H=0), "H must be 1..16384"), (dict(W=16385), "W must be 1..16384"), (dict(h=0), "h must be 1..16384"),
                    (dict(H=1), "the proxy is larger than the full frame"), (dict(bits=7), "bits must be 8..16"),
                    (dict(out=p(u16, 2049)), "uint16 pointers must be 2-byte aligned"), (dict(out=p(u16, 8)), "the output aliases an input")):
        assert app(**kw) == -1 and lib.af_last_error(None).decode() == "af_guided_apply16: " + msg, kw
    assert not u16.any() and not u8.any()
    from aiod_amd import guided as Gd
    with pytest.raises(ValueError, match="reduce_depth: bits must be an integer in 8..16"):
        Gd.reduce_depth(u16, 17)
    with pytest.raises(ValueError, match="reduce_depth: expected a non-empty uint16 array"):
        Gd.reduce_depth(u8, 10)
    with pytest.raises(ValueError, match="depth_transfer: full must be \\(H, W, 3\\) uint16"):
        Gd.depth_transfer(np.zeros((4, 6, 3), np.uint8), 10, np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6, 3), np.uint8))
    with pytest.raises(ValueError, match="yuv_to_rgb16: expected 24 uint16 samples for a 4x4 420jpeg frame, got 24 uint8"):
        aiod_amd.yuv_to_rgb16(np.zeros(24, np.uint8), 4, 4, "420jpeg", "bt601", False, 10)


# ---- flags and orchestration with stub engines -----------------------------------------------------------------------------------
H, W, N, BITS = TY.H, TY.W, TY.N, 10


class _DeepEngines(TY._VideoEngines):
    """The video route's stub engines plus the deep route's hand-offs, computed by the restatements on the host."""

    def frame16(self, x):
        x = np.asarray(x)
        assert x.dtype == np.uint16
        self.log.append(("frame16", int(x[0, 0, 0])))
        return x

    def reduce_depth(self, t, bits):
        self.log.append(("reduce_depth", int(t[0, 0, 0]), bits))
        return R.reduce_depth(t, bits)

    def depth_transfer(self, full16, bits, proxy_in, proxy_out, radius, eps):
        self.log.append(("depth_transfer", int(full16[0, 0, 0]), bits, TH._ident(proxy_in), TH._ident(proxy_out), radius, eps))
        return (full16.astype(np.int64) + 4 * (proxy_out.astype(np.int64) - proxy_in)).astype(np.uint16)

    def yuv_to_rgb16(self, payload, h, w, layout, matrix, full_range, bits):
        self.log.append(("yuv_to_rgb16", h, w, layout, matrix, bool(full_range), bits))
        return R.yuv_to_rgb(payload, h, w, layout, matrix, full_range, bits)

    def rgb16_to_yuv(self, img, layout, matrix, full_range, bits):
        self.log.append(("rgb16_to_yuv", int(np.asarray(img)[0, 0, 0]), layout, matrix, bool(full_range), bits))
        return R.rgb_to_yuv(np.asarray(img), layout, matrix, full_range, bits)


def _deep_grey_clip():
    return [np.full((H, W, 3), 4 * (10 + i) + 1, np.uint16) for i in range(N)]      # grey, full range: the conversions are the identity; reduces to 10 + i


@pytest.fixture()
def deep_clip(tmp_path):
    path = tmp_path / "deep.y4m"
    path.write_bytes(R.y4m_bytes(_deep_grey_clip(), (25, 1), "420jpeg", "bt601", True, BITS))
    cfg = tmp_path / "small.json"
    cfg.write_text(json.dumps(TH.SMALL))
    plain = tmp_path / "clip.y4m"
    plain.write_bytes(R8.y4m_bytes(TY._grey_clip(), (25, 1), "420jpeg", "bt601", True))
    return {"path": str(path), "plain": str(plain), "cfg": str(cfg), "dir": tmp_path}


def test_reduction_of_the_stub_clip():
    assert [int(R.reduce_depth(f, BITS)[0, 0, 0]) for f in _deep_grey_clip()] == [10 + i for i in range(N)]


def test_deep_video_run_call_list_header_and_record(deep_clip):
    from aiod_amd import deflicker
    E = _DeepEngines()
    out = deep_clip["dir"] / "res"
    target = deep_clip["dir"] / "o.y4m"
    assert deflicker.main(["--video", deep_clip["path"], "--video_depth", "keep", "--video_out", str(target), "--out", str(out), "--config", deep_clip["cfg"],
                           "--seed", "3"], engines=E) == 0
    names = [e[0] for e in E.log]
    nsamples = R8.frame_bytes(H, W, "420jpeg")
    deep_vals = [4 * (10 + i) + 1 for i in range(N)]
    # in: every payload uploaded as uint16 samples, converted at 10 bits, kept, reduced; all of that before RAFT opens
    assert [e for e in E.log if e[0] == "payload"] == [("payload", nsamples)] * N
    assert [e for e in E.log if e[0] == "yuv_to_rgb16"] == [("yuv_to_rgb16", H, W, "420jpeg", "bt601", True, BITS)] * N
    assert "yuv_to_rgb" not in names and "rgb_to_yuv" not in names
    assert [e for e in E.log if e[0] == "frame16"] == [("frame16", v) for v in deep_vals]
    assert [e for e in E.log if e[0] == "reduce_depth"] == [("reduce_depth", v, BITS) for v in deep_vals]
    assert names.index("raft_open") > max(i for i, n in enumerate(names) if n in ("payload", "yuv_to_rgb16", "frame16", "reduce_depth"))
    assert names[:3] == ["payload", "yuv_to_rgb16", "frame16"] and names[names.index("raft_open") - 1] == "reduce_depth"
    # what the stages see is the 8-bit reduction
    assert [e[1] for e in E.log if e[0] == "encode"] == [10 + i for i in range(N)]
    # out: after the filter is closed, every final carried to its deep frame from the 8-bit pair the run holds, then converted, in order
    from aiod_amd import DEFAULT_EPS, DEFAULT_RADIUS
    assert [e for e in E.log if e[0] == "depth_transfer"] == [("depth_transfer", v, BITS, 10 + i, 10 + i, DEFAULT_RADIUS, DEFAULT_EPS) for i, v in enumerate(deep_vals)]
    tail = [n for n in names if n in ("filter", "filter_close", "depth_transfer", "rgb16_to_yuv")]
    assert tail == ["filter"] * N + ["filter_close"] + ["depth_transfer", "rgb16_to_yuv"] * N
    assert [e for e in E.log if e[0] == "rgb16_to_yuv"] == [("rgb16_to_yuv", v, "420jpeg", "bt601", True, BITS) for v in deep_vals]
    raw = target.read_bytes()
    head = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + N * (6 + 2 * nsamples)
    assert raw == R.y4m_bytes(_deep_grey_clip(), (25, 1), "420jpeg", "bt601", True, BITS)      # the stub transfer of an unchanged pair: the input
    assert not (out / "final").exists()
    rec = json.loads((out / "deflicker.json").read_text())
    assert rec["depth"] == {"bits": BITS, "radius": DEFAULT_RADIUS, "eps": DEFAULT_EPS} and "proxy" not in rec
    assert "depth" in rec["seconds"] and "transfer" in rec["seconds"] and rec["frames"] == N and rec["yuv_layout"] == "420jpeg"


def test_keep_on_an_8_bit_stream_makes_the_calls_of_before(deep_clip):
    from aiod_amd import deflicker
    logs, outs = [], []
    for k, extra in enumerate(([], ["--video_depth", "keep"], ["--video_depth", "8"])):
        E = TY._VideoEngines()                                # the stubs as they were: no deep method exists on them
        assert not hasattr(E, "frame16")
        target = deep_clip["dir"] / ("o%d.y4m" % k)
        assert deflicker.main(["--video", deep_clip["plain"], "--video_out", str(target), "--out", str(deep_clip["dir"] / ("r%d" % k)), "--config", deep_clip["cfg"],
                               "--seed", "3"] + extra, engines=E) == 0
        logs.append(E.log)
        outs.append(target.read_bytes())
        assert "depth" not in json.loads((deep_clip["dir"] / ("r%d" % k) / "deflicker.json").read_text())
    assert logs[0] == logs[1] == logs[2] and outs[0] == outs[1] == outs[2] == TY._expected_out()


def test_keep_on_a_deep_stream_needs_video_out(deep_clip):
    from aiod_amd import deflicker
    E = _DeepEngines()
    with pytest.raises(SystemExit, match="deep.y4m: --video_depth keep on a stream of 10 bits per sample needs --video_out.*no deep PNG route"):
        deflicker.main(["--video", deep_clip["path"], "--video_depth", "keep", "--out", str(deep_clip["dir"] / "r"), "--config", deep_clip["cfg"]], engines=E)
    assert E.log == [] and not (deep_clip["dir"] / "r").exists()
    with pytest.raises(SystemExit, match="C420p10.*-pix_fmt yuv420p.*--video_depth keep"):      # and without the flag: the refusal of before, the flag named after it
        deflicker.main(["--video", deep_clip["path"], "--video_out", str(deep_clip["dir"] / "o.y4m"), "--out", str(deep_clip["dir"] / "r")], engines=E)
    assert E.log == []


def test_flag_rules(capsys):
    from aiod_amd import deflicker
    assert deflicker.parse_args(["--video", "a.y4m"]).video_depth == "8" and deflicker.parse_args(["--video", "a.y4m", "--video_depth", "keep"]).video_depth == "keep"
    for argv, msg in ((["--frames_dir", "d", "--video_depth", "keep"], "--video_depth is an option of --video"),
                      (["--video", "a.y4m", "--video_depth", "10"], "invalid choice")):
        with pytest.raises(SystemExit):
            deflicker.parse_args(argv)
        assert msg in capsys.readouterr().err, argv
    Rp = TH._load("af_run_pipeline_deep", os.path.join(PKG, "run_pipeline.py"))
    o = Rp.parse_opts(["--in_process", "--video", "in/clip.y4m", "--video_out", "out.y4m", "--video_depth", "keep"])
    (kind, cmd), = Rp.build_commands(o)
    assert kind == "sh" and cmd.endswith("--video_out out.y4m --video_depth keep")
    o = Rp.parse_opts(["--in_process", "--video", "in/clip.y4m", "--video_out", "out.y4m"])
    assert "--video_depth" not in Rp.build_commands(o)[0][1]
    with pytest.raises(SystemExit):
        Rp.parse_opts(["--in_process", "--video_name", "a.mp4", "--video_depth", "keep"])
    assert "--video_depth is an option of --video" in capsys.readouterr().err


def test_y4m_cli_depth(deep_clip, capsys):
    from aiod_amd import y4m
    assert y4m.main(["--info", deep_clip["path"], "--video_depth", "keep"]) == 0
    info = json.loads(capsys.readouterr().out)
    assert (info["bits"], info["layout"], info["frame_bytes"]) == (10, "420jpeg", 2 * R8.frame_bytes(H, W, "420jpeg"))
    assert y4m.main(["--info", deep_clip["plain"]]) == 0 and json.loads(capsys.readouterr().out)["bits"] == 8
    with pytest.raises(SystemExit, match="only 8 bits per sample are handled"):
        y4m.main(["--info", deep_clip["path"]])
    with pytest.raises(SystemExit, match="--to_png: .*deep.y4m has 10 bits per sample and there is no 16-bit PNG route"):
        y4m.main(["--to_png", deep_clip["path"], str(deep_clip["dir"] / "png"), "--video_depth", "keep"])
    with pytest.raises(SystemExit, match="--from_png: --video_depth keep has no meaning here"):
        y4m.main(["--from_png", str(deep_clip["dir"]), str(deep_clip["dir"] / "x.y4m"), "--fps", "25", "--video_depth", "keep"])
    assert not (deep_clip["dir"] / "png").exists()


def test_run_bits_refusals_and_result():
    import aiod_amd
    deep = _deep_grey_clip()[:3]
    for bits in (8, 17, 0, True, 10.0):
        with pytest.raises(ValueError, match="bits must be None or an integer in 9..16"):
            aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=_DeepEngines()).run(deep, bits=bits)
    E = _DeepEngines()
    with pytest.raises(ValueError, match="bits=10: frame 0 must be uint16, got uint8"):
        aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=E).run(TH._frames(3), bits=10)
    with pytest.raises(ValueError, match="bits=10: frame 1 must be uint16, got uint8"):      # an iterator: named when the frame is seen
        aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=E).run(iter([deep[0], TH._frames(2)[1]]), bits=10)
    with pytest.raises(ValueError, match="bits needs an engine with frame16, reduce_depth and depth_transfer; _StubEngines lacks frame16, reduce_depth, depth_transfer"):
        aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=TH._StubEngines()).run(deep, bits=10)
    E = _DeepEngines()
    got = []
    res = aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=E).run(deep, bits=10, keep=("final", "stage1"), sink=lambda name, i, t: got.append((name, i, t.dtype)))
    assert res["final"].dtype == np.uint16 and res["final"].shape == (3, H, W, 3) and res["stage1"].dtype == np.uint8
    assert res["depth"]["bits"] == 10 and "proxy" not in res and list(res["seconds"])[0] == "depth" and "transfer" in res["seconds"]
    assert [g for g in got if g[0] == "final"] == [("final", i, np.dtype(np.uint16)) for i in range(3)]
    # a default run of the reduced frames makes the calls of the deep run minus the deep route's own
    plain = TH._StubEngines()
    aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=plain).run([R.reduce_depth(f, 10) for f in deep], keep=("final", "stage1"))
    assert [e for e in E.log if e[0] not in ("frame16", "reduce_depth", "depth_transfer")] == plain.log
