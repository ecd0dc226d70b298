"""Host-side checks of the YUV4MPEG2 route (no GPU): the numpy restatement of the two conversions (tests/y4m_ref.py)
against its fp64 exact twin and against Pillow, the identities the arithmetic promises, the parser and the writer, and the flags and
the orchestration of deflicker.py / run_pipeline.py with the stub engines of tests/test_deflicker_host.py (imported, not edited)."""
import argparse
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
import y4m_ref as R  # noqa: E402
import test_deflicker_host as TH  # noqa: E402

CASES = [(layout, matrix, full) for layout in R.LAYOUTS for matrix in R.MATRICES for full in (False, True)]
SIZES = ((7, 5), (197, 130))      # (w, h): odd edges on both axes; the pipeline tests' clip


# ---- the restatement against the exact twin --------------------------------------------------------------------------------------
def test_bounds_are_the_derived_ones():
    assert R.BITS == 14
    assert R.READ_BOUND == 0.5 + (255 + 128 + 128) * 2.0 ** -15 and abs(R.READ_BOUND - 0.5156) < 1e-4
    assert R.WRITE_BOUND == 0.5 + 3 * 255 * 2.0 ** -15


@pytest.mark.parametrize("layout,matrix,full", CASES)
def test_restatement_within_the_bound_of_exact(layout, matrix, full):
    for w, h in SIZES:
        for name, payload in R.inputs(h, w, layout):
            got = R.yuv_to_rgb(payload, h, w, layout, matrix, full).astype(np.float64)
            err = np.abs(got - R.yuv_to_rgb_exact(payload, h, w, layout, matrix, full)).max()
            assert err <= R.READ_BOUND, ("read", w, h, name, err)
        for name, img in R.rgb_inputs(h, w):
            got = R.rgb_to_yuv(img, layout, matrix, full).astype(np.float64)
            err = np.abs(got - R.rgb_to_yuv_exact(img, layout, matrix, full)).max()
            assert err <= R.WRITE_BOUND, ("write", w, h, name, err)


def test_coefficient_rows_sum_exactly():
    for matrix in R.MATRICES:
        for full in (False, True):
            (ky, ku, kv), inv = R.int_matrices(matrix, full)
            assert sum(ky) == (16384 if full else round(Fraction(219, 255) * 16384)) and sum(ku) == 0 and sum(kv) == 0
            fwd, rinv = R.real_matrices(matrix, full)
            for row, real in zip((ky, ku, kv), fwd):                  # the adjustment moves one entry by at most one unit
                assert all(abs(c - v * 16384) <= 1.05 for c, v in zip(row, real)), (matrix, full, row)
            assert all(abs(c - v * 16384) <= 0.5 for c, v in zip(inv, rinv))


# ---- an independent implementation: Pillow's JFIF (full-range BT.601) ------------------------------------------------------------
def test_within_one_level_of_pillow():
    from PIL import Image
    rng = np.random.default_rng(3)
    h = w = 1024                                                      # 2^20 random triples
    tri = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    payload = np.concatenate([tri[:, :, c].reshape(-1) for c in range(3)])
    ours = R.yuv_to_rgb(payload, h, w, "444", "bt601", True)
    theirs = np.asarray(Image.frombytes("YCbCr", (w, h), tri.tobytes()).convert("RGB"))
    assert np.abs(ours.astype(np.int64) - theirs).max() <= 1
    ours = R.rgb_to_yuv(tri, "444", "bt601", True).reshape(3, h, w).transpose(1, 2, 0)
    theirs = np.asarray(Image.frombytes("RGB", (w, h), tri.tobytes()).convert("YCbCr"))
    assert np.abs(ours.astype(np.int64) - theirs).max() <= 1


# ---- identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,matrix,full", CASES)
def test_grey_stays_grey(layout, matrix, full):
    h, w = 5, 7
    ch, cw = R.plane_size(h, w, layout)
    for v in range(256):
        p = R.rgb_to_yuv(np.full((h, w, 3), v, np.uint8), layout, matrix, full)
        assert (p[h * w:] == 128).all(), v                            # chroma exactly 128
        if full:
            assert (p[:h * w] == v).all(), v                          # and Y = v
        else:
            assert (p[:h * w] == 16 + ((14071 * v + 8192) >> 14)).all() and p[0] == round(16 + 219 * v / 255.0), v
        rgb = R.yuv_to_rgb(p, h, w, layout, matrix, full)
        assert (rgb == rgb[0, 0, 0]).all() and abs(int(rgb[0, 0, 0]) - v) <= (0 if full else 1), v
    assert p.size == h * w + 2 * ch * cw


@pytest.mark.parametrize("layout,matrix", [(lay, m) for lay in R.LAYOUTS for m in R.MATRICES])
def test_limited_range_end_points(layout, matrix):
    h, w = 4, 6
    for y, want in ((16, 0), (235, 255), (0, 0), (255, 255)):
        p = np.full(R.frame_bytes(h, w, layout), 128, np.uint8)
        p[:h * w] = y
        assert (R.yuv_to_rgb(p, h, w, layout, matrix, False) == want).all(), (y, want)


def test_mono_round_trips_exactly_in_full_range():
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for matrix in R.MATRICES:
        rgb = R.yuv_to_rgb(y.reshape(-1), 16, 16, "mono", matrix, True)
        assert (rgb == y[:, :, None]).all()
        assert np.array_equal(R.rgb_to_yuv(rgb, "mono", matrix, True), y.reshape(-1))


@pytest.mark.parametrize("matrix,full", [(m, f) for m in R.MATRICES for f in (False, True)])
def test_444_write_then_read(matrix, full):
    """RGB -> YCbCr -> RGB at 4:4:4.  The exact maps are inverses (an RGB byte triple never leaves the YCbCr cube, so nothing clamps),
    the written bytes are within WRITE_BOUND of exact, the exact reading is linear with rows (cy, 0, crv), (cy, cgu, cgv), (cy, cbu, 0), and
    the integer reading adds READ_BOUND; the output clamp only moves towards the original.  Hence per channel
    |back - rgb| <= WRITE_BOUND * (sum of the row's magnitudes) + READ_BOUND, and, both being integers, its floor."""
    _, inv = R.real_matrices(matrix, full)
    cy, crv, cgu, cgv, cbu = (abs(float(v)) for v in inv)
    bound = np.floor(R.WRITE_BOUND * np.array([cy + crv, cy + cgu + cgv, cy + cbu]) + R.READ_BOUND)
    assert (bound <= 2).all()                                         # at most 2 levels
    for w, h in SIZES:
        for name, img in R.rgb_inputs(h, w):
            back = R.yuv_to_rgb(R.rgb_to_yuv(img, "444", matrix, full), h, w, "444", matrix, full)
            err = np.abs(back.astype(np.int64) - img).reshape(-1, 3).max(0)
            assert (err <= bound).all(), (name, err, bound)


# ---- the sitings, pinned by hand -----------------------------------------------------------------------------------------------
def test_sitings_against_literals():
    """The restatement and its exact twin share their index and weight tables, so the tables themselves are held here against values
    worked out by hand from the definition: centred 3/4 own + 1/4 the neighbour on the pixel's side, left-cosited even x
    1 and odd x 1/2 + 1/2, edge clamp; on the way back the 2 covered pixels, or [1, 2, 1] around column 2j, indices clamped."""
    row = np.array([[0, 16]], np.uint8)                               # one chroma row of a 4 x 2 frame: vertical weight 4/4 after the clamp
    assert R.chroma16(row, 2, 4, "420jpeg").tolist() == [[0, 64, 192, 256]] * 2       # x: 3/4*0+1/4*0 | 3/4*0+1/4*16 | 3/4*16+1/4*0 | 3/4*16+1/4*16
    assert R.chroma16(row, 2, 4, "420mpeg2").tolist() == [[0, 128, 256, 256]] * 2     # x: 0 | (0+16)/2 | 16 | (16+16 clamped)/2
    assert R.chroma16(np.array([[0, 16], [16, 0]], np.uint8), 2, 4, "422").tolist() == [[0, 128, 256, 256], [256, 128, 0, 0]]      # no vertical mixing
    col = np.array([[0], [16]], np.uint8)                             # one chroma column of a 2 x 4 frame: both 4:2:0 layouts are centred vertically
    for layout in ("420jpeg", "420mpeg2"):
        assert R.chroma16(col, 4, 2, layout).tolist() == [[0, 0], [64, 64], [192, 192], [256, 256]]
    assert R.chroma16(np.array([[3, 5], [7, 9]], np.uint8), 2, 2, "444").tolist() == [[48, 80], [112, 144]]
    c = np.array([[0, 4, 8, 12]], np.int64)
    assert [v.tolist() if hasattr(v, "tolist") else v for v in R._filter(c, 1, 4, "422")] == [[[0 + 2 * 0 + 4, 4 + 2 * 8 + 12]], 2]      # left of column 0 clamps to it
    c = np.array([[0, 4, 8, 12], [4, 8, 12, 16]], np.int64)
    assert R._filter(c, 2, 4, "420jpeg")[0].tolist() == [[0 + 4 + 4 + 8, 8 + 12 + 12 + 16]] and R._filter(c, 2, 4, "420jpeg")[1] == 2
    assert R._filter(c, 2, 4, "420mpeg2")[0].tolist() == [[(0 + 0 + 4) + (4 + 8 + 8), (4 + 16 + 12) + (8 + 24 + 16)]] and R._filter(c, 2, 4, "420mpeg2")[1] == 3
    c = np.array([[0, 4, 8]], np.int64)                               # odd w and h: the last column and row are replicated
    assert R._filter(c, 1, 3, "420jpeg")[0].tolist() == [[2 * (0 + 4), 2 * (8 + 8)]]
    assert R._filter(c, 1, 3, "444")[0].tolist() == [[0, 4, 8]] and R._filter(c, 1, 3, "444")[1] == 0


# ---- parser and writer -----------------------------------------------------------------------------------------------------------
class _Pipe:
    """A stream that cannot seek and returns short reads, as a pipe does."""

    def __init__(self, data, chunk=7):
        self._b, self._chunk = io.BytesIO(data), chunk

    def read(self, n=-1):
        return self._b.read(min(n, self._chunk) if n is not None and n >= 0 else self._chunk)

    def seek(self, *a):
        raise io.UnsupportedOperation("seek")

    def tell(self):
        raise io.UnsupportedOperation("tell")


def _stream(header, payloads, frame_line=b"FRAME\n"):
    return header.encode() + b"\n" + b"".join(frame_line + bytes(p) for p in payloads)


@pytest.mark.parametrize("tag,layout", [("C420jpeg", "420jpeg"), ("C420", "420jpeg"), (None, "420jpeg"), ("C420mpeg2", "420mpeg2"), ("C422", "422"),
                                        ("C444", "444"), ("Cmono", "mono")])
def test_reader_accepts_every_spelling(tag, layout):
    from aiod_amd import Y4MReader
    w, h = 197, 130
    n = R.frame_bytes(h, w, layout)
    rng = np.random.default_rng(1)
    payloads = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(3)]
    header = "YUV4MPEG2 W197 H130 F30000:1001 Ip A1:1" + (" " + tag if tag else "") + " XYSCSS=whatever XCOLORRANGE=FULL"
    data = _stream(header, payloads, b"FRAME Xfoo=1 Ip\n")
    for src in (io.BytesIO(data), _Pipe(data)):
        r = Y4MReader(src)
        assert (r.width, r.height, r.layout, r.full_range, r.interlace) == (w, h, layout, True, "p")
        assert r.fps == Fraction(30000, 1001) and r.aspect == Fraction(1, 1) and r.frame_bytes == n
        assert r.tags == header.split(" ")[1:]                        # untouched
        got = list(r)
        assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, payloads)) and r.frames_read == 3
        assert r.frame_params == ["Xfoo=1", "Ip"] and got[0].dtype == np.uint8
    if layout == "420jpeg":
        assert n == 197 * 130 + 2 * 99 * 65                           # odd sizes: chroma 99 x 65
    r = Y4MReader(io.BytesIO(_stream("YUV4MPEG2 W4 H2 F25:1", [bytes(12)])))
    assert not r.full_range and r.layout == "420jpeg" and r.aspect is None and r.fps == 25 and len(list(r)) == 1


def test_reader_refusals_name_the_cause():
    from aiod_amd import Y4MError, Y4MReader
    head = "YUV4MPEG2 W4 H2 F25:1 Ip A1:1 "
    for tag in ("C420paldv", "C411", "C444alpha"):
        with pytest.raises(Y4MError, match="header tag '%s': chroma layout not handled" % tag):
            Y4MReader(io.BytesIO(_stream(head + tag, [])))
    for tag in ("C420p10", "C422p10", "C444p12", "C420p16", "C444p16", "Cmono9", "Cmono10", "Cmono12", "Cmono16"):
        with pytest.raises(Y4MError, match="header tag '%s': only 8 bits per sample.*add `-pix_fmt yuv420p` to the ffmpeg command" % tag):
            Y4MReader(io.BytesIO(_stream(head + tag, [])))
    for tag in ("It", "Ib", "Im"):
        with pytest.raises(Y4MError, match="header tag '%s': interlaced streams are not handled" % tag):
            Y4MReader(io.BytesIO(_stream("YUV4MPEG2 W4 H2 F25:1 %s A1:1 C420jpeg" % tag, [])))
    with pytest.raises(Y4MError, match="header tag 'Ix': unknown interlacing"):
        Y4MReader(io.BytesIO(_stream("YUV4MPEG2 W4 H2 F25:1 Ix A1:1 C420jpeg", [])))
    with pytest.raises(Y4MError, match="truncated header: the stream is empty"):
        Y4MReader(io.BytesIO(b""))
    with pytest.raises(Y4MError, match="truncated header: the stream ends after 17 bytes without a newline"):
        Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2 F"))
    with pytest.raises(Y4MError, match="not a YUV4MPEG2 stream"):
        Y4MReader(io.BytesIO(b"RIFF W4 H2\n"))
    with pytest.raises(Y4MError, match="without a positive W and H"):
        Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 F25:1\n"))
    with pytest.raises(Y4MError, match="header tag 'XCOLORRANGE=WIDE'"):
        Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2 XCOLORRANGE=WIDE\n"))
    good = _stream(head + "C420jpeg", [bytes(12), bytes(12)])
    r = Y4MReader(io.BytesIO(good[:-5]))
    next(r)
    with pytest.raises(Y4MError, match="truncated frame 1: 7 of 12 bytes"):
        next(r)
    r = Y4MReader(io.BytesIO(_stream(head + "C420jpeg", [bytes(12)]) + b"FRAMES\n" + bytes(12)))
    next(r)
    with pytest.raises(Y4MError, match="frame 1: expected a FRAME line, got b'FRAMES'"):
        next(r)
    r = Y4MReader(io.BytesIO(_stream(head + "C420jpeg", [bytes(12)]) + b"FRA"))
    next(r)
    with pytest.raises(Y4MError, match="truncated FRAME line of frame 1"):
        next(r)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_write_then_read_returns_the_bytes(layout, tmp_path):
    from aiod_amd import Y4MReader, Y4MWriter
    w, h = 197, 130
    rng = np.random.default_rng(2)
    payloads = [rng.integers(0, 256, R.frame_bytes(h, w, layout), dtype=np.uint8) for _ in range(2)]
    path = str(tmp_path / "clip.y4m")
    with Y4MWriter(path, w, h, Fraction(24000, 1001), layout, True, aspect=Fraction(4, 3)) as wr:
        wr.write(payloads[0])
        wr.write(payloads[1].tobytes())
        with pytest.raises(ValueError, match="frame 2 has 5 bytes"):
            wr.write(bytes(5))
    raw = open(path, "rb").read()
    assert raw.startswith(b"YUV4MPEG2 W197 H130 F24000:1001 Ip A4:3 C%s XCOLORRANGE=FULL\nFRAME\n" % layout.encode())
    with Y4MReader(path) as r:
        assert (r.width, r.height, r.layout, r.full_range, r.fps, r.aspect) == (w, h, layout, True, Fraction(24000, 1001), Fraction(4, 3))
        assert all(np.array_equal(a, b) for a, b in zip(list(r), payloads)) and r.frames_read == 2
    buf = io.BytesIO()
    Y4MWriter(buf, 4, 2, "25", "mono", False).close()
    assert buf.getvalue() == b"YUV4MPEG2 W4 H2 F25:1 Ip A0:0 Cmono XCOLORRANGE=LIMITED\n"
    for head in (b"YUV4MPEG2 W4 H2 F0:0 I? A0:0 Cmono", b"YUV4MPEG2 W4 H2 Cmono"):      # an unknown rate and interlacing are repeated as the format writes them
        r = Y4MReader(io.BytesIO(head + b"\n"))
        buf = io.BytesIO()
        Y4MWriter(buf, r.width, r.height, r.fps, r.layout, r.full_range, aspect=r.aspect, interlace=r.interlace).close()
        assert buf.getvalue() == b"YUV4MPEG2 W4 H2 F0:0 I%s A0:0 Cmono XCOLORRANGE=LIMITED\n" % r.interlace.encode() and r.fps == 0
    with pytest.raises(ValueError, match="only progressive streams are written"):
        Y4MWriter(io.BytesIO(), 4, 2, "25", "mono", False, interlace="t")


def test_resolve_matrix_is_the_documented_policy():
    from aiod_amd import resolve_matrix
    from aiod_amd.y4m import frame_bytes, resolve_range
    assert resolve_matrix("auto", 719, 1279) == "bt601" and resolve_matrix("auto", 720, 10) == "bt709" and resolve_matrix("auto", 10, 1280) == "bt709"
    assert resolve_matrix("bt601", 2160, 3840) == "bt601" and resolve_matrix("bt709", 2, 2) == "bt709"
    with pytest.raises(ValueError, match="unknown matrix"):
        resolve_matrix("bt2020", 2, 2)
    assert resolve_range("auto", True) and not resolve_range("auto", False) and resolve_range("full", False) and not resolve_range("limited", True)
    for layout in R.LAYOUTS:
        for w, h in ((1, 1), (2, 2), (3, 3), (197, 130), (1920, 1080)):
            assert frame_bytes(h, w, layout) == R.frame_bytes(h, w, layout)


def test_abi_declares_the_new_symbols():
    import re
    import aiod_amd
    hdr = open(os.path.join(ROOT, "include", "atlasfit.h")).read()
    declared = set(re.findall(r"\b(af_[a-z_0-9]+)\s*\(", hdr))
    for name in ("af_yuv_to_rgb", "af_rgb_to_yuv", "af_yuv_frame_bytes"):
        assert name in declared and name in aiod_amd.atlasfit.ABI_SYMBOLS
    for name in ("AF_YUV_444 = 0", "AF_YUV_422 = 1", "AF_YUV_420JPEG = 2", "AF_YUV_420MPEG2 = 3", "AF_YUV_MONO = 4", "AF_YUV_BT601 = 0", "AF_YUV_BT709 = 1"):
        assert name in hdr
    assert aiod_amd.y4m.LAYOUTS == R.LAYOUTS and aiod_amd.y4m.MATRICES == R.MATRICES
    assert hasattr(aiod_amd.deflicker.DeviceEngines, "yuv_to_rgb") and hasattr(aiod_amd.deflicker.DeviceEngines, "rgb_to_yuv")


# ---- flags and orchestration with stub engines -----------------------------------------------------------------------------------
class _VideoEngines(TH._StubEngines):
    """The stub engines of the one-process tests plus the hand-offs of the video route, computed by y4m_ref on the host."""

    def upload(self, arr):
        self.log.append(("payload", int(np.asarray(arr).size)))      # ("upload", ...) is the stub atlas's upload_video
        return np.asarray(arr)

    def yuv_to_rgb(self, payload, h, w, layout, matrix, full_range):
        self.log.append(("yuv_to_rgb", h, w, layout, matrix, bool(full_range)))
        return R.yuv_to_rgb(payload, h, w, layout, matrix, full_range)

    def rgb_to_yuv(self, img, layout, matrix, full_range):
        self.log.append(("rgb_to_yuv", TH._ident(img), layout, matrix, bool(full_range)))
        return R.rgb_to_yuv(np.asarray(img), layout, matrix, full_range)


H, W, N = 8, 12, 7


def _grey_clip():
    return [np.full((H, W, 3), 10 + i, np.uint8) for i in range(N)]      # grey in full range: every conversion is the identity on it


@pytest.fixture()
def clip(tmp_path):
    path = tmp_path / "clip.y4m"
    data = R.y4m_bytes(_grey_clip(), (25, 1), "420jpeg", "bt601", True)
    path.write_bytes(data)
    cfg = tmp_path / "small.json"
    cfg.write_text(json.dumps(TH.SMALL))
    return {"path": str(path), "bytes": data, "cfg": str(cfg), "dir": tmp_path}


def _expected_out(full=True, layout="420jpeg", matrix="bt601", fps="25:1", aspect="1:1"):
    head = ("YUV4MPEG2 W%d H%d F%s Ip A%s C%s XCOLORRANGE=%s\n" % (W, H, fps, aspect, layout, "FULL" if full else "LIMITED")).encode()
    return head + b"".join(b"FRAME\n" + R.rgb_to_yuv(f, layout, matrix, full).tobytes() for f in _grey_clip())


def test_video_run_call_list_and_record(clip):
    from aiod_amd import deflicker
    E = _VideoEngines()
    out = clip["dir"] / "res"
    assert deflicker.main(["--video", clip["path"], "--video_out", str(clip["dir"] / "out.y4m"), "--out", str(out), "--config", clip["cfg"], "--seed", "3"],
                          engines=E) == 0
    names = [e[0] for e in E.log]
    nbytes = R.frame_bytes(H, W, "420jpeg")
    # input: every payload uploaded as it is (1.5 bytes per pixel), converted, encoded, in order; the first conversion precedes RAFT's handle
    assert [e for e in E.log if e[0] == "payload"] == [("payload", nbytes)] * N and nbytes == H * W * 3 // 2
    assert [e for e in E.log if e[0] == "yuv_to_rgb"] == [("yuv_to_rgb", H, W, "420jpeg", "bt601", True)] * N
    assert names[:4] == ["payload", "yuv_to_rgb", "raft_open", "encode"]
    assert [e[1] for e in E.log if e[0] == "encode"] == [10 + i for i in range(N)]
    # output: every final frame converted once, in frame order, each after its own filter call
    assert [e for e in E.log if e[0] == "rgb_to_yuv"] == [("rgb_to_yuv", 10 + i, "420jpeg", "bt601", True) for i in range(N)]
    tail = [n for n in names if n in ("filter", "rgb_to_yuv")]
    assert tail == ["filter", "rgb_to_yuv"] * N
    assert (clip["dir"] / "out.y4m").read_bytes() == _expected_out()
    assert not (out / "final").exists()                               # no PNGs of the final frames
    rec = json.loads((out / "deflicker.json").read_text())
    assert rec["video"] == clip["path"] and rec["video_out"] == str(clip["dir"] / "out.y4m") and rec["fps"] == [25, 1]
    assert rec["yuv_layout"] == "420jpeg" and rec["yuv_matrix"] == "bt601" and rec["yuv_range"] == "full" and rec["frames"] == N
    assert rec["windows"] == [[0, 4], [4, 7]] and rec["seed"] == 3


def test_video_flags_override_the_policy_and_the_header(clip):
    from aiod_amd import deflicker
    E = _VideoEngines()
    out = clip["dir"] / "res"
    target = clip["dir"] / "o.y4m"
    deflicker.main(["--video", clip["path"], "--video_out", str(target), "--out", str(out), "--config", clip["cfg"], "--yuv_matrix", "bt709",
                    "--yuv_range", "limited"], engines=E)
    assert {e[3:] for e in E.log if e[0] == "yuv_to_rgb"} == {("420jpeg", "bt709", False)}
    assert {e[2:] for e in E.log if e[0] == "rgb_to_yuv"} == {("420jpeg", "bt709", False)}
    assert target.read_bytes().startswith(b"YUV4MPEG2 W12 H8 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n")
    rec = json.loads((out / "deflicker.json").read_text())
    assert rec["yuv_matrix"] == "bt709" and rec["yuv_range"] == "limited"


def test_pipes_stdout_is_the_stream_and_nothing_else(clip, capfdbinary, monkeypatch):
    from aiod_amd import deflicker

    class _Stdin:
        buffer = _Pipe(clip["bytes"], chunk=1000)
    monkeypatch.setattr(sys, "stdin", _Stdin())
    E = _VideoEngines()
    capfdbinary.readouterr()
    deflicker.main(["--video", "-", "--video_out", "-", "--out", str(clip["dir"] / "res"), "--config", clip["cfg"]], engines=E)
    sys.stdout.flush()
    got = capfdbinary.readouterr()
    assert got.out == _expected_out()                                  # header plus frames, not a byte more
    assert b"wrote 7 frames to standard output" in got.err             # the messages went to standard error
    rec = json.loads((clip["dir"] / "res" / "deflicker.json").read_text())
    assert rec["video"] == "-" and rec["video_out"] == "-" and rec["frames"] == N


def test_frames_dir_with_video_out_and_without_video_flags(clip):
    """--frames_dir with --video_out takes --fps and --yuv_layout; without any video flag the run makes no new engine call, on the stub
    engines as they were before the two methods existed, and writes the PNGs it always wrote."""
    from PIL import Image
    from aiod_amd import deflicker
    frames = clip["dir"] / "frames"
    frames.mkdir()
    for i, f in enumerate(_grey_clip()):
        Image.fromarray(f).save(str(frames / ("%05d.png" % i)))
    E = _VideoEngines()
    target = clip["dir"] / "fd.y4m"
    deflicker.main(["--frames_dir", str(frames), "--video_out", str(target), "--fps", "30000:1001", "--yuv_layout", "422", "--yuv_range", "full",
                    "--out", str(clip["dir"] / "a"), "--config", clip["cfg"]], engines=E)
    assert "payload" not in [e[0] for e in E.log] and "yuv_to_rgb" not in [e[0] for e in E.log]
    assert target.read_bytes() == _expected_out(layout="422", fps="30000:1001", aspect="0:0")
    rec = json.loads((clip["dir"] / "a" / "deflicker.json").read_text())
    assert (rec["video"], rec["fps"], rec["yuv_layout"], rec["yuv_matrix"], rec["yuv_range"]) == (None, [30000, 1001], "422", "bt601", "full")
    old = TH._StubEngines()
    assert not hasattr(old, "yuv_to_rgb") and not hasattr(old, "rgb_to_yuv") and not hasattr(old, "upload")
    deflicker.main(["--frames_dir", str(frames), "--out", str(clip["dir"] / "b"), "--config", clip["cfg"], "--seed", "3"], engines=old)
    direct = TH._StubEngines()
    import aiod_amd
    aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=3, engines=direct).run(_grey_clip(), sink=lambda *a: None)
    assert old.log == direct.log                                       # exactly the engine calls of a plain run
    pngs = sorted(os.listdir(clip["dir"] / "b" / "final" / "output"))
    assert pngs == ["%05d.png" % i for i in range(N)]
    assert all((np.asarray(Image.open(str(clip["dir"] / "b" / "final" / "output" / p))) == 10 + i).all() for i, p in enumerate(pngs))
    rec = json.loads((clip["dir"] / "b" / "deflicker.json").read_text())
    assert all(rec[k] is None for k in ("video", "video_out", "fps", "yuv_layout", "yuv_matrix", "yuv_range")) and rec["frames"] == N


def test_sink_device_hands_over_the_engines_tensor():
    import aiod_amd

    class _Dev(np.ndarray):
        """What the stub's device holds: to_host strips the class."""

    class _E(TH._StubEngines):
        def quantise(self, img):
            return TH._StubEngines.quantise(self, img).view(_Dev)

        def to_host(self, t):
            return np.asarray(t).view(np.ndarray)
    for flag in (False, True):
        got = []
        res = aiod_amd.Deflicker(None, None, None, config=TH.SMALL, seed=1, engines=_E()).run(
            TH._frames(3), sink=lambda name, i, t: got.append((name, i, type(t))), **({"sink_device": True} if flag else {}))
        assert got == [("final", i, _Dev if flag else np.ndarray) for i in range(3)] and type(res["final"]) is np.ndarray


def test_truncated_stream_ends_the_run_with_the_named_error(clip):
    from aiod_amd import deflicker
    cut = clip["dir"] / "cut.y4m"
    cut.write_bytes(clip["bytes"][:-40])
    E = _VideoEngines()
    with pytest.raises(SystemExit, match="cut.y4m: truncated frame 6: 104 of 144 bytes"):
        deflicker.main(["--video", str(cut), "--video_out", str(clip["dir"] / "o.y4m"), "--out", str(clip["dir"] / "r"), "--config", clip["cfg"]], engines=E)
    names = [e[0] for e in E.log]
    assert names.count("raft_open") == names.count("raft_close") == 1 and "atlas_open" not in names
    with pytest.raises(SystemExit, match="C420p10.*-pix_fmt yuv420p"):
        bad = clip["dir"] / "bad.y4m"
        bad.write_bytes(b"YUV4MPEG2 W4 H2 F25:1 Ip C420p10\n")
        deflicker.main(["--video", str(bad), "--out", str(clip["dir"] / "r")], engines=E)
    with pytest.raises(SystemExit, match="nowhere.y4m not found \\(--video\\)"):
        deflicker.main(["--video", str(clip["dir"] / "nowhere.y4m"), "--out", str(clip["dir"] / "r")], engines=E)
    assert deflicker.main(["--video", clip["path"], "--out", str(clip["dir"] / "r"), "--config", clip["cfg"]], engines=E) == 0      # and the process runs again


def test_flag_rules(capsys):
    from aiod_amd import deflicker
    o = deflicker.parse_args(["--video", "data/clip.y4m"])
    assert o.out == os.path.join("results", "clip") and o.frames_dir is None and o.video_out is None and o.yuv_matrix == "auto" and o.yuv_range == "auto"
    assert deflicker.parse_args(["--video", "-"]).out == os.path.join("results", "stdin")
    o = deflicker.parse_args(["--frames_dir", "d", "--video_out", "-", "--fps", "24"])
    assert o.fps == 24 and o.yuv_layout is None
    for argv, msg in ((["--video", "a.y4m", "--frames_dir", "d"], "--video and --frames_dir are mutually exclusive"),
                      ([], "the following arguments are required: --frames_dir"),
                      (["--out", "x"], "the following arguments are required: --frames_dir"),
                      (["--frames_dir", "d", "--video_out", "o.y4m"], "--video_out with --frames_dir needs --fps"),
                      (["--video", "a.y4m", "--fps", "25"], "with --video the output repeats the input stream's"),
                      (["--frames_dir", "d", "--yuv_matrix", "bt709"], "are options of --video / --video_out"),
                      (["--video", "a.y4m", "--yuv_matrix", "bt2020"], "invalid choice"),
                      (["--frames_dir", "d", "--video_out", "o", "--fps", "0"], "frame rate must be positive")):
        with pytest.raises(SystemExit):
            deflicker.parse_args(argv)
        assert msg in capsys.readouterr().err, argv


def test_run_pipeline_forwards_the_video_flags(capsys):
    Rp = TH._load("af_run_pipeline_y4m", os.path.join(PKG, "run_pipeline.py"))
    py = sys.executable or "python"
    o = Rp.parse_opts(["--in_process", "--video", "in/clip.y4m", "--video_out", "-", "--yuv_matrix", "bt709", "--yuv_range", "full", "--gpu", "1"])
    assert Rp.build_commands(o) == [("sh", "%s %s --video in/clip.y4m --out ./results/clip --gpu 1 --ckpt_filter ./pretrained_weights/neural_filter.pth "
                                           "--ckpt_local ./pretrained_weights/local_refinement_net.pth --video_out - --yuv_matrix bt709 --yuv_range full"
                                     % (py, os.path.join(PKG, "deflicker.py")))]
    o = Rp.parse_opts(["--in_process", "--video_name", "data/test/clip.mp4", "--fps", "12", "--video_out", "out.y4m"])
    cmds = Rp.build_commands(o)
    assert len(cmds) == 3 and cmds[2][1].endswith("--frames_dir ./data/test/clip --out ./results/clip --gpu 0 --ckpt_filter ./pretrained_weights/neural_filter.pth "
                                                  "--ckpt_local ./pretrained_weights/local_refinement_net.pth --video_out out.y4m --fps 12")
    for argv, msg in ((["--video", "a.y4m"], "they need --in_process"), (["--video_name", "a.mp4", "--video_out", "o.y4m"], "they need --in_process"),
                      (["--video_name", "a.mp4", "--yuv_matrix", "bt709"], "they need --in_process"), (["--video_name", "a.mp4", "--yuv_range", "full"], "they need --in_process"),
                      (["--in_process", "--video", "a.y4m", "--video_name", "b.mp4"], "--video replaces --video_name"),
                      (["--in_process", "--video", "a b.y4m"], "expected a plain file name")):
        with pytest.raises(SystemExit):
            Rp.parse_opts(argv)
        assert msg in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="needs --in_process"):
        Rp.build_commands(argparse.Namespace(video="a.y4m", in_process=False, video_name=None, video_frame_folder=None, fps=10, gpu=0, class_name=None))


def test_y4m_cli_info(clip, capsys):
    from aiod_amd import y4m
    assert y4m.main(["--info", clip["path"]]) == 0
    info = json.loads(capsys.readouterr().out)
    assert (info["width"], info["height"], info["fps"], info["layout"], info["range"], info["frame_bytes"]) == (W, H, [25, 1], "420jpeg", "full", 144)
    assert info["yuv_matrix_auto"] == "bt601" and info["tags"][:2] == ["W12", "H8"]
    with pytest.raises(SystemExit):
        y4m.parse_args(["--from_png", "d", "o.y4m"])
    assert "--from_png needs --fps" in capsys.readouterr().err
