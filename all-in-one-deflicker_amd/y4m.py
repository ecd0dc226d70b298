"""YUV4MPEG2 (.y4m) in and out: the uncompressed container every ffmpeg build reads and writes, on files and on pipes.

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python all-in-one-deflicker_amd/deflicker.py --video - --video_out - ... | ffmpeg -i - out.mp4

The parser and the writer are host code; YCbCr <-> RGB with chroma resampling runs on the device (csrc/yuv.hip, af_yuv_to_rgb /
af_rgb_to_yuv): integer arithmetic only, so the bytes are exact and the tests demand equality with numpy.  This package carries no
codec.  8 bits per sample, progressive, layouts 444, 422, 420jpeg, 420mpeg2 and mono; everything else is refused by name.

More than 8 bits per sample is opt-in: `Y4MReader(source, deep=True)` / `--video_depth keep` accept the tags ffmpeg's
yuv4mpegpipe writes, C420pN, C422pN, C444pN (N in 9, 10, 12, 14, 16) and CmonoN (N in 9, 10, 12, 16); a sample is then 16 bits little-endian
and a payload a numpy uint16 array.  C420pN is read as 420jpeg (centred siting), as C420 is: that is policy, the tag says nothing else.
The conversions are af_yuv_to_rgb16 / af_rgb_to_yuv16 (csrc/yuv16.hip), the 8-bit kernels' one body (csrc/yuv_core.h) at the stream's depth.  Code values
are scaled linearly; no transfer function (PQ, HLG) is interpreted, nothing is dithered.

    python all-in-one-deflicker_amd/y4m.py --info clip.y4m                      one JSON line
    python all-in-one-deflicker_amd/y4m.py --to_png clip.y4m DIR                DIR/%05d.png through the device conversion
    python all-in-one-deflicker_amd/y4m.py --from_png DIR out.y4m --fps N[:D] [--layout 420jpeg] [--yuv_matrix auto] [--yuv_range limited]

Y4M carries no matrix tag.  `--yuv_matrix auto` is policy, not detection: BT.709 when the frame is at least 720 rows high or 1280
columns wide, else BT.601 (resolve_matrix), which is what players assume for untagged material; the resolved name is recorded."""
import argparse
import json
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np

if __package__:      # run as a script this file only re-imports itself as part of the package (below)
    from ._residence import Device, Host

_HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUTS = ("444", "422", "420jpeg", "420mpeg2", "mono")      # index = AF_YUV_* of include/atlasfit.h
MATRICES = ("bt601", "bt709")                                # index = AF_YUV_BT*
RANGES = ("limited", "full")
MAGIC = b"YUV4MPEG2"
_TAGS = {"420jpeg": "420jpeg", "420": "420jpeg", "420mpeg2": "420mpeg2", "422": "422", "444": "444", "mono": "mono"}
_HEADER_LIMIT = 4096
_DEEP_TAG = re.compile(r"^(?:(420|422|444)p(9|10|12|14|16)|(mono)(9|10|12|16))$")      # what ffmpeg's yuv4mpegpipe writes above 8 bits
_DEEP_SS = {"444": "444", "422": "422", "420jpeg": "420", "mono": None}                 # ffmpeg's XYSCSS comment: C420p10 -> XYSCSS=420P10
DEPTHS = ("8", "keep")


def check_bits(bits, what, lo=8):
    """bits as an int, or ValueError: an integer in lo..16 (bits per sample of uint16 samples)."""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not lo <= int(bits) <= 16:
        raise ValueError("%s: bits must be an integer in %d..16, got %r" % (what, lo, bits))
    return int(bits)


class Y4MError(ValueError):
    pass


def layout_code(layout):
    if layout not in LAYOUTS:
        raise ValueError("unknown layout %r (known: %s)" % (layout, ", ".join(LAYOUTS)))
    return LAYOUTS.index(layout)


def matrix_code(matrix):
    if matrix not in MATRICES:
        raise ValueError("unknown matrix %r (known: %s; resolve_matrix turns auto into one)" % (matrix, ", ".join(MATRICES)))
    return MATRICES.index(matrix)


def resolve_matrix(matrix, h, w):
    """auto | bt601 | bt709 -> bt601 | bt709.  auto is policy: BT.709 when h >= 720 or w >= 1280, else BT.601."""
    if matrix == "auto":
        return "bt709" if (int(h) >= 720 or int(w) >= 1280) else "bt601"
    matrix_code(matrix)
    return matrix


def resolve_range(yuv_range, header_full_range):
    """auto | limited | full -> full_range (bool); auto follows the stream's header."""
    if yuv_range == "auto":
        return bool(header_full_range)
    if yuv_range not in RANGES:
        raise ValueError("unknown range %r (known: auto, %s)" % (yuv_range, ", ".join(RANGES)))
    return yuv_range == "full"


def frame_bytes(h, w, layout, bits=8):
    """Bytes of one frame payload: Y h x w, then Cb and Cr, each ceil(h / 2) or h by ceil(w / 2) or w (af_yuv_frame_bytes's arithmetic);
    above 8 bits per sample a sample takes two bytes."""
    code = layout_code(layout)
    h, w = int(h), int(w)
    per = 2 if check_bits(bits, "frame_bytes") > 8 else 1
    if code == 4:
        return h * w * per
    cw = w if code == 0 else (w + 1) // 2
    ch = (h + 1) // 2 if code in (2, 3) else h
    return (h * w + 2 * ch * cw) * per


def parse_fps(text):
    """N or N:D or N/D -> Fraction."""
    t = str(text).replace("/", ":")
    n, _, d = t.partition(":")
    try:
        f = Fraction(int(n), int(d) if d else 1)
    except (ValueError, ZeroDivisionError):
        raise argparse.ArgumentTypeError("expected N or N:D, got %r" % text)
    if f <= 0:
        raise argparse.ArgumentTypeError("the frame rate must be positive, got %r" % text)
    return f


def _open(target, mode):
    """(file object, owned): a path is opened, '-' is the process's binary stdin / stdout, a file object is used as it is."""
    if hasattr(target, "read") or hasattr(target, "write"):
        return target, False
    if str(target) == "-":
        return (sys.stdin.buffer if "r" in mode else sys.stdout.buffer), False
    return open(str(target), mode), True


def _read_exact(f, n):
    """Up to n bytes from a stream that may return short reads (a pipe), as a writable uint8 array of what arrived."""
    buf, got = np.empty(n, np.uint8), 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        buf[got:got + len(b)] = np.frombuffer(b, np.uint8)
        got += len(b)
    return buf[:got]


def _read_line(f, what):
    """One '\\n'-terminated line without the terminator, read a byte at a time (the stream need not seek); None at a clean end."""
    out = bytearray()
    while True:
        b = f.read(1)
        if not b:
            if not out:
                return None
            raise Y4MError("truncated %s: the stream ends after %d bytes without a newline" % (what, len(out)))
        if b == b"\n":
            return bytes(out)
        out += b
        if len(out) > _HEADER_LIMIT:
            raise Y4MError("%s: no newline within %d bytes: not a YUV4MPEG2 stream" % (what, _HEADER_LIMIT))


class Y4MReader:
    """Iterates the frame payloads (numpy uint8, frame_bytes long) of a YUV4MPEG2 stream given as a path, '-' (stdin) or a binary file
    object; the stream need not seek.  Attributes: width, height, fps (Fraction), aspect (Fraction or None), interlace, layout,
    full_range (XCOLORRANGE=FULL; default limited), tags (the header's tags as written), frame_params (the parameters of the last FRAME
    line), frames_read, bits (8, or with deep=True the depth of a C420pN / C422pN / C444pN / CmonoN stream, whose payloads are numpy
    uint16 arrays, views of the little-endian bytes read).  Without deep=True a stream above 8 bits is refused at the header."""

    def __init__(self, source, deep=False):
        self.deep, self.bits = bool(deep), 8
        self._f, self._own = _open(source, "rb")
        try:
            self._parse_header()
        except BaseException:
            self.close()
            raise
        self.frames_read, self.frame_params = 0, []

    def _parse_header(self):
        line = _read_line(self._f, "header")
        if line is None:
            raise Y4MError("truncated header: the stream is empty")
        try:
            fields = line.decode("ascii").split(" ")
        except UnicodeDecodeError:
            raise Y4MError("not a YUV4MPEG2 stream: the first line is not ASCII")
        if fields[0] != MAGIC.decode():
            raise Y4MError("not a YUV4MPEG2 stream: the first line starts with %r" % fields[0][:16])
        self.tags = [t for t in fields[1:] if t]
        self.width = self.height = None
        self.fps, self.aspect, self.interlace, self.layout, self.full_range = Fraction(0), None, "p", "420jpeg", False
        for t in self.tags:
            key, val = t[0], t[1:]
            try:
                if key == "W":
                    self.width = int(val)
                elif key == "H":
                    self.height = int(val)
                elif key == "F":
                    n, d = val.split(":")
                    self.fps = Fraction(int(n), int(d)) if int(d) else Fraction(0)      # F0:0: the format's "unknown rate"
                    if self.fps < 0:
                        raise ValueError(t)
                elif key == "A":
                    n, d = val.split(":")
                    self.aspect = Fraction(int(n), int(d)) if int(n) and int(d) else None
            except ValueError:
                raise Y4MError("header tag %r does not parse" % t)
            if key == "I":
                if val in ("t", "b", "m"):
                    raise Y4MError("header tag %r: interlaced streams are not handled (deinterlace first, e.g. ffmpeg -vf yadif)" % t)
                if val not in ("p", "?"):
                    raise Y4MError("header tag %r: unknown interlacing (handled: Ip, I?)" % t)
                self.interlace = val
            elif key == "C":
                m = _DEEP_TAG.match(val) if self.deep else None
                if m:
                    self.layout, self.bits = _TAGS[m.group(1) or m.group(3)], int(m.group(2) or m.group(4))
                    continue
                if re.search(r"(p|mono)(9|10|12|14|16)$", val):
                    if self.deep:
                        raise Y4MError("header tag %r: deep layout not handled (handled: C420pN, C422pN, C444pN for N in 9, 10, 12, 14, 16; CmonoN for N in 9, 10, 12, 16)" % t)
                    raise Y4MError("header tag %r: only 8 bits per sample are handled; add `-pix_fmt yuv420p` to the ffmpeg command, "
                                   "or keep the depth with --video_depth keep (Y4MReader(deep=True))" % t)
                if val not in _TAGS:
                    raise Y4MError("header tag %r: chroma layout not handled (handled: C420jpeg, C420, C420mpeg2, C422, C444, Cmono)" % t)
                self.layout = _TAGS[val]
            elif key == "X" and val.upper().startswith("COLORRANGE="):
                rng = val.split("=", 1)[1].upper()
                if rng not in ("FULL", "LIMITED"):
                    raise Y4MError("header tag %r: expected XCOLORRANGE=FULL or XCOLORRANGE=LIMITED" % t)
                self.full_range = rng == "FULL"
        if not self.width or not self.height or self.width < 1 or self.height < 1:
            raise Y4MError("header without a positive W and H: %r" % line.decode("ascii"))
        self.frame_bytes = frame_bytes(self.height, self.width, self.layout, self.bits)

    def info(self):
        out = {"width": self.width, "height": self.height, "fps": [self.fps.numerator, self.fps.denominator],
               "aspect": [self.aspect.numerator, self.aspect.denominator] if self.aspect is not None else None, "interlace": self.interlace,
               "layout": self.layout, "range": "full" if self.full_range else "limited", "frame_bytes": self.frame_bytes, "tags": self.tags}
        if self.deep:
            out["bits"] = self.bits
        return out

    def __iter__(self):
        return self

    def __next__(self):
        line = _read_line(self._f, "FRAME line of frame %d" % self.frames_read)
        if line is None:
            raise StopIteration
        fields = line.split(b" ")
        if fields[0] != b"FRAME":
            raise Y4MError("frame %d: expected a FRAME line, got %r" % (self.frames_read, line[:32]))
        self.frame_params = [p.decode("ascii", "replace") for p in fields[1:] if p]
        data = _read_exact(self._f, self.frame_bytes)
        if len(data) != self.frame_bytes:
            raise Y4MError("truncated frame %d: %d of %d bytes" % (self.frames_read, len(data), self.frame_bytes))
        self.frames_read += 1
        return data.view("<u2") if self.bits > 8 else data

    def close(self):
        if self._own and self._f is not None:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes a progressive YUV4MPEG2 stream to a path, '-' (stdout) or a binary file object: the header with XCOLORRANGE, then
    write(payload) per frame.  bits above 8: the tag is C<layout>p<bits> (Cmono<bits>) followed by ffmpeg's XYSCSS comment, and a payload
    is uint16 samples, written little-endian."""

    def __init__(self, target, width, height, fps, layout, full_range, aspect=None, interlace="p", bits=8):
        layout_code(layout)
        self.bits = check_bits(bits, "Y4MWriter")
        if self.bits > 8:
            if layout == "420mpeg2":
                raise ValueError("Y4MWriter: 420mpeg2 has no tag above 8 bits per sample (ffmpeg writes C420pN, which is read as 420jpeg)")
            if self.bits not in ((9, 10, 12, 16) if layout == "mono" else (9, 10, 12, 14, 16)):
                raise ValueError("Y4MWriter: no %s tag at %d bits per sample (9, 10, 12%s or 16)" % (layout, self.bits, "" if layout == "mono" else ", 14"))
        if interlace not in ("p", "?"):
            raise ValueError("Y4MWriter: only progressive streams are written (interlace 'p', or '?' for unknown), got %r" % (interlace,))
        self.interlace = interlace
        self.width, self.height, self.layout, self.full_range = int(width), int(height), layout, bool(full_range)
        if self.width < 1 or self.height < 1:
            raise ValueError("Y4MWriter: width and height must be positive, got %dx%d" % (self.width, self.height))
        self.fps = fps if isinstance(fps, Fraction) else parse_fps(fps)      # Fraction(0): an unknown rate, written F0:0 as the format has it
        if self.fps < 0:
            raise ValueError("Y4MWriter: the frame rate must not be negative, got %s" % (self.fps,))
        self.aspect = aspect
        self.frame_bytes = frame_bytes(self.height, self.width, layout, self.bits)
        self.frames_written = 0
        self._f, self._own = _open(target, "wb")
        self._f.write(self.header())

    def header(self):
        a = "%d:%d" % (self.aspect.numerator, self.aspect.denominator) if self.aspect is not None else "0:0"
        if self.bits > 8:
            ss = _DEEP_SS[self.layout]      # ffmpeg writes the comment for the colour layouts only
            tag = "mono%d" % self.bits if self.layout == "mono" else "%sp%d XYSCSS=%sP%d" % (ss, self.bits, ss, self.bits)
            return ("YUV4MPEG2 W%d H%d F%d:%d I%s A%s C%s XCOLORRANGE=%s\n"
                    % (self.width, self.height, self.fps.numerator, self.fps.denominator if self.fps else 0, self.interlace, a, tag,
                       "FULL" if self.full_range else "LIMITED")).encode("ascii")
        return ("YUV4MPEG2 W%d H%d F%d:%d I%s A%s C%s XCOLORRANGE=%s\n" % (self.width, self.height, self.fps.numerator, self.fps.denominator if self.fps else 0, self.interlace, a,
                                                                         self.layout, "FULL" if self.full_range else "LIMITED")).encode("ascii")

    def write(self, payload):
        if self.bits > 8:
            p = np.asarray(payload)
            if p.dtype != np.uint16 or 2 * p.size != self.frame_bytes:
                raise ValueError("Y4MWriter: frame %d is %d %s samples, a %dx%d %s frame at %d bits has %d uint16 samples"
                                 % (self.frames_written, p.size, p.dtype, self.width, self.height, self.layout, self.bits, self.frame_bytes // 2))
            self._f.write(b"FRAME\n")
            self._f.write(np.ascontiguousarray(p).astype("<u2", copy=False).tobytes())
            self.frames_written += 1
            return
        p = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1) if not isinstance(payload, (bytes, bytearray, memoryview)) else payload
        n = p.size if hasattr(p, "size") else len(p)
        if n != self.frame_bytes:
            raise ValueError("Y4MWriter: frame %d has %d bytes, a %dx%d %s frame has %d" % (self.frames_written, n, self.width, self.height, self.layout, self.frame_bytes))
        self._f.write(b"FRAME\n")
        self._f.write(p.tobytes() if hasattr(p, "tobytes") else p)
        self.frames_written += 1

    def close(self):
        if self._f is not None:
            self._f.flush()
            if self._own:
                self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the conversions, through the C ABI ------------------------------------------------------------------------------------------
# Each direction is written once, over a residence and a depth; the public names below bind them.
#   residence (_residence.py): Host(device) for host pointers; Device(tensor.device, device) for device pointers, whose outputs land on the
#     tensor's device and which, for device=None, names that device to the library.
#   depth: "uint8" calls af_yuv_to_rgb / af_rgb_to_yuv, which take no bits; "uint16" (csrc/yuv16.hip) calls their "16"
#     siblings with bits before the output.  frame_bytes at 8 bits is the payload's sample count at every depth.
def _to_rgb(what, res, payload, h, w, layout, matrix, full_range, dtype="uint8", bits=None):
    from .atlasfit import load_library, _util_chk
    codes = (layout_code(layout), matrix_code(matrix), int(bool(full_range)))
    bits = None if dtype == "uint8" else check_bits(bits, what)
    src, n = res.array(payload), frame_bytes(h, w, layout)
    if not res.typed(src, dtype) or math.prod(src.shape) != n:
        unit = "bytes" if bits is None else "samples"
        want = "a %s CUDA tensor of %d %s" % (dtype, n, unit) if res.on_device else "%d %s %s" % (n, dtype, unit)
        raise ValueError("%s: expected %s for a %dx%d %s frame, got %d %s" % (what, want, w, h, layout, math.prod(src.shape), src.dtype))
    src, dst = res.contiguous(src), res.empty((int(h), int(w), 3), dtype)
    res.sync()
    entry = getattr(load_library(), "af_yuv_to_rgb" if bits is None else "af_yuv_to_rgb16")
    _util_chk(entry(res.ordinal, res.ptr(src), int(h), int(w), *codes, *(() if bits is None else (bits,)), res.ptr(dst), res.on_device))
    return dst


def _to_yuv(what, res, rgb, layout, matrix, full_range, dtype="uint8", bits=None):
    from .atlasfit import load_library, _util_chk
    codes = (layout_code(layout), matrix_code(matrix), int(bool(full_range)))
    bits = None if dtype == "uint8" else check_bits(bits, what)
    img = res.array(rgb)
    if not res.typed(img, dtype) or len(img.shape) != 3 or img.shape[2] != 3:
        raise ValueError("%s: expected an (H, W, 3) %s %s, got %s %s" % (what, dtype, "CUDA tensor" if res.on_device else "image", tuple(img.shape), img.dtype))
    src = res.contiguous(img)
    h, w = int(src.shape[0]), int(src.shape[1])
    dst = res.empty((frame_bytes(h, w, layout),), dtype)
    res.sync()
    entry = getattr(load_library(), "af_rgb_to_yuv" if bits is None else "af_rgb_to_yuv16")
    _util_chk(entry(res.ordinal, res.ptr(src), h, w, *codes, *(() if bits is None else (bits,)), res.ptr(dst), res.on_device))
    return dst


def yuv_to_rgb(payload, h, w, layout, matrix, full_range, device=0):
    """One frame payload (bytes or numpy uint8) -> (h, w, 3) uint8 RGB, through host pointers (af_yuv_to_rgb stages both sides)."""
    if isinstance(payload, (bytes, bytearray, memoryview)):
        payload = np.frombuffer(payload, np.uint8)
    return _to_rgb("yuv_to_rgb", Host(device), payload, h, w, layout, matrix, full_range)


def rgb_to_yuv(rgb, layout, matrix, full_range, device=0):
    """(h, w, 3) uint8 RGB -> one frame payload (numpy uint8), through host pointers (af_rgb_to_yuv)."""
    return _to_yuv("rgb_to_yuv", Host(device), rgb, layout, matrix, full_range)


def yuv_to_rgb_device(payload, h, w, layout, matrix, full_range, device=None):
    """The same on the device: payload a 1-D uint8 CUDA tensor, returns an (h, w, 3) uint8 CUDA tensor."""
    return _to_rgb("yuv_to_rgb_device", Device(payload.device, device), payload, h, w, layout, matrix, full_range)


def rgb_to_yuv_device(rgb, layout, matrix, full_range, device=None):
    """(h, w, 3) uint8 CUDA tensor -> the frame payload as a 1-D uint8 CUDA tensor."""
    return _to_yuv("rgb_to_yuv_device", Device(rgb.device, device), rgb, layout, matrix, full_range)


def yuv_to_rgb16(payload, h, w, layout, matrix, full_range, bits, device=0):
    """One frame payload of uint16 samples holding `bits` (8..16) bits -> (h, w, 3) uint16 RGB at the same depth, through host pointers
    (af_yuv_to_rgb16).  A sample above 2^bits - 1 reads as that maximum."""
    return _to_rgb("yuv_to_rgb16", Host(device), payload, h, w, layout, matrix, full_range, "uint16", bits)


def rgb16_to_yuv(rgb, layout, matrix, full_range, bits, device=0):
    """(h, w, 3) uint16 RGB holding `bits` bits -> one frame payload (numpy uint16), through host pointers (af_rgb_to_yuv16)."""
    return _to_yuv("rgb16_to_yuv", Host(device), rgb, layout, matrix, full_range, "uint16", bits)


def yuv_to_rgb16_device(payload, h, w, layout, matrix, full_range, bits, device=None):
    """The same on the device: payload a 1-D torch.uint16 CUDA tensor, returns an (h, w, 3) torch.uint16 CUDA tensor (storage only: torch
    has few operators for the type)."""
    return _to_rgb("yuv_to_rgb16_device", Device(payload.device, device), payload, h, w, layout, matrix, full_range, "uint16", bits)


def rgb16_to_yuv_device(rgb, layout, matrix, full_range, bits, device=None):
    """(h, w, 3) torch.uint16 CUDA tensor -> the frame payload as a 1-D torch.uint16 CUDA tensor."""
    return _to_yuv("rgb16_to_yuv_device", Device(rgb.device, device), rgb, layout, matrix, full_range, "uint16", bits)


# ---- the small CLI ---------------------------------------------------------------------------------------------------------------
def add_yuv_arguments(p):
    p.add_argument("--yuv_matrix", type=str, default="auto", choices=("auto",) + MATRICES,
                   help="YCbCr matrix of the video streams (Y4M carries no matrix tag).  auto is policy: bt709 when the frame is at least 720 rows "
                        "high or 1280 columns wide, else bt601")
    p.add_argument("--yuv_range", type=str, default="auto", choices=("auto",) + RANGES,
                   help="sample range of the video streams: auto follows the input's XCOLORRANGE tag (limited without one; limited for frames from a folder)")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="YUV4MPEG2 streams: describe one, or convert to / from a folder of PNG frames on the MI355X")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--info", metavar="Y4M", help="print one JSON line describing the stream (header only)")
    g.add_argument("--to_png", nargs=2, metavar=("Y4M", "DIR"), help="write DIR/%%05d.png through the device conversion")
    g.add_argument("--from_png", nargs=2, metavar=("DIR", "Y4M"), help="write the folder's frames (*.jpg / *.png, by name) as a stream; needs --fps")
    p.add_argument("--fps", type=parse_fps, default=None, help="N or N:D (--from_png)")
    p.add_argument("--layout", type=str, default="420jpeg", choices=LAYOUTS, help="chroma layout of the written stream (--from_png)")
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--video_depth", type=str, default="8", choices=DEPTHS,
                   help="8: a stream above 8 bits per sample is refused; keep: --info describes it (bits)")
    add_yuv_arguments(p)
    o = p.parse_args(argv)
    if o.from_png and o.fps is None:
        p.error("--from_png needs --fps")
    return o


def main(argv=None):
    o = parse_args(argv)
    if o.info:
        try:
            with Y4MReader(o.info, deep=o.video_depth == "keep") as r:
                info = r.info()
                info["bits"] = r.bits
        except Y4MError as e:
            raise SystemExit(str(e))
        info["yuv_matrix_auto"] = resolve_matrix("auto", info["height"], info["width"])
        print(json.dumps(info))
        return 0
    if o.video_depth == "keep":      # a deep stream has no PNG route here: refuse it by name, before anything else
        if o.to_png:
            with Y4MReader(o.to_png[0], deep=True) as r:
                if r.bits > 8:
                    raise SystemExit("--to_png: %s has %d bits per sample and there is no 16-bit PNG route; convert with --video_depth 8 after "
                                     "`-pix_fmt yuv420p`, or run deflicker.py --video_depth keep --video_out" % (o.to_png[0], r.bits))
        else:
            raise SystemExit("--from_png: --video_depth keep has no meaning here: PNG frames are read as 8 bits per sample")
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: the conversion has no CPU path")
    dev = torch.device("cuda", o.gpu)
    try:
        if o.to_png:
            src, folder = o.to_png
            os.makedirs(folder, exist_ok=True)
            with Y4MReader(src) as r:
                matrix, full = resolve_matrix(o.yuv_matrix, r.height, r.width), resolve_range(o.yuv_range, r.full_range)
                for i, payload in enumerate(r):
                    rgb = yuv_to_rgb_device(torch.from_numpy(payload).to(dev), r.height, r.width, r.layout, matrix, full)
                    Image.fromarray(rgb.cpu().numpy()).save(os.path.join(folder, "%05d.png" % i))
                n = r.frames_read
            print(json.dumps({"frames": n, "yuv_matrix": matrix, "yuv_range": "full" if full else "limited", "layout": r.layout}))
            return 0
        from .neural_filter import read_png
        from .warp_error import list_frames
        folder, dst = o.from_png
        files = list_frames(folder)
        if not files:
            raise SystemExit("no frames (*.jpg / *.png) under %s" % folder)
        first = read_png(str(files[0]))
        h, w = first.shape[:2]
        matrix, full = resolve_matrix(o.yuv_matrix, h, w), resolve_range(o.yuv_range, False)
        with Y4MWriter(dst, w, h, o.fps, o.layout, full) as wr:
            for path in files:
                img = read_png(str(path))
                if img.dtype != np.uint8 or img.shape != first.shape:
                    raise SystemExit("%s: expected an 8-bit %dx%d frame" % (path, w, h))
                wr.write(rgb_to_yuv_device(torch.from_numpy(img).to(dev), o.layout, matrix, full).cpu().numpy())
        if dst != "-":
            print(json.dumps({"frames": len(files), "yuv_matrix": matrix, "yuv_range": "full" if full else "limited", "layout": o.layout}))
        return 0
    except Y4MError as e:
        raise SystemExit(str(e))


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import y4m as _y
        sys.exit(_y.main())
    sys.exit(main())
