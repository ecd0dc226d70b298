"""Residual guided transfer: a correction computed on a proxy-size copy of a frame, carried to the full-size frame.

Flicker is a low-frequency colour error, so the pipeline may run on a shrunk copy of the clip (`Deflicker(proxy_long_edge=N)`) and hand
its result up.  For one frame: F is the full-size frame, I its area shrink (the proxy input) and P the pipeline's final frame at the proxy
size.  Per channel the fast guided filter (He & Sun) of the residual d = P - I with guide I gives a gain a and an offset b per proxy
pixel, d ~ a I + b over a (2r + 1)^2 window, regularised by eps (in squared 8-bit levels); their box means are sampled bilinearly at the
full-size pixel centres and out = clamp(rint(F + (a F + b)), 0, 255).  Every detail above the proxy's resolution is the input frame's own.

P == I returns F byte for byte; P == I + c with nothing clipped returns F + c.  The kernels (csrc/guided.hip, af_guided_coeffs and
af_guided_apply) compute every value in one fixed order of correctly rounded operations, so the result is the same everywhere and equal
to a numpy restatement.

With the colour guide (the *_colour functions below, Deflicker(proxy_guide="colour")) every output channel is fitted on all
three guide channels, d_k ~ sum_c A_kc I_c + b_k: a 3 x 3 solve per proxy pixel in fp64 (af_guided_coeffs_colour), A (h, w, 9) with entry
3k + c, and out_k = clamp(rint(F_k + (sum_c A_kc F_c + b_k))) (af_guided_apply_colour), so the field can carry a correction that mixes
channels.  The default guide, "channel", is the above; guided_coeffs, guided_transfer and depth_transfer keep their signatures, and the
colour guide has names of its own (guided_coeffs_colour, guided_transfer_colour, depth_transfer_colour), as it has in the C ABI.

DEFAULT_RADIUS and DEFAULT_EPS are policy: nobody has measured them on footage."""
import math

import numpy as np

from ._residence import Host, one_device
from .y4m import check_bits

DEFAULT_RADIUS = 8       # window radius in proxy pixels (1..32)
DEFAULT_EPS = 64.0       # squared 8-bit levels: a window whose guide varies by less than ~8 levels gets an offset, hardly a gain
MAX_RADIUS = 32
GUIDES = ("channel", "colour")
COLOUR_EPS_FLOOR = 2.0 ** -20      # af_guided_coeffs_colour's: the pivots of its fp64 solve are at least eps n^2


def check_guide(guide, what="guided transfer"):
    if not isinstance(guide, str) or guide not in GUIDES:
        raise ValueError("%s: guide must be one of %s, got %r" % (what, ", ".join(GUIDES), guide))
    return guide


def check_guided(radius, eps, what="guided transfer", guide="channel"):
    """(radius, eps) as (int, float), or ValueError: radius an integer in 1..32, eps finite and > 0 (as the fp32 the library receives), and
    at least 2^-20 with the colour guide."""
    check_guide(guide, what)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in 1..%d, got %r" % (what, MAX_RADIUS, radius))
    try:
        e = float(np.float32(eps))
    except (TypeError, ValueError):
        raise ValueError("%s: eps must be a number, got %r" % (what, eps))
    if not np.isfinite(e) or e <= 0:
        raise ValueError("%s: eps must be finite and > 0 (in fp32), got %r" % (what, eps))
    if guide == "colour" and e < COLOUR_EPS_FLOOR:
        raise ValueError("%s: eps must be at least 2^-20 with the colour guide, got %r" % (what, eps))
    return int(radius), e


# Every operation below is written once over a residence `res` (_residence.py): Host(device) for numpy arrays through host pointers, or,
# from the *_device bindings (res None), the Device of CUDA tensors that must all live on one device.
def _on(what, res, tensors):
    return res or one_device(tensors, "%s: the images must be CUDA tensors on one device (host arrays go through the function without _device)" % what)


def _check_image(x, name, what, res, dtype="uint8"):
    if not hasattr(x, "shape") or len(x.shape) != 3 or x.shape[2] != 3 or str(x.dtype) != ("torch." if res.on_device else "") + dtype:
        raise ValueError("%s: %s must be (H, W, 3) %s, got %s %s" % (what, name, dtype, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x).__name__)))
    return int(x.shape[0]), int(x.shape[1])


def _check_pair(proxy_in, proxy_out, what, res):
    h, w = _check_image(proxy_in, "proxy_in", what, res)
    if _check_image(proxy_out, "proxy_out", what, res) != (h, w):
        raise ValueError("%s: proxy_in is %dx%d, proxy_out %dx%d" % (what, w, h, proxy_out.shape[1], proxy_out.shape[0]))
    return h, w


def _check_full(full, h, w, what, res, dtype="uint8"):
    H, W = _check_image(full, "full", what, res, dtype)
    if h > H or w > W:
        raise ValueError("%s: the proxy (%dx%d) is larger than the full frame (%dx%d)" % (what, w, h, W, H))
    return H, W


def _check_planes(a, b, what, res, na=3):
    for name, x, nch in (("A" if na == 9 else "a", a, na), ("b", b, 3)):
        if not hasattr(x, "shape") or len(x.shape) != 3 or x.shape[2] != nch or str(x.dtype) != ("torch." if res.on_device else "") + "float32":
            raise ValueError("%s: %s must be (h, w, %d) float32, got %s %s" % (what, name, nch, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x).__name__)))
    if tuple(a.shape[:2]) != tuple(b.shape[:2]):
        raise ValueError("%s: a is %dx%d, b %dx%d" % (what, a.shape[1], a.shape[0], b.shape[1], b.shape[0]))
    return int(a.shape[0]), int(a.shape[1])


def _coeffs(what, res, proxy_in, proxy_out, radius, eps, guide="channel"):
    from .atlasfit import load_library, _util_chk
    radius, eps = check_guided(radius, eps, what, guide)
    res = _on(what, res, [proxy_in, proxy_out])
    h, w = _check_pair(proxy_in, proxy_out, what, res)
    i, p = res.contiguous(proxy_in), res.contiguous(proxy_out)
    colour = guide == "colour"
    a, b = res.empty((h, w, 9 if colour else 3), "float32"), res.empty((h, w, 3), "float32")
    # the unsmoothed planes (colour: after the 21 planes of window sums), from torch's allocator: no hipMalloc per frame
    work = res.empty((33, h, w) if colour else (2, h, w, 3), "float32") if res.on_device else None
    res.sync()
    entry = load_library().af_guided_coeffs_colour if colour else load_library().af_guided_coeffs
    _util_chk(entry(res.ordinal, res.ptr(i), res.ptr(p), h, w, radius, eps, res.ptr(a), res.ptr(b), res.ptr(work), res.on_device))
    return a, b


def _apply(what, res, full, a, b, dtype="uint8", bits=None, guide="channel"):
    """af_guided_apply on a uint8 frame, af_guided_apply16 with `bits` on a uint16 one; their _colour siblings with the colour guide's A."""
    from .atlasfit import load_library, _util_chk
    bits = None if dtype == "uint8" else check_bits(bits, what)
    res = _on(what, res, [full, a, b])
    h, w = _check_planes(a, b, what, res, 9 if guide == "colour" else 3)
    H, W = _check_full(full, h, w, what, res, dtype)
    f, pa, pb = res.contiguous(full), res.contiguous(a), res.contiguous(b)
    out = res.empty((H, W, 3), dtype)
    res.sync()
    lib, tail = load_library(), (res.ptr(pa), res.ptr(pb), h, w, res.ptr(out), res.on_device)
    if guide == "colour":
        _util_chk(lib.af_guided_apply_colour(res.ordinal, res.ptr(f), H, W, *tail) if bits is None else lib.af_guided_apply_colour16(res.ordinal, res.ptr(f), H, W, bits, *tail))
    else:
        _util_chk(lib.af_guided_apply(res.ordinal, res.ptr(f), H, W, *tail) if bits is None else lib.af_guided_apply16(res.ordinal, res.ptr(f), H, W, bits, *tail))
    return out


def _transfer(what, res, full, proxy_in, proxy_out, radius, eps, guide="channel"):
    radius, eps = check_guided(radius, eps, what, guide)
    res = _on(what, res, [full, proxy_in, proxy_out])
    h, w = _check_pair(proxy_in, proxy_out, what, res)
    _check_full(full, h, w, what, res)
    a, b = _coeffs(what, res, proxy_in, proxy_out, radius, eps, guide)
    return _apply(what, res, full, a, b, guide=guide)


def guided_coeffs(proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """The smoothed coefficient planes (abar, bbar), each (h, w, 3) float32, of numpy images through host pointers (the library stages the
    call on GPU `device`)."""
    return _coeffs("guided_coeffs", Host(device), proxy_in, proxy_out, radius, eps)


def guided_transfer(full, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """full (H, W, 3) uint8 with the correction proxy_in -> proxy_out (both (h, w, 3) uint8, h <= H, w <= W) carried to it: (H, W, 3) uint8.
    numpy arrays through host pointers."""
    return _transfer("guided_transfer", Host(device), full, proxy_in, proxy_out, radius, eps)


def guided_apply(full, a, b, device=0):
    """af_guided_apply with planes of the caller's: full (H, W, 3) uint8, a and b (h, w, 3) float32 with h <= H, w <= W, sampled bilinearly at
    the full-size pixel centres; out = clamp(rint(F + (a F + b)), 0, 255), (H, W, 3) uint8.  numpy arrays through host pointers."""
    return _apply("guided_apply", Host(device), full, a, b)


def guided_coeffs_device(proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guided_coeffs on CUDA tensors (device pointers, no host copy): two (h, w, 3) float32 tensors on the images' device."""
    return _coeffs("guided_coeffs_device", None, proxy_in, proxy_out, radius, eps)


def guided_transfer_device(full, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guided_transfer on CUDA tensors: an (H, W, 3) uint8 tensor on the images' device; nothing leaves it."""
    return _transfer("guided_transfer_device", None, full, proxy_in, proxy_out, radius, eps)


def guided_apply_device(full, a, b):
    """guided_apply on CUDA tensors: an (H, W, 3) uint8 tensor on the images' device."""
    return _apply("guided_apply_device", None, full, a, b)


# ---- the colour guide: every output channel fitted on all three guide channels ------------------------------------
def guided_coeffs_colour(proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """af_guided_coeffs_colour: the smoothed planes (A, b) of numpy images through host pointers, A (h, w, 9) float32 with entry 3k + c (the
    weight of guide channel c in output channel k) and b (h, w, 3); eps at least 2^-20."""
    return _coeffs("guided_coeffs_colour", Host(device), proxy_in, proxy_out, radius, eps, "colour")


def guided_coeffs_colour_device(proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guided_coeffs_colour on CUDA tensors: (h, w, 9) and (h, w, 3) float32 tensors on the images' device."""
    return _coeffs("guided_coeffs_colour_device", None, proxy_in, proxy_out, radius, eps, "colour")


def guided_transfer_colour(full, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """guided_transfer with the colour guide: guided_coeffs_colour, then guided_apply_colour.  numpy arrays through host pointers."""
    return _transfer("guided_transfer_colour", Host(device), full, proxy_in, proxy_out, radius, eps, "colour")


def guided_transfer_colour_device(full, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guided_transfer_colour on CUDA tensors: an (H, W, 3) uint8 tensor on the images' device; nothing leaves it."""
    return _transfer("guided_transfer_colour_device", None, full, proxy_in, proxy_out, radius, eps, "colour")


def guided_apply_colour(full, A, b, device=0):
    """af_guided_apply_colour with planes of the caller's: full (H, W, 3) uint8, A (h, w, 9) and b (h, w, 3) float32 with h <= H, w <= W;
    out_k = clamp(rint(F_k + (((A_k0 F_0 + A_k1 F_1) + A_k2 F_2) + b_k)), 0, 255), (H, W, 3) uint8.  numpy arrays through host pointers."""
    return _apply("guided_apply_colour", Host(device), full, A, b, guide="colour")


def guided_apply_colour_device(full, A, b):
    """guided_apply_colour on CUDA tensors: an (H, W, 3) uint8 tensor on the images' device."""
    return _apply("guided_apply_colour_device", None, full, A, b, guide="colour")


# ---- more than 8 bits per sample -------------------------------------------------------------------------------
# The transfer was written for reduced resolution and serves reduced bit depth alike: the pipeline sees the 8-bit reduction of a deep
# frame, and the correction it made there is carried to the deep frame as the same smooth field, out = F + (a F + b M / 255) with
# M = 2^bits - 1.  Every bit below the eighth is the input's own, and a field that is smooth by construction cannot band.
def _reduce_depth(what, res, samples, bits):
    from .atlasfit import load_library, _util_chk
    bits = check_bits(bits, what)
    res = _on(what, res, [samples])
    src = res.array(samples)
    if not res.typed(src, "uint16") or math.prod(src.shape) < 1:
        raise ValueError("%s: expected a non-empty uint16 %s, got %s %s" % (what, "CUDA tensor" if res.on_device else "array", tuple(src.shape), src.dtype))
    src = res.contiguous(src)
    out = res.empty(tuple(src.shape), "uint8")
    res.sync()
    _util_chk(load_library().af_depth_reduce(res.ordinal, res.ptr(src), math.prod(src.shape), bits, res.ptr(out), res.on_device))
    return out


def _depth_transfer(what, res, full16, bits, proxy_in, proxy_out, radius, eps, guide="channel"):
    bits = check_bits(bits, what)
    radius, eps = check_guided(radius, eps, what, guide)
    res = _on(what, res, [full16, proxy_in, proxy_out])
    h, w = _check_pair(proxy_in, proxy_out, what, res)
    _check_full(full16, h, w, what, res, "uint16")
    a, b = _coeffs(what, res, proxy_in, proxy_out, radius, eps, guide)
    return _apply(what, res, full16, a, b, "uint16", bits, guide)


def reduce_depth(samples, bits, device=0):
    """uint16 samples of `bits` (8..16) bits -> uint8 of the same shape, round(255 v / M) with M = 2^bits - 1 (af_depth_reduce: no tie
    exists); a sample above M reads as M.  A numpy array through host pointers."""
    return _reduce_depth("reduce_depth", Host(device), samples, bits)


def reduce_depth_device(samples, bits):
    """reduce_depth on a torch.uint16 CUDA tensor: a uint8 tensor of the same shape on its device."""
    return _reduce_depth("reduce_depth_device", None, samples, bits)


def guided_apply16(full16, bits, a, b, device=0):
    """af_guided_apply16: full16 (H, W, 3) uint16 of `bits` bits, a and b (h, w, 3) float32 planes of an 8-bit pair;
    out = clamp(rint(F + (a F + b M / 255)), 0, M), (H, W, 3) uint16.  numpy arrays through host pointers."""
    return _apply("guided_apply16", Host(device), full16, a, b, "uint16", bits)


def guided_apply16_device(full16, bits, a, b):
    """guided_apply16 on CUDA tensors: an (H, W, 3) torch.uint16 tensor on the images' device."""
    return _apply("guided_apply16_device", None, full16, a, b, "uint16", bits)


def guided_apply_colour16(full16, bits, A, b, device=0):
    """af_guided_apply_colour16: guided_apply_colour on a (H, W, 3) uint16 frame of `bits` bits with the planes of an 8-bit pair, b scaled
    by M / 255 and the result clamped to M; (H, W, 3) uint16.  numpy arrays through host pointers."""
    return _apply("guided_apply_colour16", Host(device), full16, A, b, "uint16", bits, "colour")


def guided_apply_colour16_device(full16, bits, A, b):
    """guided_apply_colour16 on CUDA tensors: an (H, W, 3) torch.uint16 tensor on the images' device."""
    return _apply("guided_apply_colour16_device", None, full16, A, b, "uint16", bits, "colour")


def depth_transfer(full16, bits, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """full16 (H, W, 3) uint16 of `bits` bits with the correction proxy_in -> proxy_out of an 8-bit pair (both (h, w, 3) uint8, h <= H,
    w <= W; the pair of the frame's own size is the common case) carried to it: guided_coeffs, then guided_apply16.  numpy arrays."""
    return _depth_transfer("depth_transfer", Host(device), full16, bits, proxy_in, proxy_out, radius, eps)


def depth_transfer_device(full16, bits, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """depth_transfer on CUDA tensors (full16 torch.uint16, the pair torch.uint8): nothing leaves the device."""
    return _depth_transfer("depth_transfer_device", None, full16, bits, proxy_in, proxy_out, radius, eps)


def depth_transfer_colour(full16, bits, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """depth_transfer with the colour guide: guided_coeffs_colour of the 8-bit pair, then guided_apply_colour16.  numpy arrays."""
    return _depth_transfer("depth_transfer_colour", Host(device), full16, bits, proxy_in, proxy_out, radius, eps, "colour")


def depth_transfer_colour_device(full16, bits, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """depth_transfer_colour on CUDA tensors (full16 torch.uint16, the pair torch.uint8): nothing leaves the device."""
    return _depth_transfer("depth_transfer_colour_device", None, full16, bits, proxy_in, proxy_out, radius, eps, "colour")
