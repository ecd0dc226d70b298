"""Residual guided transfer: a correction computed on a proxy-size copy of a frame, carried to the full-size frame.

Flicker is a low-frequency colour error, so the pipeline may run on a shrunk copy of the clip (`Deflicker(proxy_long_edge=N)`) and hand
its result up.  For one frame: F is the full-size frame, I its area shrink (the proxy input) and P the pipeline's final frame at the proxy
size.  Per channel the fast guided filter (He & Sun) of the residual d = P - I with guide I gives a gain a and an offset b per proxy
pixel, d ~ a I + b over a (2r + 1)^2 window, regularised by eps (in squared 8-bit levels); their box means are sampled bilinearly at the
full-size pixel centres and out = clamp(rint(F + (a F + b)), 0, 255).  Every detail above the proxy's resolution is the input frame's own.

P == I returns F byte for byte; P == I + c with nothing clipped returns F + c.  The kernels (csrc/guided.hip, af_guided_coeffs and
af_guided_apply) compute every value in one fixed order of correctly rounded operations, so the result is the same everywhere and equal
to a numpy restatement.

DEFAULT_RADIUS and DEFAULT_EPS are policy: nobody has measured them on footage."""
import ctypes as C

import numpy as np

from .y4m import check_bits

DEFAULT_RADIUS = 8       # window radius in proxy pixels (1..32)
DEFAULT_EPS = 64.0       # squared 8-bit levels: a window whose guide varies by less than ~8 levels gets an offset, hardly a gain
MAX_RADIUS = 32


def check_guided(radius, eps, what="guided transfer"):
    """(radius, eps) as (int, float), or ValueError: radius an integer in 1..32, eps finite and > 0 (as the fp32 the library receives)."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in 1..%d, got %r" % (what, MAX_RADIUS, radius))
    try:
        e = float(np.float32(eps))
    except (TypeError, ValueError):
        raise ValueError("%s: eps must be a number, got %r" % (what, eps))
    if not np.isfinite(e) or e <= 0:
        raise ValueError("%s: eps must be finite and > 0 (in fp32), got %r" % (what, eps))
    return int(radius), e


def _check_image(x, name, what, torch_side):
    dt = "torch.uint8" if torch_side else "uint8"
    if not hasattr(x, "shape") or len(x.shape) != 3 or x.shape[2] != 3 or str(x.dtype) != dt:
        raise ValueError("%s: %s must be (H, W, 3) uint8, got %s %s" % (what, name, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x).__name__)))
    return int(x.shape[0]), int(x.shape[1])


def _check_pair(proxy_in, proxy_out, what, torch_side):
    h, w = _check_image(proxy_in, "proxy_in", what, torch_side)
    if _check_image(proxy_out, "proxy_out", what, torch_side) != (h, w):
        raise ValueError("%s: proxy_in is %dx%d, proxy_out %dx%d" % (what, w, h, proxy_out.shape[1], proxy_out.shape[0]))
    return h, w


def _check_full(full, h, w, what, torch_side):
    H, W = _check_image(full, "full", what, torch_side)
    if h > H or w > W:
        raise ValueError("%s: the proxy (%dx%d) is larger than the full frame (%dx%d)" % (what, w, h, W, H))
    return H, W


def guided_coeffs(proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """The smoothed coefficient planes (abar, bbar), each (h, w, 3) float32, of numpy images through host pointers (the library stages the
    call on GPU `device`)."""
    from .atlasfit import load_library, _util_chk, _ptr
    radius, eps = check_guided(radius, eps, "guided_coeffs")
    h, w = _check_pair(proxy_in, proxy_out, "guided_coeffs", False)
    i, p = np.ascontiguousarray(proxy_in), np.ascontiguousarray(proxy_out)
    a, b = np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.float32)
    _util_chk(load_library().af_guided_coeffs(int(device), _ptr(i), _ptr(p), h, w, radius, eps, _ptr(a), _ptr(b), None, 0))
    return a, b


def guided_transfer(full, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """full (H, W, 3) uint8 with the correction proxy_in -> proxy_out (both (h, w, 3) uint8, h <= H, w <= W) carried to it: (H, W, 3) uint8.
    numpy arrays through host pointers."""
    from .atlasfit import load_library, _util_chk, _ptr
    radius, eps = check_guided(radius, eps, "guided_transfer")
    h, w = _check_pair(proxy_in, proxy_out, "guided_transfer", False)
    H, W = _check_full(full, h, w, "guided_transfer", False)
    a, b = guided_coeffs(proxy_in, proxy_out, radius, eps, device)
    f = np.ascontiguousarray(full)
    out = np.empty((H, W, 3), np.uint8)
    _util_chk(load_library().af_guided_apply(int(device), _ptr(f), H, W, _ptr(a), _ptr(b), h, w, _ptr(out), 0))
    return out


def _check_planes(a, b, what, torch_side):
    dt = "torch.float32" if torch_side else "float32"
    for name, x in (("a", a), ("b", b)):
        if not hasattr(x, "shape") or len(x.shape) != 3 or x.shape[2] != 3 or str(x.dtype) != dt:
            raise ValueError("%s: %s must be (h, w, 3) float32, got %s %s" % (what, name, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x).__name__)))
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("%s: a is %dx%d, b %dx%d" % (what, a.shape[1], a.shape[0], b.shape[1], b.shape[0]))
    return int(a.shape[0]), int(a.shape[1])


def guided_apply(full, a, b, device=0):
    """af_guided_apply with planes of the caller's: full (H, W, 3) uint8, a and b (h, w, 3) float32 with h <= H, w <= W, sampled bilinearly at
    the full-size pixel centres; out = clamp(rint(F + (a F + b)), 0, 255), (H, W, 3) uint8.  numpy arrays through host pointers."""
    from .atlasfit import load_library, _util_chk, _ptr
    h, w = _check_planes(a, b, "guided_apply", False)
    H, W = _check_full(full, h, w, "guided_apply", False)
    f, pa, pb = np.ascontiguousarray(full), np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.empty((H, W, 3), np.uint8)
    _util_chk(load_library().af_guided_apply(int(device), _ptr(f), H, W, _ptr(pa), _ptr(pb), h, w, _ptr(out), 0))
    return out


def _device_of(tensors, what):
    dev = tensors[0].device if hasattr(tensors[0], "is_cuda") else None
    for t in tensors:
        if not hasattr(t, "is_cuda") or not t.is_cuda or t.device != dev:
            raise ValueError("%s: the images must be CUDA tensors on one device (host arrays go through the function without _device)" % what)
    return dev


def guided_coeffs_device(proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guided_coeffs on CUDA tensors (device pointers, no host copy): two (h, w, 3) float32 tensors on the images' device."""
    import torch
    from .atlasfit import load_library, _util_chk
    radius, eps = check_guided(radius, eps, "guided_coeffs_device")
    dev = _device_of([proxy_in, proxy_out], "guided_coeffs_device")
    h, w = _check_pair(proxy_in, proxy_out, "guided_coeffs_device", True)
    i, p = proxy_in.contiguous(), proxy_out.contiguous()
    a, b = torch.empty((h, w, 3), device=dev), torch.empty((h, w, 3), device=dev)
    work = torch.empty((2, h, w, 3), device=dev)            # the unsmoothed planes, from torch's allocator: no hipMalloc per frame
    torch.cuda.synchronize(dev)                              # the tensors' producers ran on torch's streams, the library on the default one
    q = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    _util_chk(load_library().af_guided_coeffs(dev.index, q(i), q(p), h, w, radius, eps, q(a), q(b), q(work), 1))
    return a, b


def guided_transfer_device(full, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """guided_transfer on CUDA tensors: an (H, W, 3) uint8 tensor on the images' device; nothing leaves it."""
    import torch
    from .atlasfit import load_library, _util_chk
    radius, eps = check_guided(radius, eps, "guided_transfer_device")
    dev = _device_of([full, proxy_in, proxy_out], "guided_transfer_device")
    h, w = _check_pair(proxy_in, proxy_out, "guided_transfer_device", True)
    H, W = _check_full(full, h, w, "guided_transfer_device", True)
    a, b = guided_coeffs_device(proxy_in, proxy_out, radius, eps)
    f = full.contiguous()
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    q = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    _util_chk(load_library().af_guided_apply(dev.index, q(f), H, W, q(a), q(b), h, w, q(out), 1))
    return out


def guided_apply_device(full, a, b):
    """guided_apply on CUDA tensors: an (H, W, 3) uint8 tensor on the images' device."""
    import torch
    from .atlasfit import load_library, _util_chk
    dev = _device_of([full, a, b], "guided_apply_device")
    h, w = _check_planes(a, b, "guided_apply_device", True)
    H, W = _check_full(full, h, w, "guided_apply_device", True)
    f, pa, pb = full.contiguous(), a.contiguous(), b.contiguous()
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    q = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    _util_chk(load_library().af_guided_apply(dev.index, q(f), H, W, q(pa), q(pb), h, w, q(out), 1))
    return out


# ---- more than 8 bits per sample -------------------------------------------------------------------------------
# The transfer was written for reduced resolution and serves reduced bit depth alike: the pipeline sees the 8-bit reduction of a deep
# frame, and the correction it made there is carried to the deep frame as the same smooth field, out = F + (a F + b M / 255) with
# M = 2^bits - 1.  Every bit below the eighth is the input's own, and a field that is smooth by construction cannot band.
def _check_image16(x, name, what, torch_side):
    dt = "torch.uint16" if torch_side else "uint16"
    if not hasattr(x, "shape") or len(x.shape) != 3 or x.shape[2] != 3 or str(x.dtype) != dt:
        raise ValueError("%s: %s must be (H, W, 3) uint16, got %s %s" % (what, name, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x).__name__)))
    return int(x.shape[0]), int(x.shape[1])


def _check_full16(full, h, w, what, torch_side):
    H, W = _check_image16(full, "full", what, torch_side)
    if h > H or w > W:
        raise ValueError("%s: the proxy (%dx%d) is larger than the full frame (%dx%d)" % (what, w, h, W, H))
    return H, W


def reduce_depth(samples, bits, device=0):
    """uint16 samples of `bits` (8..16) bits -> uint8 of the same shape, round(255 v / M) with M = 2^bits - 1 (af_depth_reduce: no tie
    exists); a sample above M reads as M.  A numpy array through host pointers."""
    from .atlasfit import load_library, _util_chk, _ptr
    bits = check_bits(bits, "reduce_depth")
    src = np.asarray(samples)
    if src.dtype != np.uint16 or src.size < 1:
        raise ValueError("reduce_depth: expected a non-empty uint16 array, got %s %s" % (src.shape, src.dtype))
    src = np.ascontiguousarray(src)
    out = np.empty(src.shape, np.uint8)
    _util_chk(load_library().af_depth_reduce(int(device), _ptr(src), src.size, bits, _ptr(out), 0))
    return out


def reduce_depth_device(samples, bits):
    """reduce_depth on a torch.uint16 CUDA tensor: a uint8 tensor of the same shape on its device."""
    import torch
    from .atlasfit import load_library, _util_chk
    bits = check_bits(bits, "reduce_depth_device")
    dev = _device_of([samples], "reduce_depth_device")
    if samples.dtype != torch.uint16 or samples.numel() < 1:
        raise ValueError("reduce_depth_device: expected a non-empty uint16 CUDA tensor, got %s %s" % (tuple(samples.shape), samples.dtype))
    src = samples.contiguous()
    out = torch.empty(tuple(src.shape), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    _util_chk(load_library().af_depth_reduce(dev.index, C.c_void_p(src.data_ptr()), src.numel(), bits, C.c_void_p(out.data_ptr()), 1))
    return out


def guided_apply16(full16, bits, a, b, device=0):
    """af_guided_apply16: full16 (H, W, 3) uint16 of `bits` bits, a and b (h, w, 3) float32 planes of an 8-bit pair;
    out = clamp(rint(F + (a F + b M / 255)), 0, M), (H, W, 3) uint16.  numpy arrays through host pointers."""
    from .atlasfit import load_library, _util_chk, _ptr
    bits = check_bits(bits, "guided_apply16")
    h, w = _check_planes(a, b, "guided_apply16", False)
    H, W = _check_full16(full16, h, w, "guided_apply16", False)
    f, pa, pb = np.ascontiguousarray(full16), np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.empty((H, W, 3), np.uint16)
    _util_chk(load_library().af_guided_apply16(int(device), _ptr(f), H, W, bits, _ptr(pa), _ptr(pb), h, w, _ptr(out), 0))
    return out


def guided_apply16_device(full16, bits, a, b):
    """guided_apply16 on CUDA tensors: an (H, W, 3) torch.uint16 tensor on the images' device."""
    import torch
    from .atlasfit import load_library, _util_chk
    bits = check_bits(bits, "guided_apply16_device")
    dev = _device_of([full16, a, b], "guided_apply16_device")
    h, w = _check_planes(a, b, "guided_apply16_device", True)
    H, W = _check_full16(full16, h, w, "guided_apply16_device", True)
    f, pa, pb = full16.contiguous(), a.contiguous(), b.contiguous()
    out = torch.empty((H, W, 3), dtype=torch.uint16, device=dev)
    torch.cuda.synchronize(dev)
    q = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    _util_chk(load_library().af_guided_apply16(dev.index, q(f), H, W, bits, q(pa), q(pb), h, w, q(out), 1))
    return out


def depth_transfer(full16, bits, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS, device=0):
    """full16 (H, W, 3) uint16 of `bits` bits with the correction proxy_in -> proxy_out of an 8-bit pair (both (h, w, 3) uint8, h <= H,
    w <= W; the pair of the frame's own size is the common case) carried to it: guided_coeffs, then guided_apply16.  numpy arrays."""
    bits = check_bits(bits, "depth_transfer")
    radius, eps = check_guided(radius, eps, "depth_transfer")
    h, w = _check_pair(proxy_in, proxy_out, "depth_transfer", False)
    _check_full16(full16, h, w, "depth_transfer", False)
    a, b = guided_coeffs(proxy_in, proxy_out, radius, eps, device)
    return guided_apply16(full16, bits, a, b, device)


def depth_transfer_device(full16, bits, proxy_in, proxy_out, radius=DEFAULT_RADIUS, eps=DEFAULT_EPS):
    """depth_transfer on CUDA tensors (full16 torch.uint16, the pair torch.uint8): nothing leaves the device."""
    bits = check_bits(bits, "depth_transfer_device")
    radius, eps = check_guided(radius, eps, "depth_transfer_device")
    _device_of([full16, proxy_in, proxy_out], "depth_transfer_device")
    h, w = _check_pair(proxy_in, proxy_out, "depth_transfer_device", True)
    _check_full16(full16, h, w, "depth_transfer_device", True)
    a, b = guided_coeffs_device(proxy_in, proxy_out, radius, eps)
    return guided_apply16_device(full16, bits, a, b)
