"""ctypes binding of the stage-2 calls of libatlasfit.so (include/atlasfit.h, af_filter_* and af_conv2d): the neural filter UNet and
the local refinement TransformNet of src/neural_filter_and_refinement.py:44-130 on the GPU.

`NeuralFilter(h, w)` holds both nets and the recurrence state of the reference's frame loop (:89-121) for one frame size, in fp32
or, with precision="fp16", in the arithmetic of the reference's modules under fp16 autocast (AF_FILTER_FP16).
There is no CPU fallback: without the library and a GPU every call raises."""
import ctypes as C
import re

import numpy as np

from .atlasfit import AtlasFitError, load_library

NET_FILTER, NET_LOCAL = 0, 1
PRECISIONS = {"fp32": 0, "fp16": 1}      # AF_FILTER_FP32, AF_FILTER_FP16 (include/atlasfit.h)


def precision_code(precision):
    """"fp32" / "fp16" -> the library's code; any other name raises ValueError."""
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (", ".join(sorted(PRECISIONS, reverse=True)), precision))
    return PRECISIONS[precision]

# InstanceNorm2d(track_running_stats=True) buffers of the TransformNet: in its state_dict, never applied (network_local.py:141,
# `self.norm in ["BN" or "IN"]` is `in ["BN"]`), so the loader accepts and ignores exactly these keys
NORM_BUFFER = re.compile(r"^.+\.norm_layer\.(running_mean|running_var|num_batches_tracked)$")

# the activations af_filter_debug_activation names: (pyramid level, channels); level l is (Hp >> l, Wp >> l)
ACTIVATIONS = {
    "input": (0, 6), "enc1": (0, 32), "enc2": (1, 64), "enc3": (2, 128), "enc4": (3, 256), "bottleneck": (4, 512),
    "dec4": (3, 256), "dec3": (2, 128), "dec2": (1, 64), "dec1": (0, 32), "pred": (0, 3),
    "E1a": (0, 32), "E1b": (0, 32), "E2a": (1, 64), "E2b": (1, 64), "E3": (2, 128), "RB": (2, 128), "hidden": (2, 128),
    "D2": (1, 64), "D1": (0, 32), "Y": (0, 3), "final": (0, 3),
}


def filter_keys():
    """[(key, shape)] of UNet(in_channels=6, out_channels=3, init_features=32).state_dict() (network_filter.py:9-57)."""
    keys, c = [], 6
    for i, f in enumerate((32, 64, 128, 256), 1):
        keys += [("encoder%d.enc%dconv1.weight" % (i, i), (f, c, 3, 3)), ("encoder%d.enc%dconv2.weight" % (i, i), (f, f, 3, 3))]
        c = f
    keys += [("bottleneck.bottleneckconv1.weight", (512, 256, 3, 3)), ("bottleneck.bottleneckconv2.weight", (512, 512, 3, 3))]
    for n, f in zip((4, 3, 2, 1), (256, 128, 64, 32)):
        keys += [("upconv%d.1.weight" % n, (f, 2 * f, 3, 3)), ("upconv%d.1.bias" % n, (f,)),
                 ("decoder%d.dec%dconv1.weight" % (n, n), (f, 2 * f, 3, 3)), ("decoder%d.dec%dconv2.weight" % (n, n), (f, f, 3, 3))]
    keys += [("conv.weight", (3, 32, 1, 1)), ("conv.bias", (3,))]
    return keys


def local_keys():
    """[(key, shape)] of TransformNet(nf=32, norm='IN', blocks=5, nc_in=12, nc_out=3).state_dict() without the norm buffers
    (network_local.py:60-86)."""
    keys = []

    def conv(name, o, i, k):
        keys.extend([(name + ".weight", (o, i, k, k)), (name + ".bias", (o,))])
    conv("conv1a.conv2d", 32, 6, 7)
    conv("conv1b.conv2d", 32, 6, 7)
    conv("conv2a.conv2d", 64, 32, 3)
    conv("conv2b.conv2d", 64, 32, 3)
    conv("conv3.conv2d", 128, 128, 3)
    for b in range(5):
        conv("ResBlocks.%d.conv1.conv2d" % b, 128, 128, 3)
        conv("ResBlocks.%d.conv2.conv2d" % b, 128, 128, 3)
    conv("convlstm.Gates", 512, 256, 3)
    conv("deconv1.conv2d", 64, 128, 3)
    conv("deconv2.conv2d", 32, 128, 3)
    conv("deconv3.conv2d", 3, 64, 7)
    return keys


class StateDictError(ValueError):
    """A checkpoint that does not match the net: names the offending key."""


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def flatten_state_dict(sd, net):
    """state_dict -> flat fp32 in state_dict order, strict: a missing key, an unexpected key or a wrong shape raises
    StateDictError naming it.  The TransformNet's InstanceNorm buffers (NORM_BUFFER) are the only keys accepted and dropped."""
    expect = filter_keys() if net == NET_FILTER else local_keys()
    names = {k for k, _ in expect}
    label = "neural filter" if net == NET_FILTER else "local refinement"
    for k in sd.keys():
        if k not in names and not (net == NET_LOCAL and NORM_BUFFER.match(k)):
            raise StateDictError("%s state_dict: unexpected key %r" % (label, k))
    parts = []
    for k, shape in expect:
        if k not in sd:
            raise StateDictError("%s state_dict: missing key %r" % (label, k))
        a = _np(sd[k])
        if tuple(a.shape) != shape:
            raise StateDictError("%s state_dict: %r has shape %s, expected %s" % (label, k, tuple(a.shape), shape))
        parts.append(np.asarray(a, np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts))


def padded_size(h, w):
    """InputPadder (src/models/utils.py:600-612): every side to the next multiple of 32 -> (Hp, Wp, left)."""
    ph = (((h // 32) + 1) * 32 - h) % 32
    pw = (((w // 32) + 1) * 32 - w) % 32
    return h + ph, w + pw, pw // 2


_SIGS_SET = False


def _lib():
    global _SIGS_SET
    lib = load_library()
    if not _SIGS_SET:
        vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
        for name, res, args in (
                ("af_filter_create", i32, [i32, i32, i32, C.POINTER(vp)]),
                ("af_filter_destroy", None, [vp]),
                ("af_filter_param_count", sz, [vp, i32]),
                ("af_filter_set_params", i32, [vp, i32, vp, sz]),
                ("af_filter_reset", i32, [vp]),
                ("af_filter_frame", i32, [vp, vp, vp, vp, vp, i32]),
                ("af_filter_debug_activation", i32, [vp, C.c_char_p, vp, sz]),
                ("af_conv2d", i32, [i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32]),
                ("af_filter_set_precision", i32, [vp, i32]),
                ("af_filter_get_precision", i32, [vp, C.POINTER(i32)]),
                ("af_conv2d_prec", i32, [i32, i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32])):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        _SIGS_SET = True
    return lib


def _chk(rc):
    if rc != 0:
        raise AtlasFitError(rc, _lib().af_last_error(None).decode())


def _is_cuda(a):
    return hasattr(a, "is_cuda") and a.is_cuda


def conv2d(x, weight, bias=None, stride=1, pad_mode=0, act=0, residual=None, device=0, precision="fp32"):
    """One convolution as the stage-2 nets run it (af_conv2d; af_conv2d_prec for precision="fp16"): x (h, w, cin) HWC, weight
    (cout, cin, k, k) OIHW, padding k // 2 (pad_mode 0 zeros, 1 reflection), act 0 none / 1 ReLU / 2 LeakyReLU(0.2) / 3 tanh, residual
    (ho, wo, cout) added last.  numpy arrays in -> numpy out; CUDA tensors in -> CUDA tensor out."""
    prec = precision_code(precision)
    lib = _lib()
    call = lib.af_conv2d if prec == 0 else (lambda *a: lib.af_conv2d_prec(prec, *a))
    h, w, cin = x.shape
    cout, cin_w, k, _ = weight.shape
    if cin_w != cin:
        raise ValueError("conv2d: weight has %d input channels, x %d" % (cin_w, cin))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if _is_cuda(x):
        import torch
        ts = [None if t is None else t.contiguous().float() for t in (x, weight, bias, residual)]
        y = torch.empty((ho, wo, cout), device=x.device)
        torch.cuda.synchronize(x.device)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
        _chk(call(int(x.device.index or 0), p(ts[0]), h, w, cin, p(ts[1]), p(ts[2]), cout, k, stride, pad_mode, act, p(ts[3]), p(y), 1))
        return y
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (x, weight, bias, residual)]
    y = np.empty((ho, wo, cout), np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    _chk(call(int(device), p(arrs[0]), h, w, cin, p(arrs[1]), p(arrs[2]), cout, k, stride, pad_mode, act, p(arrs[3]), p(y), 0))
    return y


class NeuralFilter:
    """Stage 2 of the pipeline for frames of (h, w): UNet(cat(content, style)) -> pred, then the TransformNet refinement of the
    frame loop -> final (src/neural_filter_and_refinement.py:89-121), both at the padded size (Hp, Wp)."""

    def __init__(self, h, w, device=0, precision="fp32"):
        precision_code(precision)
        self.lib = _lib()
        self.h, self.w, self.device = int(h), int(w), int(device)
        self.Hp, self.Wp, self.left = padded_size(self.h, self.w)
        self.f = C.c_void_p()
        _chk(self.lib.af_filter_create(self.device, self.h, self.w, C.byref(self.f)))
        self.precision = "fp32"
        if precision != "fp32":
            self.set_precision(precision)

    def set_precision(self, precision):
        """"fp32" (the default) or "fp16" (module docstring), at any time; the next frame is treated as frame 0."""
        _chk(self.lib.af_filter_set_precision(self.f, precision_code(precision)))
        self.precision = precision

    def load_state_dicts(self, filter_sd, local_sd):
        """Both checkpoints as torch.load returns them (plain state_dicts)."""
        for net, sd in ((NET_FILTER, filter_sd), (NET_LOCAL, local_sd)):
            flat = flatten_state_dict(sd, net)
            n = self.lib.af_filter_param_count(self.f, net)
            if n != flat.size:
                raise AtlasFitError(-1, "net %d: %d parameters, the library expects %d" % (net, flat.size, n))
            _chk(self.lib.af_filter_set_params(self.f, net, flat.ctypes.data_as(C.c_void_p), flat.size))

    def reset(self):
        """The next frame is treated as frame 0 (final = pred)."""
        _chk(self.lib.af_filter_reset(self.f))

    def frame(self, content, style):
        """content, style: (h, w, 3) float in [0, 1] (numpy, or CUDA tensors on this device).  Returns (pred, final), (Hp, Wp, 3)
        fp32 unclamped, of the inputs' kind."""
        shape = (self.h, self.w, 3)
        if tuple(content.shape) != shape or tuple(style.shape) != shape:
            raise ValueError("frame: content and style must be %s, got %s and %s" % (shape, tuple(content.shape), tuple(style.shape)))
        if _is_cuda(content):
            import torch
            c, s = content.contiguous().float(), style.contiguous().float().to(content.device)
            pred = torch.empty((self.Hp, self.Wp, 3), device=content.device)
            final = torch.empty_like(pred)
            torch.cuda.synchronize(content.device)
            _chk(self.lib.af_filter_frame(self.f, C.c_void_p(c.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(pred.data_ptr()),
                                          C.c_void_p(final.data_ptr()), 1))
            return pred, final
        c = np.ascontiguousarray(content, np.float32)
        s = np.ascontiguousarray(style, np.float32)
        pred = np.empty((self.Hp, self.Wp, 3), np.float32)
        final = np.empty_like(pred)
        _chk(self.lib.af_filter_frame(self.f, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), pred.ctypes.data_as(C.c_void_p),
                                      final.ctypes.data_as(C.c_void_p), 0))
        return pred, final

    def activation(self, name):
        """A named intermediate of the last frame (ACTIVATIONS), HWC fp32 numpy."""
        if name not in ACTIVATIONS:
            raise KeyError("unknown activation %r (known: %s)" % (name, ", ".join(ACTIVATIONS)))
        lvl, ch = ACTIVATIONS[name]
        out = np.empty((self.Hp >> lvl, self.Wp >> lvl, ch), np.float32)
        _chk(self.lib.af_filter_debug_activation(self.f, name.encode(), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def close(self):
        if self.f:
            self.lib.af_filter_destroy(self.f)
            self.f = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
