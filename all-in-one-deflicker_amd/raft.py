"""ctypes binding of the optical-flow calls of libatlasfit.so (include/atlasfit.h, af_raft_*): the forward pass of RAFT ("basic",
small=False; src/models/stage_1/core/raft.py) as src/models/stage_1/raft_wrapper.py drives it — InputPadder 'sintel', 20 iterations,
test mode, no unpad — in fp32 on the GPU, or with precision="fp16" in the arithmetic the reference itself runs on a GPU (both encoders
and the update block under fp16 autocast; the correlation, the lookup, the coordinates and the upsampling stay fp32).

`RAFT(h, w)` holds the weights, the encoded frames (each frame goes through fnet and cnet once, whatever number of pairs it is
part of) and the buffers of `capacity` pair-directions that run as one batch.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from .atlasfit import AtlasFitError, load_library
from .stage2 import StateDictError, _np, _is_cuda

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 3, 4
PRECISIONS = {"fp32": 0, "fp16": 1}      # AF_RAFT_FP32, AF_RAFT_FP16 (include/atlasfit.h)


def precision_code(precision):
    """"fp32" | "fp16" -> the ABI's value; any other name is a ValueError naming the choices."""
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (", ".join(sorted(PRECISIONS, reverse=True)), precision))
    return PRECISIONS[precision]

# the intermediates af_raft_debug_activation names: channels per 1/8-grid position (corr_vol<l>: the grid positions of level l)
ACTIVATIONS = {"fmap1": 256, "fmap2": 256, "net0": 128, "inp": 128, "corr_l0": 81, "corr_l1": 81, "corr_l2": 81, "corr_l3": 81,
               "motion": 128, "net": 128, "delta": 2, "flow_lo": 2, "mask": 576}

_BLOCKS = (("layer1.0", 64, 1), ("layer1.1", 64, 1), ("layer2.0", 96, 2), ("layer2.1", 96, 1), ("layer3.0", 128, 2), ("layer3.1", 128, 1))


def raft_keys():
    """[(key, shape)] of RAFT(small=False).state_dict() in its own order (core/raft.py, extractor.py, update.py).  fnet's
    InstanceNorm2d has no entries; cnet's BatchNorm2d has five each, and the norm3 of a strided block appears a second time as
    downsample.1 (the same module registered twice)."""
    keys = []

    def conv(name, o, i, kh, kw):
        keys.extend([(name + ".weight", (o, i, kh, kw)), (name + ".bias", (o,))])

    def bn(name, c):
        keys.extend([(name + ".weight", (c,)), (name + ".bias", (c,)), (name + ".running_mean", (c,)), (name + ".running_var", (c,)),
                     (name + ".num_batches_tracked", ())])
    for net, has_bn in (("fnet", False), ("cnet", True)):
        if has_bn:
            bn(net + ".norm1", 64)
        conv(net + ".conv1", 64, 3, 7, 7)
        cin = 64
        for blk, c, s in _BLOCKS:
            p = "%s.%s." % (net, blk)
            conv(p + "conv1", c, cin, 3, 3)
            conv(p + "conv2", c, c, 3, 3)
            if has_bn:
                bn(p + "norm1", c)
                bn(p + "norm2", c)
                if s != 1:
                    bn(p + "norm3", c)
            if s != 1:
                conv(p + "downsample.0", c, cin, 1, 1)
                if has_bn:
                    bn(p + "downsample.1", c)
            cin = c
        conv(net + ".conv2", 256, 128, 1, 1)
    u = "update_block."
    conv(u + "encoder.convc1", 256, 324, 1, 1)
    conv(u + "encoder.convc2", 192, 256, 3, 3)
    conv(u + "encoder.convf1", 128, 2, 7, 7)
    conv(u + "encoder.convf2", 64, 128, 3, 3)
    conv(u + "encoder.conv", 126, 256, 3, 3)
    for n, kh, kw in (("1", 1, 5), ("2", 5, 1)):
        for g in "zrq":
            conv(u + "gru.conv%s%s" % (g, n), 128, 384, kh, kw)
    conv(u + "flow_head.conv1", 256, 128, 3, 3)
    conv(u + "flow_head.conv2", 2, 256, 3, 3)
    conv(u + "mask.0", 256, 128, 3, 3)
    conv(u + "mask.2", 576, 256, 1, 1)
    return keys


def flatten_state_dict(sd):
    """state_dict -> flat fp32 in state_dict order without the num_batches_tracked entries.  Accepts the published checkpoint layout
    (every key prefixed with DataParallel's `module.`) or the bare one; a missing key, an unexpected key or a wrong shape raises
    StateDictError naming it."""
    if len(sd) and all(k.startswith("module.") for k in sd.keys()):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    expect = raft_keys()
    names = {k for k, _ in expect}
    for k in sd.keys():
        if k not in names:
            raise StateDictError("RAFT state_dict: unexpected key %r" % (k,))
    parts = []
    for k, shape in expect:
        if k not in sd:
            raise StateDictError("RAFT state_dict: missing key %r" % (k,))
        a = _np(sd[k])
        if tuple(a.shape) != shape:
            raise StateDictError("RAFT state_dict: %r has shape %s, expected %s" % (k, tuple(a.shape), shape))
        if not k.endswith("num_batches_tracked"):
            parts.append(np.asarray(a, np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts))


def padded_size(h, w):
    """InputPadder mode 'sintel' (core/utils/utils.py): -> (Hp, Wp, top, left)."""
    ph = (((h // 8) + 1) * 8 - h) % 8
    pw = (((w // 8) + 1) * 8 - w) % 8
    return h + ph, w + pw, ph // 2, pw // 2


_SIGS_SET = False


def _lib():
    global _SIGS_SET
    lib = load_library()
    if not _SIGS_SET:
        vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
        ip = C.POINTER(i32)
        for name, res, args in (
                ("af_raft_create", i32, [i32, i32, i32, i32, C.POINTER(vp)]),
                ("af_raft_destroy", None, [vp]),
                ("af_raft_param_count", sz, [vp]),
                ("af_raft_info", i32, [vp, ip, ip, ip]),
                ("af_raft_set_params", i32, [vp, vp, sz]),
                ("af_raft_encode", i32, [vp, i32, vp, i32]),
                ("af_raft_flow", i32, [vp, i32, ip, ip, i32, vp, vp, i32]),
                ("af_raft_step", i32, [vp, i32, i32, vp, vp, vp, vp]),
                ("af_raft_lookup", i32, [vp, i32, i32, vp, vp]),
                ("af_raft_debug_activation", i32, [vp, C.c_char_p, vp, sz]),
                ("af_raft_conv2d", i32, [i32, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp]),
                ("af_raft_gru", i32, [i32, i32, i32, i32, i32] + [vp] * 9),
                ("af_raft_instance_norm", i32, [i32, vp, i32, i32, i32, i32, vp, vp]),
                ("af_raft_set_precision", i32, [vp, i32]),
                ("af_raft_get_precision", i32, [vp, ip]),
                ("af_raft_conv2d_prec", i32, [i32, i32, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp]),
                ("af_raft_gru_prec", i32, [i32, i32, i32, i32, i32, i32] + [vp] * 9),
                ("af_raft_instance_norm_prec", i32, [i32, i32, vp, i32, i32, i32, i32, vp, vp])):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        _SIGS_SET = True
    return lib


def _chk(rc):
    if rc != 0:
        raise AtlasFitError(rc, _lib().af_last_error(None).decode())


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def conv2d(x, weight, bias=None, stride=1, act=ACT_NONE, device=0, precision="fp32"):
    """One convolution as the RAFT path runs it (af_raft_conv2d; af_raft_conv2d_prec for precision="fp16"): x (b, h, w, cin) NHWC numpy,
    weight (cout, cin, kh, kw), zero padding k // 2 per axis -> (b, ho, wo, cout)."""
    prec = precision_code(precision)
    x, weight, bias = _f32(x), _f32(weight), _f32(bias)
    b, h, w, cin = x.shape
    cout, cin_w, kh, kw = weight.shape
    if cin_w != cin:
        raise ValueError("conv2d: weight has %d input channels, x %d" % (cin_w, cin))
    y = np.empty((b, (h - 1) // stride + 1, (w - 1) // stride + 1, cout), np.float32)
    if prec:
        _chk(_lib().af_raft_conv2d_prec(prec, int(device), _p(x), b, h, w, cin, _p(weight), _p(bias), cout, kh, kw, stride, act, _p(y)))
    else:
        _chk(_lib().af_raft_conv2d(int(device), _p(x), b, h, w, cin, _p(weight), _p(bias), cout, kh, kw, stride, act, _p(y)))
    return y


def gru_half(net, x, wz, bz, wr, br, wq, bq, vertical, device=0, precision="fp32"):
    """One half of SepConvGRU (af_raft_gru; af_raft_gru_prec for precision="fp16"): net (b, h, w, 128), x (b, h, w, 256), OIHW weights
    (128, 384, 1, 5) or (128, 384, 5, 1)."""
    prec = precision_code(precision)
    net, x = _f32(net), _f32(x)
    ws = [_f32(a) for a in (wz, bz, wr, br, wq, bq)]
    b, h, w, _ = net.shape
    out = np.empty_like(net)
    if prec:
        _chk(_lib().af_raft_gru_prec(prec, int(device), b, h, w, int(bool(vertical)), _p(net), _p(x), *[_p(a) for a in ws], _p(out)))
    else:
        _chk(_lib().af_raft_gru(int(device), b, h, w, int(bool(vertical)), _p(net), _p(x), *[_p(a) for a in ws], _p(out)))
    return out


def instance_norm(x, relu=False, residual=None, device=0, precision="fp32"):
    """InstanceNorm2d (no affine, eps 1e-5) of x (h, w, c) (+ ReLU, + relu(residual + y)) (af_raft_instance_norm; with precision="fp16"
    af_raft_instance_norm_prec: the result rounded to fp16 once)."""
    prec = precision_code(precision)
    x, residual = _f32(x), _f32(residual)
    h, w, c = x.shape
    y = np.empty_like(x)
    if prec:
        _chk(_lib().af_raft_instance_norm_prec(prec, int(device), _p(x), h, w, c, int(bool(relu)), _p(residual), _p(y)))
    else:
        _chk(_lib().af_raft_instance_norm(int(device), _p(x), h, w, c, int(bool(relu)), _p(residual), _p(y)))
    return y


class RAFT:
    """Optical flow between frames of (h, w) as the reference's RAFTWrapper.compute_flow returns it: (Hp, Wp, 2) fp32 at the padded size."""

    def __init__(self, h, w, capacity=2, device=0, precision="fp32"):
        prec = precision_code(precision)
        self.lib = _lib()
        self.h, self.w, self.device, self.capacity = int(h), int(w), int(device), int(capacity)
        self.Hp, self.Wp, self.top, self.left = padded_size(self.h, self.w)
        self.P = (self.Hp // 8) * (self.Wp // 8)
        self.slots = 2 * self.capacity
        self.r = C.c_void_p()
        _chk(self.lib.af_raft_create(self.device, self.h, self.w, self.capacity, C.byref(self.r)))
        self.precision = "fp32"
        if prec:
            self.set_precision(precision)

    def set_precision(self, precision):
        """"fp32" (the default) or "fp16" (the reference's GPU arithmetic).  Allowed at any time; the encoded frames are dropped: a flow
        call on slots that were not encoded again fails with the library's "no encoded frame" error."""
        _chk(self.lib.af_raft_set_precision(self.r, precision_code(precision)))
        self.precision = precision

    def load_state_dict(self, sd):
        """The checkpoint as torch.load returns it (with or without the `module.` prefix)."""
        flat = flatten_state_dict(sd)
        n = self.lib.af_raft_param_count(self.r)
        if n != flat.size:
            raise AtlasFitError(-1, "RAFT: %d parameters, the library expects %d" % (flat.size, n))
        _chk(self.lib.af_raft_set_params(self.r, _p(flat), flat.size))

    def encode(self, slot, image):
        """image (h, w, 3) with values 0..255 (numpy of any dtype, or a CUDA float tensor on this device) -> frame slot."""
        if tuple(image.shape) != (self.h, self.w, 3):
            raise ValueError("encode: image must be %s, got %s" % ((self.h, self.w, 3), tuple(image.shape)))
        if _is_cuda(image):
            import torch
            t = image.contiguous().float()
            torch.cuda.synchronize(image.device)
            _chk(self.lib.af_raft_encode(self.r, int(slot), C.c_void_p(t.data_ptr()), 1))
        else:
            a = _f32(image)
            _chk(self.lib.af_raft_encode(self.r, int(slot), _p(a), 0))

    def flow_slots(self, pairs, iters=20, want_lo=False, on_device=False):
        """pairs [(slot_a, slot_b)] (at most `capacity`) -> flows (n, Hp, Wp, 2) [and the 1/8 flows (n, Hp / 8, Wp / 8, 2)]: numpy, or
        with on_device CUDA tensors on the handle's device (no copy to the host)."""
        n = len(pairs)
        a = (C.c_int * n)(*[int(p[0]) for p in pairs])
        b = (C.c_int * n)(*[int(p[1]) for p in pairs])
        if on_device:
            import torch
            dev = torch.device("cuda:%d" % self.device)
            up = torch.empty((n, self.Hp, self.Wp, 2), device=dev)
            lo = torch.empty((n, self.Hp // 8, self.Wp // 8, 2), device=dev) if want_lo else None
            torch.cuda.synchronize(dev)
            _chk(self.lib.af_raft_flow(self.r, n, a, b, int(iters), C.c_void_p(up.data_ptr()), C.c_void_p(lo.data_ptr()) if want_lo else None, 1))
            return (up, lo) if want_lo else up
        up = np.empty((n, self.Hp, self.Wp, 2), np.float32)
        lo = np.empty((n, self.Hp // 8, self.Wp // 8, 2), np.float32) if want_lo else None
        _chk(self.lib.af_raft_flow(self.r, n, a, b, int(iters), _p(up), _p(lo), 0))
        return (up, lo) if want_lo else up

    def flow(self, im1, im2, iters=20):
        """RAFTWrapper.compute_flow(im1, im2): (Hp, Wp, 2)."""
        self.encode(0, im1)
        self.encode(1, im2)
        return self.flow_slots([(0, 1)], iters)[0]

    def clip(self, frames, iters=20):
        """Yields (i, flow i -> i + 1, flow i + 1 -> i) for every neighbouring pair of `frames` (an iterable of (h, w, 3) images): each frame
        is encoded once, both directions of a pair run as one batch when the capacity allows."""
        prev = None
        for i, f in enumerate(frames):
            cur = i & 1
            self.encode(cur, f)
            if prev is not None:
                if self.capacity >= 2:
                    up = self.flow_slots([(prev, cur), (cur, prev)], iters)
                    yield i - 1, up[0], up[1]
                else:
                    yield i - 1, self.flow_slots([(prev, cur)], iters)[0], self.flow_slots([(cur, prev)], iters)[0]
            prev = cur

    def step(self, slot_a, slot_b, net, coords1):
        """One update iteration from a given state: net (P, 128), coords1 (P, 2) -> (net, delta)."""
        net, coords1 = _f32(net).reshape(self.P, 128), _f32(coords1).reshape(self.P, 2)
        net_out, delta = np.empty_like(net), np.empty_like(coords1)
        _chk(self.lib.af_raft_step(self.r, int(slot_a), int(slot_b), _p(net), _p(coords1), _p(net_out), _p(delta)))
        return net_out, delta

    def lookup(self, slot_a, slot_b, coords):
        """The 324-channel correlation lookup at coords (P, 2) = (x, y) per 1/8-grid position -> (P, 324)."""
        coords = _f32(coords).reshape(self.P, 2)
        out = np.empty((self.P, 324), np.float32)
        _chk(self.lib.af_raft_lookup(self.r, int(slot_a), int(slot_b), _p(coords), _p(out)))
        return out

    def activation(self, name):
        """A named intermediate of batch element 0 of the last call (ACTIVATIONS, corr_vol0..3), (P, C) fp32 numpy."""
        if name.startswith("corr_vol") and name[8:] in ("0", "1", "2", "3"):
            l = int(name[8:])
            ch = ((self.Hp // 8) >> l) * ((self.Wp // 8) >> l)
        elif name in ACTIVATIONS:
            ch = ACTIVATIONS[name]
        else:
            raise KeyError("unknown activation %r (known: %s, corr_vol0..3)" % (name, ", ".join(ACTIVATIONS)))
        out = np.empty((self.P, ch), np.float32)
        _chk(self.lib.af_raft_debug_activation(self.r, name.encode(), _p(out), out.size))
        return out

    def close(self):
        if self.r:
            self.lib.af_raft_destroy(self.r)
            self.r = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
