"""ctypes binding of libatlasfit.so (include/atlasfit.h).

`AtlasFit` mirrors the objects the reference's loop drives (src/stage1_neural_atlas.py:112-231):
two IMLP networks addressed through `state_dict()`-compatible dictionaries (keys `hidden.{i}.weight`,
`hidden.{i}.bias`, implicit_neural_networks.py:37-52), `pre_train_mapping` (unwrap_utils.py:176-198) and the
loop body.  torch is imported first so the library binds to torch's HIP runtime (one runtime per process).
"""
import ctypes as C
import os
import sys

import numpy as np

if __package__:      # a golden-file recipe loads this file by path, outside the package, for REFERENCE_CONFIG alone
    from ._residence import Device, Host

NET_MAPPING1, NET_ATLAS, NET_MAPPING2, NET_ALPHA = 0, 1, 2, 3
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libatlasfit.so")
_lib = None

# symbols declared in include/atlasfit.h (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "af_create", "af_destroy", "af_last_error", "af_upload_video", "af_param_count", "af_set_params",
    "af_get_params", "af_get_adam_state", "af_set_adam_state", "af_pretrain", "af_train_steps",
    "af_render_frame", "af_render_frame_u8", "af_render_frame_at", "af_psnr", "af_sync", "af_debug_forward", "af_set_debug", "af_get_last_grads",
    "af_set_timing", "af_get_timing", "af_step_work", "af_loss_width", "af_config_size", "af_debug_records", "af_debug_plan",
    "af_resize_bilinear", "af_resize_area", "af_luma_grid", "af_yuv_to_rgb", "af_rgb_to_yuv", "af_yuv_frame_bytes", "af_mask_step", "af_mask_blend", "af_guided_coeffs", "af_guided_apply", "af_yuv_to_rgb16", "af_rgb_to_yuv16", "af_depth_reduce", "af_guided_apply16", "af_guided_coeffs_colour", "af_guided_apply_colour", "af_guided_apply_colour16", "af_fidelity", "af_flow_consistency", "af_debug_dw_clocks", "af_debug_step_clocks", "af_set_dw_mode", "af_set_mlp_mode", "af_debug_dw_schedule",
    "af_debug_set_dw_cost", "af_debug_tiles", "af_get_modes",
    "af_render_layers", "af_mapping_area", "af_render_atlas_texture", "af_render_edit", "af_render_loss_maps",
    "af_render_layers_at", "af_edit_create", "af_edit_frame", "af_edit_usage", "af_edit_reset_usage", "af_edit_destroy",
    "af_warp_error_pair", "af_warp_error",
    "af_filter_create", "af_filter_destroy", "af_filter_param_count", "af_filter_set_params", "af_filter_reset", "af_filter_frame",
    "af_filter_debug_activation", "af_conv2d", "af_filter_set_precision", "af_filter_get_precision", "af_conv2d_prec",
    "af_raft_create", "af_raft_destroy", "af_raft_param_count", "af_raft_info", "af_raft_set_params", "af_raft_encode", "af_raft_flow",
    "af_raft_step", "af_raft_lookup", "af_raft_debug_activation", "af_raft_conv2d", "af_raft_gru", "af_raft_instance_norm",
    "af_raft_set_precision", "af_raft_get_precision", "af_raft_conv2d_prec", "af_raft_gru_prec", "af_raft_instance_norm_prec",
]


AF_ERANGE = -6      # include/atlasfit.h
AF_ESTATE = -5


class AtlasFitError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("atlasfit error %d: %s" % (code, msg))
        self.code = code


class AfConfig(C.Structure):
    _fields_ = [
        ("resx", C.c_int32), ("resy", C.c_int32), ("number_of_frames", C.c_int32),
        ("samples_batch", C.c_int32),
        ("number_of_channels_mapping1", C.c_int32), ("number_of_layers_mapping1", C.c_int32),
        ("number_of_channels_atlas", C.c_int32), ("number_of_layers_atlas", C.c_int32),
        ("positional_encoding_num_atlas", C.c_int32),
        ("use_positional_encoding_mapping1", C.c_int32),
        ("derivative_amount", C.c_int32),
        ("include_global_rigidity_loss", C.c_int32),
        ("global_rigidity_derivative_amount_fg", C.c_int32),
        ("stop_global_rigidity", C.c_int32),
        ("use_gradient_loss", C.c_int32),
        ("rgb_coeff", C.c_float), ("gradient_loss_coeff", C.c_float), ("rigidity_coeff", C.c_float),
        ("optical_flow_coeff", C.c_float),
        ("global_rigidity_coeff_fg", C.c_float),
        ("uv_mapping_scale", C.c_float),
        ("lr", C.c_float),
        ("pretrain_batch", C.c_int32),
        # fg/bg dual-atlas path (src/stage1_neural_atlas_seg.py); read only when two_layer != 0
        ("two_layer", C.c_int32),
        ("number_of_channels_mapping2", C.c_int32), ("number_of_layers_mapping2", C.c_int32),
        ("number_of_channels_alpha", C.c_int32), ("number_of_layers_alpha", C.c_int32),
        ("positional_encoding_num_alpha", C.c_int32),
        ("use_positional_encoding_mapping2", C.c_int32),
        ("global_rigidity_derivative_amount_bg", C.c_int32),
        ("stop_bootstrapping_iteration", C.c_int32),
        ("global_rigidity_coeff_bg", C.c_float),
        ("alpha_bootstrapping_factor", C.c_float), ("alpha_flow_factor", C.c_float), ("sparsity_coeff", C.c_float),
        ("number_of_positional_encoding_mapping1", C.c_int32), ("number_of_positional_encoding_mapping2", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


# the shipped hyper-parameters (reference src/config/config_flow_100.json)
REFERENCE_CONFIG = {
    "maximum_number_of_frames": 200, "iters_num": 10001, "samples_batch": 10000, "optical_flow_coeff": 500.0,
    "evaluate_every": 10000, "derivative_amount": 1, "rgb_coeff": 5000, "rigidity_coeff": 1.0,
    "uv_mapping_scale": 0.8, "pretrain_mapping1": True, "pretrain_mapping2": True,
    "alpha_bootstrapping_factor": 2000.0, "alpha_flow_factor": 4900.0, "positional_encoding_num_alpha": 5,
    "number_of_channels_atlas": 256, "number_of_layers_atlas": 8, "number_of_channels_alpha": 256,
    "number_of_layers_alpha": 8, "stop_bootstrapping_iteration": 10000, "number_of_channels_mapping1": 256,
    "number_of_layers_mapping1": 6, "number_of_channels_mapping2": 256, "number_of_layers_mapping2": 4,
    "gradient_loss_coeff": 1000, "use_gradient_loss": True, "sparsity_coeff": 1000.0,
    "positional_encoding_num_atlas": 10, "use_positional_encoding_mapping1": False,
    "number_of_positional_encoding_mapping1": 4, "use_positional_encoding_mapping2": False,
    "number_of_positional_encoding_mapping2": 2, "pretrain_iter_number": 100, "load_checkpoint": False,
    "checkpoint_path": "", "include_global_rigidity_loss": True, "global_rigidity_derivative_amount_fg": 100,
    "global_rigidity_derivative_amount_bg": 100, "global_rigidity_coeff_fg": 5.0, "global_rigidity_coeff_bg": 50.0,
    "stop_global_rigidity": 5000,
}


def default_config(resx, resy, number_of_frames, config=None, two_layer=False, **over):
    """af_config from the reference's JSON config dict (keys as read at stage1_neural_atlas.py:28-90, or
    stage1_neural_atlas_seg.py:27-107 when two_layer)."""
    cfg = dict(REFERENCE_CONFIG)
    if config:
        cfg.update(config)
    cfg.update(over)
    c = AfConfig()
    c.two_layer = int(bool(two_layer))
    c.number_of_channels_mapping2 = int(cfg["number_of_channels_mapping2"])
    c.number_of_layers_mapping2 = int(cfg["number_of_layers_mapping2"])
    c.number_of_channels_alpha = int(cfg["number_of_channels_alpha"])
    c.number_of_layers_alpha = int(cfg["number_of_layers_alpha"])
    c.positional_encoding_num_alpha = int(cfg["positional_encoding_num_alpha"])
    c.use_positional_encoding_mapping2 = int(bool(cfg["use_positional_encoding_mapping2"]))
    c.number_of_positional_encoding_mapping1 = int(cfg.get("number_of_positional_encoding_mapping1", 4))
    c.number_of_positional_encoding_mapping2 = int(cfg.get("number_of_positional_encoding_mapping2", 2))
    c.global_rigidity_derivative_amount_bg = int(cfg["global_rigidity_derivative_amount_bg"])
    c.stop_bootstrapping_iteration = int(cfg["stop_bootstrapping_iteration"])
    c.global_rigidity_coeff_bg = float(cfg["global_rigidity_coeff_bg"])
    c.alpha_bootstrapping_factor = float(cfg["alpha_bootstrapping_factor"])
    c.alpha_flow_factor = float(cfg["alpha_flow_factor"])
    c.sparsity_coeff = float(cfg["sparsity_coeff"])
    c.resx, c.resy, c.number_of_frames = int(resx), int(resy), int(number_of_frames)
    c.samples_batch = int(cfg["samples_batch"])
    c.number_of_channels_mapping1 = int(cfg["number_of_channels_mapping1"])
    c.number_of_layers_mapping1 = int(cfg["number_of_layers_mapping1"])
    c.number_of_channels_atlas = int(cfg["number_of_channels_atlas"])
    c.number_of_layers_atlas = int(cfg["number_of_layers_atlas"])
    c.positional_encoding_num_atlas = int(cfg["positional_encoding_num_atlas"])
    c.use_positional_encoding_mapping1 = int(bool(cfg["use_positional_encoding_mapping1"]))
    c.derivative_amount = int(cfg["derivative_amount"])
    c.include_global_rigidity_loss = int(bool(cfg["include_global_rigidity_loss"]))
    c.global_rigidity_derivative_amount_fg = int(cfg["global_rigidity_derivative_amount_fg"])
    c.stop_global_rigidity = int(cfg["stop_global_rigidity"])
    c.use_gradient_loss = int(bool(cfg["use_gradient_loss"]))
    c.rgb_coeff = float(cfg["rgb_coeff"])
    c.gradient_loss_coeff = float(cfg["gradient_loss_coeff"])
    c.rigidity_coeff = float(cfg["rigidity_coeff"])
    c.optical_flow_coeff = float(cfg["optical_flow_coeff"])
    c.global_rigidity_coeff_fg = float(cfg["global_rigidity_coeff_fg"])
    c.uv_mapping_scale = float(cfg["uv_mapping_scale"])
    c.lr = float(cfg.get("lr", 1e-4))
    c.pretrain_batch = int(cfg.get("pretrain_batch", 10000))
    return c


def load_library(path=None):
    """dlopen libatlasfit.so.  Fails loudly if it has not been built (python build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (must come first: share torch's HIP runtime)
    path = path or os.environ.get("AF_LIB_PATH") or _LIB_PATH      # AF_LIB_PATH: an experiment build of the same library (tools/ab_step.sh), never a fallback
    if not os.path.exists(path):
        raise AtlasFitError(-100, "libatlasfit.so not built: run `python %s`" % os.path.join(_HERE, "build.py"))
    lib = C.CDLL(path)
    vp, i32, i64, u64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t
    fp = C.POINTER(C.c_float)
    sig = {
        "af_create": (i32, [C.POINTER(AfConfig), i32, C.POINTER(vp)]),
        "af_destroy": (None, [vp]),
        "af_last_error": (C.c_char_p, [vp]),
        "af_upload_video": (i32, [vp, vp, vp, vp, vp, vp, vp, i32]),
        "af_param_count": (sz, [vp, i32]),
        "af_set_params": (i32, [vp, i32, vp, sz]),
        "af_get_params": (i32, [vp, i32, vp, sz]),
        "af_get_adam_state": (i32, [vp, i32, vp, vp, C.POINTER(i64)]),
        "af_set_adam_state": (i32, [vp, i32, vp, vp, i64]),
        "af_pretrain": (i32, [vp, i32, i32, vp, vp, u64, vp]),
        "af_train_steps": (i32, [vp, i32, i32, vp, u64, vp]),
        "af_render_frame": (i32, [vp, i32, vp, C.POINTER(C.c_double)]),
        "af_render_frame_u8": (i32, [vp, i32, vp, vp, i32, C.POINTER(C.c_double)]),
        "af_render_frame_at": (i32, [vp, i32, i32, i32, vp, vp, vp, C.POINTER(C.c_double), i32]),
        "af_psnr": (i32, [vp, C.POINTER(C.c_double), vp]),
        "af_sync": (i32, [vp]),
        "af_debug_forward": (i32, [vp, i32, vp, i32, vp]),
        "af_set_debug": (i32, [vp, i32]),
        "af_get_last_grads": (i32, [vp, i32, vp, sz]),
        "af_set_timing": (i32, [vp, i32]),
        "af_get_timing": (i32, [vp, vp, vp, vp, i32]),
        "af_step_work": (i32, [vp, i32, C.POINTER(i64 * 4), C.POINTER(C.c_double)]),
        "af_loss_width": (i32, [vp]),
        "af_config_size": (sz, []),
        "af_debug_records": (i32, [vp, vp, i32, vp]),
        "af_debug_plan": (i32, [i32, i32, i32, i32, C.POINTER(i32 * 3)]),
        "af_resize_bilinear": (i32, [i32, vp, i32, i32, i32, i32, vp, i32, i32, i64, i64, i64, C.c_double, C.c_double, i32]),
        "af_resize_area": (i32, [i32, vp, i32, i32, i32, vp, i32, i32, i32]),
        "af_luma_grid": (i32, [i32, vp, i32, i32, i32, i32, i32, vp, i32]),
        "af_yuv_to_rgb": (i32, [i32, vp, i32, i32, i32, i32, i32, vp, i32]),
        "af_rgb_to_yuv": (i32, [i32, vp, i32, i32, i32, i32, i32, vp, i32]),
        "af_yuv_frame_bytes": (i64, [i32, i32, i32]),
        "af_mask_step": (i32, [i32, vp, vp, vp, vp, i32, i32, C.c_float, vp, vp, i32]),
        "af_mask_blend": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32]),
        "af_guided_coeffs": (i32, [i32, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp, i32]),
        "af_guided_apply": (i32, [i32, vp, i32, i32, vp, vp, i32, i32, vp, i32]),
        "af_yuv_to_rgb16": (i32, [i32, vp, i32, i32, i32, i32, i32, i32, vp, i32]),
        "af_rgb_to_yuv16": (i32, [i32, vp, i32, i32, i32, i32, i32, i32, vp, i32]),
        "af_depth_reduce": (i32, [i32, vp, i64, i32, vp, i32]),
        "af_guided_apply16": (i32, [i32, vp, i32, i32, i32, vp, vp, i32, i32, vp, i32]),
        "af_guided_coeffs_colour": (i32, [i32, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp, i32]),
        "af_guided_apply_colour": (i32, [i32, vp, i32, i32, vp, vp, i32, i32, vp, i32]),
        "af_guided_apply_colour16": (i32, [i32, vp, i32, i32, i32, vp, vp, i32, i32, vp, i32]),
        "af_fidelity": (i32, [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32]),
        "af_flow_consistency": (i32, [i32, vp, vp, i32, i32, vp, i64, i64, C.c_float, i32]),
        "af_debug_dw_clocks": (i32, [vp, i32, vp, i32]),
        "af_debug_step_clocks": (i32, [vp, i32, vp, i32]),
        "af_debug_dw_schedule": (i32, [vp, i32, vp, i32]),
        "af_set_dw_mode": (i32, [vp, i32]),
        "af_set_mlp_mode": (i32, [vp, i32]),
        "af_debug_set_dw_cost": (i32, [vp, vp, C.c_double]),
        "af_debug_tiles": (i32, [vp, i32, i32, i32, i32, i32, i32, vp]),
        "af_get_modes": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "af_render_layers": (i32, [vp, i32, vp, vp, vp, vp, vp]),
        "af_mapping_area": (i32, [vp, i32, vp]),
        "af_render_atlas_texture": (i32, [vp, i32, C.c_float, C.c_float, C.c_float, vp]),
        "af_render_edit": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "af_render_loss_maps": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "af_render_layers_at": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32]),
        "af_edit_create": (i32, [vp, i32, vp, vp, vp, vp, i32, C.POINTER(vp)]),
        "af_edit_frame": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, i32]),
        "af_edit_usage": (i32, [vp, vp, vp]),
        "af_edit_reset_usage": (i32, [vp]),
        "af_edit_destroy": (None, [vp]),
        "af_warp_error_pair": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, C.POINTER(C.c_double), vp, vp, i32]),
        "af_warp_error": (i32, [vp, i32, i32, vp, C.POINTER(C.c_double)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    if lib.af_config_size() != C.sizeof(AfConfig):
        raise AtlasFitError(-101, "af_config mirror (%d B) does not match libatlasfit.so (%d B): rebuild" % (C.sizeof(AfConfig), lib.af_config_size()))
    _lib = lib
    return lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _render_outputs(af, oh, ow, spec, on_device):
    """The output arrays of a render of `af` on an (oh, ow) grid, spec = {name: (trailing shape, numpy dtype)}: numpy arrays, or with
    on_device torch CUDA tensors on the handle's device (the device is synchronised first: the library runs on its own stream).  Returns
    (arrays, ptr): ptr(name) is the pointer to pass to the library, None for a name that was not asked for."""
    hw = (max(int(oh), 0), max(int(ow), 0))
    if on_device:
        import torch
        res = Device(torch.device("cuda", af.device))
    else:
        res = Host()
    out = {n: res.empty(hw + tail, np.dtype(dt).name) for n, (tail, dt) in spec.items()}
    res.sync()
    return out, lambda n: res.ptr(out.get(n))


# layer shapes of the IMLPs (stage1_neural_atlas.py:112-128; stage1_neural_atlas_seg.py:127-161; IMLP.__init__,
# implicit_neural_networks.py:16-60: skip layers [4, 7] on the atlas net only)
def imlp_shapes(net, cfg=None, pe_atlas=10, pe_alpha=5):
    """[(out_features, in_features)] per layer.  With `cfg` (an AfConfig) the widths / depths / PE sizes come from it —
    AtlasFit.__init__ checks the result against the library's own parameter count, so a config the library cannot run
    fails loudly in Python, before anything reaches the C side."""
    hid = {NET_MAPPING1: 256, NET_MAPPING2: 256, NET_ATLAS: 256, NET_ALPHA: 256}
    nl = {NET_MAPPING1: 6, NET_MAPPING2: 4, NET_ATLAS: 8, NET_ALPHA: 8}
    if cfg is not None:
        hid = {NET_MAPPING1: cfg.number_of_channels_mapping1, NET_MAPPING2: cfg.number_of_channels_mapping2,
               NET_ATLAS: cfg.number_of_channels_atlas, NET_ALPHA: cfg.number_of_channels_alpha}
        nl = {NET_MAPPING1: cfg.number_of_layers_mapping1, NET_MAPPING2: cfg.number_of_layers_mapping2,
              NET_ATLAS: cfg.number_of_layers_atlas, NET_ALPHA: cfg.number_of_layers_alpha}
        pe_atlas, pe_alpha = cfg.positional_encoding_num_atlas, cfg.positional_encoding_num_alpha
    if net not in hid:
        raise ValueError("net")
    h, L = int(hid[net]), int(nl[net])
    enc = {NET_MAPPING1: 3, NET_MAPPING2: 3, NET_ATLAS: 4 * pe_atlas, NET_ALPHA: 6 * pe_alpha}[net]
    if cfg is not None:     # a mapping net with positional encoding reads 2 * 3 * K Fourier features (implicit_neural_networks.py:28-33)
        if net == NET_MAPPING1 and cfg.use_positional_encoding_mapping1:
            enc = 6 * int(cfg.number_of_positional_encoding_mapping1)
        if net == NET_MAPPING2 and cfg.use_positional_encoding_mapping2:
            enc = 6 * int(cfg.number_of_positional_encoding_mapping2)
    out = {NET_MAPPING1: 2, NET_MAPPING2: 2, NET_ATLAS: 3, NET_ALPHA: 1}[net]
    skips = (4, 7) if net == NET_ATLAS else ()
    dims = []
    for i in range(L):
        fan_in = enc if i == 0 else (h + enc if i in skips else h)
        dims.append((out if i == L - 1 else h, fan_in))
    return dims


def flatten_state_dict(sd, net, cfg=None):
    """IMLP.state_dict() (torch tensors or arrays) -> flat fp32 vector in state_dict order."""
    parts = []
    for i, (o, k) in enumerate(imlp_shapes(net, cfg)):
        w = np.asarray(sd["hidden.%d.weight" % i].detach().cpu().numpy() if hasattr(sd["hidden.%d.weight" % i], "detach") else sd["hidden.%d.weight" % i], dtype=np.float32)
        b = np.asarray(sd["hidden.%d.bias" % i].detach().cpu().numpy() if hasattr(sd["hidden.%d.bias" % i], "detach") else sd["hidden.%d.bias" % i], dtype=np.float32)
        assert w.shape == (o, k) and b.shape == (o,), (i, w.shape, b.shape)
        parts += [w.reshape(-1), b]
    return np.concatenate(parts)


def unflatten_state_dict(flat, net, cfg=None):
    out, off = {}, 0
    for i, (o, k) in enumerate(imlp_shapes(net, cfg)):
        out["hidden.%d.weight" % i] = flat[off:off + o * k].reshape(o, k).copy(); off += o * k
        out["hidden.%d.bias" % i] = flat[off:off + o].copy(); off += o
    assert off == flat.size
    return out


# ---- input builder on the device (unwrap_utils.py:10-38,105-163) ------------------------------------------------
def _util_chk(rc):
    if rc != 0:
        raise AtlasFitError(rc, load_library().af_last_error(None).decode())


def resize_bilinear_device(src, dst, dh, dw, pix_stride, ch_stride, offset, scale=(1.0, 1.0), device=0):
    """cv2.resize(src, (dw, dh)) (INTER_LINEAR) on the GPU.  src: torch CUDA tensor (H, W, C), uint8 or float32,
    contiguous.  dst: torch CUDA float32 tensor; element (y, x, c) is written at
    dst.view(-1)[(y*dw + x)*pix_stride + c*ch_stride + offset] (so a frame can land directly in (resy,resx,C,F))."""
    import torch
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous() and dst.dtype == torch.float32
    assert src.dtype in (torch.uint8, torch.float32) and src.dim() == 3
    torch.cuda.synchronize()
    sh, sw, ch = src.shape
    _util_chk(load_library().af_resize_bilinear(int(device), C.c_void_p(src.data_ptr()), int(src.dtype == torch.uint8), sh, sw, ch,
                                                C.c_void_p(dst.data_ptr()), int(dh), int(dw), int(pix_stride), int(ch_stride), int(offset),
                                                float(scale[0]), float(scale[1]), 1))


def _resize_area(res, src, dh, dw):
    """af_resize_area of an (H, W, C) uint8 image over a residence (_residence.py)."""
    src = res.contiguous(src)
    sh, sw, ch = src.shape
    dst = res.empty((max(int(dh), 0), max(int(dw), 0), ch), "uint8")
    res.sync()
    _util_chk(load_library().af_resize_area(res.ordinal, res.ptr(src), sh, sw, ch, res.ptr(dst), int(dh), int(dw), res.on_device))
    return dst


def resize_area_device(src, dh, dw, device=0):
    """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) of a uint8 image on the GPU, shrinking only (af_resize_area).
    src: torch CUDA uint8 tensor (H, W, C), C in 1..4.  Returns a (dh, dw, C) uint8 CUDA tensor."""
    import torch
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3
    return _resize_area(Device(src.device, device, sync_current=True), src, dh, dw)


def resize_area(img, dh, dw, device=0):
    """The same resize of a numpy uint8 image (H, W, C) or (H, W) through host pointers: the library stages the image on the GPU
    and copies the result back.  Returns a uint8 array (dh, dw, C), or (dh, dw) for a 2-D input."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("resize_area: expected a uint8 image (H, W[, C]), got %s %s" % (img.shape, img.dtype))
    dst = _resize_area(Host(device), img.reshape(img.shape[0], img.shape[1], -1), dh, dw)
    return dst if img.ndim == 3 else dst[:, :, 0]


def flow_consistency_device(flow12, flow21, out, pix_stride, offset, thresh=1.0, device=0):
    """unwrap_utils.py:10-23,151-159: out.view(-1)[(y*w + x)*pix_stride + offset] = (|| f12 + remap(f21, f12) || < thresh)
    as 1.0 / 0.0 (thresh <= 0: the norm itself).  flow12 / flow21: torch CUDA float32 (h, w, 2) contiguous."""
    import torch
    assert flow12.is_cuda and flow21.is_cuda and out.is_cuda and flow12.is_contiguous() and flow21.is_contiguous() and out.is_contiguous()
    assert flow12.dtype == torch.float32 and flow12.shape == flow21.shape and flow12.shape[2] == 2
    torch.cuda.synchronize()
    h, w, _ = flow12.shape
    _util_chk(load_library().af_flow_consistency(int(device), C.c_void_p(flow12.data_ptr()), C.c_void_p(flow21.data_ptr()), h, w,
                                                 C.c_void_p(out.data_ptr()), int(pix_stride), int(offset), float(thresh), 1))


# ---- warping error E_warp (Lai et al. 2018; src/models/utils.py:478-572; include/atlasfit.h af_warp_error_pair) -------------
def warp_error_pair(img1, img2, flow12, flow21, align_corners=True, device=0, return_maps=False):
    """E of one frame pair: sum noc (flow_warping(img2, flow12) - img1)^2 / (3 sum noc), noc = 1 - detect_occlusion(flow21, flow12).
    img1 / img2 (H, W, 3) and flow12 / flow21 (H, W, 2, pixels) are numpy arrays or CUDA torch tensors (then nothing leaves the
    device).  align_corners True ("exact": zero flow is the identity) or False ("reference": the reference's function under
    torch >= 1.3).  Returns E (float), or with return_maps (E, noc (H, W) 0/1, warped (H, W, 3)) as arrays of the inputs' kind."""
    if align_corners not in (True, False, 0, 1):
        raise ValueError("align_corners must be True / False")
    if hasattr(img1, "is_cuda") and img1.is_cuda:
        arrs = [t.contiguous().float() for t in (img1, img2, flow12, flow21)]
        dev = arrs[0].device
        assert all(t.is_cuda and t.device == dev for t in arrs), "all inputs on the same CUDA device"
        res = Device(dev, dev.index if dev.index is not None else device)
    else:
        arrs = [_f32(a.numpy() if hasattr(a, "numpy") else a) for a in (img1, img2, flow12, flow21)]
        res = Host(device)
    H, W = arrs[0].shape[:2]
    for a, ch in zip(arrs, (3, 3, 2, 2)):
        if tuple(a.shape) != (H, W, ch):
            raise ValueError("warp_error_pair: expected (%d, %d, %d), got %s" % (H, W, ch, tuple(a.shape)))
    err = C.c_double(0)
    noc = res.empty((H, W), "float32") if return_maps else None
    warped = res.empty((H, W, 3), "float32") if return_maps else None
    res.sync()
    _util_chk(load_library().af_warp_error_pair(res.ordinal, *[res.ptr(a) for a in arrs], int(H), int(W), int(bool(align_corners)), C.byref(err),
                                                res.ptr(noc), res.ptr(warped), res.on_device))
    return (float(err.value), noc, warped) if return_maps else float(err.value)


class AtlasFit:
    """One video on one MI355X.  Mirrors the objects of stage1_neural_atlas.main()."""

    LOSS_NAMES = ("rgb", "gradient", "rigidity", "global_rigidity", "flow", "total", "valid_fwd", "valid_bwd")
    LOSS_NAMES_TWO_LAYER = ("rgb", "gradient", "rigidity1", "rigidity2", "global_rigidity1", "global_rigidity2", "flow1", "flow2",
                            "flow_alpha", "alpha_bootstrapping", "sparsity", "total", "valid_fwd", "valid_bwd", "_", "_")
    TIMING_NAMES = ("prep", "fwd_1", "fwd_2", "loss", "bwd_1", "bwd_2", "dw", "adam")

    def __init__(self, cfg, device=0):
        self.lib = load_library()
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.lib.af_create(C.byref(cfg), int(device), C.byref(h))
        if rc != 0:
            raise AtlasFitError(rc, self.lib.af_last_error(None).decode())
        self.h = h
        self.device = int(device)
        self.N = cfg.samples_batch
        self.two_layer = bool(cfg.two_layer)
        self.nets = (NET_MAPPING1, NET_MAPPING2, NET_ATLAS, NET_ALPHA) if self.two_layer else (NET_MAPPING1, NET_ATLAS)
        self.loss_width = int(self.lib.af_loss_width(h))
        for net in self.nets:                       # the Python view of the architecture must be the library's
            n = sum(o * k + o for o, k in imlp_shapes(net, cfg))
            built = self.param_count(net)
            if n != built:
                self.close()
                raise AtlasFitError(-1, "net %d: config describes %d parameters, libatlasfit.so built %d" % (net, n, built))
        self._apply_experiment_env()

    def _apply_experiment_env(self):
        """The A/B tools' environment switches, mapped onto the explicit calls (libatlasfit.so itself reads no environment):
        AF_MLP_MODE / AF_MLP_FP32, AF_DW_MODE / AF_DW_FP32 (include/atlasfit.h: af_set_mlp_mode, af_set_dw_mode) and
        AF_DW_COST="c8x8,c8x2,c8x1,c1x8,c1x2[,seg]" (af_debug_set_dw_cost; tools/dw_cost_sweep.sh).
        Honoured ONLY under AF_EXPERIMENT=1 (a stale exported AF_*MODE must not switch the arithmetic of a production run silently), every
        override is reported on stderr, and `self.arithmetic` records what is in force (stage1.py writes it into the results' config.json)."""
        env = os.environ
        m, d = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.af_get_modes(self.h, C.byref(m), C.byref(d)))
        self.arithmetic = {"mlp_mode": int(m.value), "dw_mode": int(d.value), "dw_cost": None, "overrides": []}
        asked = [k for k in ("AF_MLP_FP32", "AF_MLP_MODE", "AF_DW_FP32", "AF_DW_MODE", "AF_DW_COST") if env.get(k)]
        if not asked:
            return
        if env.get("AF_EXPERIMENT", "0") in ("", "0"):
            sys.stderr.write("[atlasfit] ignoring %s: experiment switches need AF_EXPERIMENT=1\n" % ", ".join("%s=%s" % (k, env[k]) for k in asked))
            return
        try:
            if env.get("AF_MLP_FP32") and int(env["AF_MLP_FP32"]):
                self.set_mlp_mode(0)
            elif env.get("AF_MLP_MODE"):
                self.set_mlp_mode(int(env["AF_MLP_MODE"]))
            if env.get("AF_DW_FP32") and int(env["AF_DW_FP32"]):
                self.set_dw_mode(0)
            elif env.get("AF_DW_MODE"):
                self.set_dw_mode(int(env["AF_DW_MODE"]))
            if env.get("AF_DW_COST"):
                self.set_dw_cost(env["AF_DW_COST"])
        except Exception:
            self.close()
            raise
        self.arithmetic["overrides"] = ["%s=%s" % (k, env[k]) for k in asked]
        sys.stderr.write("[atlasfit] AF_EXPERIMENT: %s -> mlp_mode %d, dw_mode %d\n" % (", ".join(self.arithmetic["overrides"]), self.arithmetic["mlp_mode"], self.arithmetic["dw_mode"]))

    def close(self):
        for s in list(getattr(self, "_sessions", ())):      # open edit sessions go first: their device memory is the handle's device's
            s.close()
        if getattr(self, "h", None):
            self.lib.af_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise AtlasFitError(rc, self.lib.af_last_error(self.h).decode())

    # ---- data (load_input_data_single outputs, unwrap_utils.py:105-163)
    def upload_video(self, video_frames, optical_flows, optical_flows_reverse, optical_flows_mask,
                     optical_flows_reverse_mask, mask_frames=None):
        c = self.cfg
        shp = (c.resy, c.resx, 3, c.number_of_frames)
        if hasattr(video_frames, "is_cuda") and video_frames.is_cuda:      # torch tensors already in HBM
            ts = [video_frames, optical_flows, optical_flows_reverse, optical_flows_mask, optical_flows_reverse_mask, mask_frames]
            ts = [None if t is None else t.contiguous().float() for t in ts]
            assert tuple(ts[0].shape) == shp, (tuple(ts[0].shape), shp)
            import torch
            torch.cuda.synchronize()
            ptrs = [None if t is None else C.c_void_p(t.data_ptr()) for t in ts]
            self._chk(self.lib.af_upload_video(self.h, *ptrs, 1))
            return
        arrs = [video_frames, optical_flows, optical_flows_reverse, optical_flows_mask, optical_flows_reverse_mask, mask_frames]
        arrs = [None if a is None else _f32(a.numpy() if hasattr(a, "numpy") else a) for a in arrs]
        assert arrs[0].shape == shp, (arrs[0].shape, shp)
        assert arrs[1].size == c.resy * c.resx * 2 * c.number_of_frames
        assert arrs[3].size == c.resy * c.resx * c.number_of_frames
        self._chk(self.lib.af_upload_video(self.h, *[_ptr(a) for a in arrs], 0))

    # ---- parameters
    def param_count(self, net):
        return int(self.lib.af_param_count(self.h, net))

    def load_state_dict(self, net, sd):
        flat = flatten_state_dict(sd, net, self.cfg)
        self._chk(self.lib.af_set_params(self.h, net, _ptr(flat), flat.size))

    def state_dict(self, net):
        flat = np.empty(self.param_count(net), np.float32)
        self._chk(self.lib.af_get_params(self.h, net, _ptr(flat), flat.size))
        return unflatten_state_dict(flat, net, self.cfg)

    def get_params_flat(self, net):
        flat = np.empty(self.param_count(net), np.float32)
        self._chk(self.lib.af_get_params(self.h, net, _ptr(flat), flat.size))
        return flat

    def adam_state(self, net):
        n = self.param_count(net)
        m, v, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
        self._chk(self.lib.af_get_adam_state(self.h, net, _ptr(m), _ptr(v), C.byref(step)))
        return m, v, int(step.value)

    def set_adam_state(self, net, m, v, step):
        m, v = _f32(m), _f32(v)
        self._chk(self.lib.af_set_adam_state(self.h, net, _ptr(m), _ptr(v), int(step)))

    # ---- pre_train_mapping (unwrap_utils.py:176-198)
    def pre_train_mapping(self, pretrain_iters, ys=None, xs=None, seed=0, net=NET_MAPPING1, return_losses=False):
        steps = pretrain_iters * self.cfg.number_of_frames
        losses = np.zeros(steps, np.float32) if return_losses else None
        if ys is not None:
            ys = np.ascontiguousarray(ys, np.int64); xs = np.ascontiguousarray(xs, np.int64)
            assert ys.size == steps * self.cfg.pretrain_batch == xs.size
        self._chk(self._range_fallback(self.lib.af_pretrain(self.h, net, int(pretrain_iters), _ptr(ys), _ptr(xs), int(seed), _ptr(losses)), "af_pretrain"))
        return losses

    # ---- the loop body (stage1_neural_atlas.py:151-231)
    def train_steps(self, first_iter, n_iters, inds=None, seed=0, return_losses=True):
        losses = np.zeros((n_iters, self.loss_width), np.float32) if return_losses else None
        if inds is not None:
            inds = np.ascontiguousarray(inds, np.int64)
            assert inds.size == n_iters * self.N, (inds.shape, n_iters, self.N)
        self._chk(self._range_fallback(self.lib.af_train_steps(self.h, int(first_iter), int(n_iters), _ptr(inds), int(seed), _ptr(losses)), "af_train_steps"))
        return losses

    range_fallback = False

    def _range_fallback(self, rc, what):
        """AF_ERANGE (include/atlasfit.h): in the f16x3 arithmetic k_adam saw a hidden-layer weight at |w| >= 8 — half of what the fp16 weight images
        hold.  The steps of the call that reports it are complete and valid (the images are finite below 16 and Adam moves a weight by <= lr per step;
        the losses are already written), so a caller that must not stop — the stage-1 CLIs set `range_fallback = True` — goes on from the same state
        on the bf16x6 chains, which have no range limit; said on stderr and recorded in `self.arithmetic` (-> config.json).  Off by default: the
        library's own behaviour is the error."""
        if rc != AF_ERANGE or not self.range_fallback:
            return rc
        msg = self.lib.af_last_error(self.h).decode()
        self.set_mlp_mode(1)
        self.arithmetic.setdefault("overrides", []).append("range fallback after %s: mlp_mode 3 -> 1" % what)
        sys.stderr.write("[atlasfit] %s -- continuing from the same state on the bf16x6 chains (af_set_mlp_mode(h, 1))\n" % msg)
        return 0

    # ---- evaluate_model_single core (evaluate.py:640-743)
    def render_frame(self, f):
        rgb = np.empty((self.cfg.resy, self.cfg.resx, 3), np.float32)
        sse = C.c_double(0)
        self._chk(self.lib.af_render_frame(self.h, int(f), _ptr(rgb), C.byref(sse)))
        return rgb, float(sse.value)

    def _render(self, f, oh, ow, want_float, want_u8, ref, on_device):
        """(rgb, u8, sse) of frame f on an (oh, ow) grid: the lattice frame of the uploaded video (oh None: af_render_frame_u8, sse against
        the video) or af_render_frame_at (sse against `ref`, None without it)."""
        lattice = oh is None
        spec = dict(rgb=((3,), np.float32), u8=((3,), np.uint8))
        out, p = _render_outputs(self, self.cfg.resy if lattice else oh, self.cfg.resx if lattice else ow,
                                 {n: spec[n] for n, want in (("rgb", want_float), ("u8", want_u8)) if want}, on_device)
        sse = C.c_double(0)
        if lattice:
            self._chk(self.lib.af_render_frame_u8(self.h, int(f), p("rgb"), p("u8"), int(on_device), C.byref(sse)))
        else:
            ref_p = None if ref is None else C.c_void_p(ref.data_ptr()) if on_device else _ptr(ref)
            self._chk(self.lib.af_render_frame_at(self.h, int(f), int(oh), int(ow), p("rgb"), p("u8"), ref_p, C.byref(sse) if ref is not None else None,
                                                  int(on_device)))
        return out.get("rgb"), out.get("u8"), (float(sse.value) if lattice or ref is not None else None)

    def render_frame_device(self, f, want_float=True, want_u8=True):
        """render_frame without the host round trip (af_render_frame_u8): (rgb, u8, sse) with rgb a (resy, resx, 3) float32 and u8 a
        (resy, resx, 3) uint8 torch CUDA tensor on the handle's device (None when not wanted).  rgb is render_frame's array bit for bit;
        u8 is (rgb.astype(float64) * 255).astype(uint8), the pixels evaluate_model_single writes to stage_1/output."""
        return self._render(f, None, None, want_float, want_u8, None, True)

    def render_frame_u8(self, f, want_float=True, want_u8=True):
        """render_frame_device with host (numpy) outputs: (rgb, u8, sse)."""
        return self._render(f, None, None, want_float, want_u8, None, False)

    # ---- the same reconstruction at another size (include/atlasfit.h af_render_frame_at)
    def render_frame_at(self, f, oh, ow, ref=None):
        """Frame f with the nets evaluated at the pixel centres of an (oh, ow) grid over the stage-1 lattice (cv2.resize's pixel-centre
        geometry, clamped at the border): rgb (oh, ow, 3) float32; with `ref`, an (oh, ow, 3) uint8 image, (rgb, sse) with sse the fp64
        sum of (ref / 255 - rgb)^2.  (resy, resx) gives render_frame's array bit for bit.  Forward-only; needs no uploaded video."""
        rgb, _, sse = self.render_frame_at_u8(f, oh, ow, want_u8=False, ref=ref)
        return rgb if ref is None else (rgb, sse)

    def render_frame_at_u8(self, f, oh, ow, want_float=True, want_u8=True, ref=None):
        """render_frame_at_device with host (numpy) arrays: (rgb, u8, sse), None for what was not asked for."""
        shp = (int(oh), int(ow), 3)
        if ref is not None:
            ref = np.ascontiguousarray(ref)
            if ref.dtype != np.uint8 or ref.shape != shp:
                raise ValueError("render_frame_at: ref must be uint8 %s, got %s %s" % (shp, ref.dtype, ref.shape))
        return self._render(f, oh, ow, want_float, want_u8, ref, False)

    def render_frame_at_device(self, f, oh, ow, want_float=True, want_u8=True, ref=None):
        """render_frame_at without the host round trip: (rgb, u8, sse) with rgb an (oh, ow, 3) float32 and u8 an (oh, ow, 3) uint8 torch
        CUDA tensor on the handle's device (None when not wanted); `ref`: an (oh, ow, 3) uint8 CUDA tensor, sse None without it."""
        import torch
        shp = (int(oh), int(ow), 3)
        if ref is not None:
            if not ref.is_cuda or ref.dtype != torch.uint8 or tuple(ref.shape) != shp:
                raise ValueError("render_frame_at_device: ref must be a uint8 CUDA tensor %s, got %s %s" % (shp, ref.dtype, tuple(ref.shape)))
            ref = ref.contiguous()
        return self._render(f, oh, ow, want_float, want_u8, ref, True)

    def psnr(self):
        per = np.zeros(self.cfg.number_of_frames, np.float64)
        mean = C.c_double(0)
        self._chk(self.lib.af_psnr(self.h, C.byref(mean), _ptr(per)))
        return float(mean.value), per

    # ---- layer decomposition (evaluate.py:24-200,300-438; include/atlasfit.h af_render_layers ...)
    LAYERS = ("uv1", "uv2", "alpha", "rgb1", "rgb2")
    _LAYER_TAIL = {"uv1": (2,), "uv2": (2,), "alpha": (), "rgb1": (3,), "rgb2": (3,)}

    def _layers_at_names(self, which, what):
        names = tuple(which)
        bad = [n for n in names if n not in self.LAYERS]
        if bad:
            raise ValueError("%s: unknown outputs %s (known: %s)" % (what, bad, ", ".join(self.LAYERS)))
        if not self.two_layer and ("uv2" in names or "rgb2" in names):
            if tuple(which) != self.LAYERS:
                raise ValueError("%s: uv2 / rgb2 need a two_layer handle" % what)
            names = tuple(n for n in names if n not in ("uv2", "rgb2"))      # the default set on a single-atlas handle: what it has
        return names

    def _layer_outputs(self, names, oh, ow, alpha_u8, on_device):
        """_render_outputs for the layer outputs `names` (and alpha_u8): (arrays, their pointers in the order of LAYERS, then alpha_u8's)."""
        spec = {n: (self._LAYER_TAIL[n], np.float32) for n in names}
        if alpha_u8:
            spec["alpha_u8"] = ((), np.uint8)
        out, p = _render_outputs(self, oh, ow, spec, on_device)
        return out, [p(k) for k in self.LAYERS + ("alpha_u8",)]

    def render_layers(self, f):
        """{"uv1", "uv2": (resy, resx, 2) raw mapping outputs, "alpha": (resy, resx), "rgb1", "rgb2": (resy, resx, 3) layer colours} of
        frame f (evaluate.py:302-337).  A single-atlas handle returns uv1, rgb1 and alpha == 1 (uv2 / rgb2 None)."""
        names = [n for n in self.LAYERS if self.two_layer or n not in ("uv2", "rgb2")]
        out, ptrs = self._layer_outputs(names, self.cfg.resy, self.cfg.resx, False, False)
        self._chk(self.lib.af_render_layers(self.h, int(f), *ptrs[:5]))
        return dict({"uv2": None, "rgb2": None}, **out)

    def render_layers_at(self, f, oh, ow, which=("uv1", "uv2", "alpha", "rgb1", "rgb2"), alpha_u8=False):
        """render_layers with the nets evaluated at the pixel centres of an (oh, ow) grid over the lattice (render_frame_at's geometry):
        {name: float32 array (oh, ow[, 2 | 3])} for the names in `which`, plus "alpha_u8" (oh, ow) uint8 = to_u8(alpha) with alpha_u8.
        (resy, resx) gives render_layers' arrays bit for bit.  A single-atlas handle has uv1, rgb1 and alpha == 1.  Forward-only; needs no
        uploaded video."""
        return self._render_layers_at(f, oh, ow, self._layers_at_names(which, "render_layers_at"), alpha_u8, False)

    def render_layers_at_device(self, f, oh, ow, which=("uv1", "uv2", "alpha", "rgb1", "rgb2"), alpha_u8=False):
        """render_layers_at without the host round trip: the same dict of torch CUDA tensors on the handle's device."""
        return self._render_layers_at(f, oh, ow, self._layers_at_names(which, "render_layers_at_device"), alpha_u8, True)

    def _render_layers_at(self, f, oh, ow, names, alpha_u8, on_device):
        out, ptrs = self._layer_outputs(names, oh, ow, alpha_u8, on_device)
        self._chk(self.lib.af_render_layers_at(self.h, int(f), int(oh), int(ow), *ptrs, int(on_device)))
        return out

    def edit_session(self, res, tex_fg=None, win_fg=None, tex_bg=None, win_bg=None, track_usage=False):
        """An EditSession: render_edit's propagation with the textures (uploaded once, here) and the usage masks resident on the device,
        at the lattice or any other size.  Arguments as render_edit's; track_usage: accumulate the texel usage masks on the device."""
        return EditSession(self, res, tex_fg, win_fg, tex_bg, win_bg, track_usage)

    def mapping_area(self, which):
        """get_mapping_area (evaluate.py:142-190): (maxx, minx, maxy, miny, edge) as float32; which = 0 foreground (mask > 0.5, a > 0.95),
        1 background (-a > -0.5).  An empty selection gives (-1, 1, -1, 1, -2)."""
        out = np.zeros(5, np.float32)
        self._chk(self.lib.af_mapping_area(self.h, int(which), _ptr(out)))
        return tuple(np.float32(v) for v in out)

    @staticmethod
    def area_window(area):
        """(minx, miny, edge) of a mapping_area result: the window texture and edit calls take (evaluate.py:248-257)."""
        return (np.float32(area[1]), np.float32(area[3]), np.float32(area[4]))

    def atlas_texture(self, res, window):
        """texture_orig of get_high_res_texture (evaluate.py:87-104): (res, res, 3) colours of the atlas on the window
        (minx, miny, edge) = torch.linspace(min, min + edge, res) along columns (x) and rows (y)."""
        out = np.empty((int(res), int(res), 3), np.float32)
        mx, my, e = (float(np.float32(v)) for v in window)
        self._chk(self.lib.af_render_atlas_texture(self.h, int(res), mx, my, e, _ptr(out)))
        return out

    def render_edit(self, f, res, tex_fg=None, win_fg=None, tex_bg=None, win_bg=None, use_fg=None, use_bg=None, outputs=("edit", "edit_fg", "edit_bg")):
        """Texture-edit propagation of frame f (evaluate.py:373-438): {name: (resy, resx, 3)} for the requested outputs among edit,
        edit_fg, edit_bg.  use_fg / use_bg: float32 (res, res) arrays the texel usage is accumulated into (in place; start from zeros).
        A layer without a window is skipped; a window without a texture gives usage only."""
        H, W = self.cfg.resy, self.cfg.resx
        tex = [None if t is None else _f32(t) for t in (tex_fg, tex_bg)]
        for t in tex:
            if t is not None and t.shape != (res, res, 3):
                raise ValueError("render_edit: textures must be (res, res, 3), got %s" % (t.shape,))
        win = [None if w is None else np.asarray(w, np.float32).reshape(3) for w in (win_fg, win_bg)]
        for u in (use_fg, use_bg):
            if u is not None and (u.dtype != np.float32 or u.shape != (res, res) or not u.flags.c_contiguous):
                raise ValueError("render_edit: use_fg / use_bg must be C-contiguous float32 (res, res)")
        out = {k: np.empty((H, W, 3), np.float32) for k in outputs}
        self._chk(self.lib.af_render_edit(self.h, int(f), int(res), _ptr(tex[0]), _ptr(win[0]), _ptr(tex[1]), _ptr(win[1]),
                                          _ptr(out.get("edit")), _ptr(out.get("edit_fg")), _ptr(out.get("edit_bg")), _ptr(use_fg), _ptr(use_bg)))
        return out

    def texture_masks(self, res, win_fg, win_bg):
        """(masks1, masks2) (res, res) float32 over all frames (evaluate.py:398-419): masks1 = max alpha over the texels each relevant fg
        pixel touches (the true maximum), masks2 = 1 on any bg use."""
        m1, m2 = np.zeros((res, res), np.float32), np.zeros((res, res), np.float32)
        for f in range(self.cfg.number_of_frames):
            self.render_edit(f, res, None, win_fg, None, win_bg, use_fg=m1, use_bg=m2, outputs=())
        return m1, m2

    # ---- per-pixel loss maps (evaluate.py:338-384 / :650-705; include/atlasfit.h af_render_loss_maps)
    LOSS_MAPS = ("rigidity_loss1", "rigidity_loss2", "flow_loss1", "flow_loss2", "flow_alpha_loss", "rgb_error", "rgb_residual")
    LOSS_MAPS_FG_BG = ("rigidity_loss2", "flow_loss2", "flow_alpha_loss")     # two_layer handles only

    def loss_maps(self, f, which=None):
        """Per-pixel loss maps of frame f, named after the reference's variables: rigidity_loss1/2, flow_loss1/2, flow_alpha_loss
        (resy, resx) and rgb_error (resy, resx), rgb_residual (resy, resx, 3), all float32.  `which`: the names to compute (default: all
        of this handle's path; a single-atlas handle has no rigidity_loss2 / flow_loss2 / flow_alpha_loss).  Only those are computed."""
        names = tuple(n for n in self.LOSS_MAPS if self.two_layer or n not in self.LOSS_MAPS_FG_BG) if which is None else tuple(which)
        bad = [n for n in names if n not in self.LOSS_MAPS]
        if bad:
            raise ValueError("unknown loss maps %s (known: %s)" % (bad, ", ".join(self.LOSS_MAPS)))
        H, W = self.cfg.resy, self.cfg.resx
        out = {n: np.empty((H, W, 3) if n == "rgb_residual" else (H, W), np.float32) for n in names}
        self._chk(self.lib.af_render_loss_maps(self.h, int(f), *[_ptr(out.get(n)) for n in self.LOSS_MAPS]))
        return out

    # ---- warping error of the whole clip (include/atlasfit.h af_warp_error)
    WARP_ERROR_WHICH = ("input", "reconstruction")

    def warp_error(self, which="input", align_corners=True):
        """(mean, per_pair): E_warp of the uploaded video ("input") or of af_render_frame's reconstruction ("reconstruction") over the
        F-1 consecutive pairs, with the uploaded flows; per_pair float64 (F-1,).  align_corners as warp_error_pair."""
        if which not in self.WARP_ERROR_WHICH:
            raise ValueError("which must be one of %s" % (self.WARP_ERROR_WHICH,))
        per = np.zeros(max(self.cfg.number_of_frames - 1, 1), np.float64)
        mean = C.c_double(0)
        self._chk(self.lib.af_warp_error(self.h, self.WARP_ERROR_WHICH.index(which), int(bool(align_corners)), _ptr(per), C.byref(mean)))
        return float(mean.value), per[:self.cfg.number_of_frames - 1]

    # ---- hooks
    def debug_forward(self, net, rows):
        rows = _f32(rows)
        assert rows.ndim == 2 and rows.shape[1] == 4
        out = np.empty_like(rows)
        self._chk(self.lib.af_debug_forward(self.h, net, _ptr(rows), rows.shape[0], _ptr(out)))
        return out

    def debug_tiles(self, net, which, layer, rows, tile0=0, ntiles=None):
        """Tensors the last training step left for the weight-gradient GEMMs (include/atlasfit.h af_debug_tiles): which = "acts" (plane `layer` =
        relu(Z_layer), (ntiles, 256, 32)), "dz" (dZ_layer), "masks" ((ntiles, 64, 4) uint32), "pe" ((ntiles, 64, 32)), "dz_last" / "x0" ((ntiles, 32, 32)),
        "out" / "dout" (the net's output rows and the gradient on them as the backward seed read it, row-major (ntiles, 32, 4)), "rows" (the net's
        input rows (x, y, t, 0) as the batch preparation wrote them, row-major (ntiles, 32, 4); the atlas net has none).
        `rows` = rows of that net's batch in the step (its planes are ceil(rows / 32) tiles apart)."""
        kinds = {"acts": (0, (256, 32)), "dz": (1, (256, 32)), "masks": (2, (64, 4)), "pe": (3, (64, 32)), "dz_last": (4, (32, 32)), "x0": (5, (32, 32)),
                 "out": (6, (32, 4)), "dout": (7, (32, 4)), "rows": (8, (32, 4))}
        code, shp = kinds[which]
        stride = (int(rows) + 31) // 32
        ntiles = stride - tile0 if ntiles is None else int(ntiles)
        out = np.empty((ntiles,) + shp, np.float32)
        self._chk(self.lib.af_debug_tiles(self.h, net, code, int(layer), stride, int(tile0), ntiles, _ptr(out)))
        return out.view(np.uint32) if which == "masks" else out

    def read_records(self, inds):
        """(n, 16) packed pixel records for pixel-frame indices `inds` (column numbers of get_tuples' table)."""
        inds = np.ascontiguousarray(inds, np.int64)
        out = np.empty((inds.size, 16), np.float32)
        self._chk(self.lib.af_debug_records(self.h, _ptr(inds), inds.size, _ptr(out)))
        return out

    def dw_clocks(self, enable=True):
        """(#CUs, 2) start / end s_memrealtime ticks (100 MHz) per workgroup of the most recent k_dw launch."""
        out = np.zeros((1024, 2), np.uint64)
        n = self.lib.af_debug_dw_clocks(self.h, int(enable), _ptr(out), 1024)
        if n < 0:
            self._chk(n)
        return out[:n]

    STEP_CLOCK_LAUNCHES = ("fwd_1", "fwd_2", "bwd_1", "bwd_2", "dw")

    def step_clocks(self, enable=True):
        """{launch: (#workgroups, 4) uint64 = s_memrealtime (100 MHz), s_memtime (shader clock) at workgroup start, then at its end} of
        the most recent training step for the five hot launches (include/atlasfit.h: af_debug_step_clocks); the first call enables the stamps."""
        out = np.zeros((5, 4096, 4), np.uint64)
        n = self.lib.af_debug_step_clocks(self.h, int(enable), _ptr(out), 4096)
        if n < 0:
            self._chk(n)
        return {name: out[i][out[i, :, 2] > 0] for i, name in enumerate(self.STEP_CLOCK_LAUNCHES)}

    def dw_schedule(self, which):
        """(#workgroups, 16, 4) int32 segments {shape, t0, t1, job} of k_dw's static schedule `which` (0: 9 segments, 1: 7)."""
        n = self.lib.af_debug_dw_schedule(self.h, int(which), None, 0)
        if n < 0:
            self._chk(n)
        out = np.zeros((n, 16, 4), np.int32)
        self.lib.af_debug_dw_schedule(self.h, int(which), _ptr(out), n)
        return out

    def set_dw_mode(self, mode):
        """k_dw arithmetic: 1 = bf16x6 (fp32-faithful; the default), 2 = bf16x3 (two bf16 per operand, three products: narrower than fp32, opt-in), 0 = fp32 MFMA."""
        self._chk(self.lib.af_set_dw_mode(self.h, int(mode)))
        if hasattr(self, "arithmetic"):
            self.arithmetic["dw_mode"] = int(mode)

    def set_dw_cost(self, row, seg_cost=0.0):
        """Another split-K partition of k_dw (af_debug_set_dw_cost): row = five tile costs (8x8, 8x2, 8x1, 1x8, 1x2), a sequence or the
        "a,b,c,d,e[,seg]" string of the sweep tools; None = the shipped row.  Same arithmetic, another summation order."""
        if row is None:
            self._chk(self.lib.af_debug_set_dw_cost(self.h, None, 0.0))
            return
        if isinstance(row, str):
            vals = [float(x) for x in row.split(",")]
            if len(vals) == 6:
                seg_cost = vals[5]
            row = vals[:5]
        if len(row) != 5:
            raise ValueError("set_dw_cost: five tile costs (8x8, 8x2, 8x1, 1x8, 1x2)")
        arr = (C.c_double * 5)(*[float(x) for x in row])
        self._chk(self.lib.af_debug_set_dw_cost(self.h, arr, float(seg_cost)))

    def set_mlp_mode(self, mode):
        """Hidden-layer products of the MLP chains: 3 = f16x3 on the fp16 matrix pipe (default since round 6), 1 = bf16x6 on the bf16 matrix pipe,
        0 = fp32 MFMA (cross-check), 2 = bf16x6 forward, three-product bf16 backward chain (experiment)."""
        self._chk(self.lib.af_set_mlp_mode(self.h, int(mode)))
        if hasattr(self, "arithmetic"):
            self.arithmetic["mlp_mode"] = int(mode)

    def set_debug(self, on=True):
        self._chk(self.lib.af_set_debug(self.h, int(on)))

    def last_grads(self, net):
        g = np.empty(self.param_count(net), np.float32)
        self._chk(self.lib.af_get_last_grads(self.h, net, _ptr(g), g.size))
        return g

    def set_timing(self, mask=0xFFFF, every=1):
        """HIP events around the launch classes in `mask`; `every` = P: only every P-th step of a train_steps call is timed (an event
        costs ~5 us in-stream)."""
        m = int(mask) if not isinstance(mask, bool) else (0xFFFF if mask else 0)
        if not 1 <= int(every) <= 255:          # the period travels in bits 16..23 of af_set_timing's argument: 256 would wrap to "every step"
            raise ValueError("set_timing: every must be 1..255, got %r" % (every,))
        self._chk(self.lib.af_set_timing(self.h, (m & 0xFFFF) | ((max(1, int(every)) & 0xFF) << 16)))

    def timing(self, reset=True):
        """{launch class: (milliseconds, launches, algorithmic FLOPs)} accumulated since the last reset."""
        ms = np.zeros(16, np.float64); cnt = np.zeros(16, np.int64); fl = np.zeros(16, np.float64)
        self._chk(self.lib.af_get_timing(self.h, _ptr(ms), _ptr(cnt), _ptr(fl), int(reset)))
        return {n: (float(m), int(c), float(f)) for n, m, c, f in zip(self.TIMING_NAMES, ms, cnt, fl)}

    def step_work(self, it):
        """(rows per net indexed by NET_*, fwd+bwd FLOPs) of one loop iteration."""
        rows, fl = (C.c_int64 * 4)(), C.c_double(0)
        self._chk(self.lib.af_step_work(self.h, int(it), C.byref(rows), C.byref(fl)))
        return [int(r) for r in rows], float(fl.value)

    def sync(self):
        self._chk(self.lib.af_sync(self.h))


class EditSession:
    """Texture-edit propagation of one AtlasFit with resident textures (include/atlasfit.h af_edit_create ...).  Made by
    AtlasFit.edit_session; a context manager.  The nets are the handle's at each call.  AtlasFit.close() closes its open sessions."""

    OUTPUTS = ("edit", "edit_fg", "edit_bg")

    def __init__(self, af, res, tex_fg=None, win_fg=None, tex_bg=None, win_bg=None, track_usage=False):
        self.af, self.lib, self.e = af, af.lib, None
        self.res = res = int(res)
        tex = [None if t is None else _f32(t) for t in (tex_fg, tex_bg)]
        for t in tex:
            if t is not None and t.shape != (res, res, 3):
                raise ValueError("edit_session: textures must be (res, res, 3), got %s" % (t.shape,))
        win = []
        for w in (win_fg, win_bg):
            w = None if w is None else np.asarray(w, np.float32)
            if w is not None and w.size != 3:
                raise ValueError("edit_session: a window is (minx, miny, edge), got shape %s" % (w.shape,))
            win.append(None if w is None else np.ascontiguousarray(w.reshape(3)))
        self.track_usage = bool(track_usage)
        e = C.c_void_p()
        af._chk(self.lib.af_edit_create(af.h, res, _ptr(tex[0]), _ptr(win[0]), _ptr(tex[1]), _ptr(win[1]), int(self.track_usage), C.byref(e)))
        self.e = e
        if not hasattr(af, "_sessions"):
            af._sessions = []
        af._sessions.append(self)

    def _open(self):
        if self.e is None:      # closed here, or by AtlasFit.close(): the state error the library gives for a session whose handle is gone
            raise AtlasFitError(AF_ESTATE, "EditSession: the session is closed")
        return self.e

    def _chk(self, rc):
        if rc != 0:      # a dead session (its handle destroyed) has no handle to ask: the library leaves that message with the calling thread
            raise AtlasFitError(rc, self.lib.af_last_error(self.af.h if self.af.h else None).decode())

    def _names(self, outputs, what):
        names = tuple(outputs)
        bad = [n for n in names if n not in self.OUTPUTS]
        if bad:
            raise ValueError("%s: unknown outputs %s (known: %s)" % (what, bad, ", ".join(self.OUTPUTS)))
        return names

    def _size(self, oh, ow):
        c = self.af.cfg
        return int(c.resy if oh is None else oh), int(c.resx if ow is None else ow)

    def frame(self, f, oh=None, ow=None, outputs=("edit",), u8=False):
        """{name: (oh, ow, 3) float32} for the names in `outputs` among edit, edit_fg, edit_bg, plus "edit_u8" (oh, ow, 3) uint8 =
        to_u8(edit) with u8.  Default size: the lattice, where the arrays are render_edit's bit for bit."""
        return self._frame(f, oh, ow, self._names(outputs, "EditSession.frame"), u8, False)

    def frame_device(self, f, oh=None, ow=None, outputs=("edit",), u8=False):
        """frame without the host round trip: the same dict of torch CUDA tensors on the handle's device."""
        return self._frame(f, oh, ow, self._names(outputs, "EditSession.frame_device"), u8, True)

    def _frame(self, f, oh, ow, names, u8, on_device):
        e = self._open()
        oh, ow = self._size(oh, ow)
        spec = {n: ((3,), np.float32) for n in names}
        if u8:
            spec["edit_u8"] = ((3,), np.uint8)
        out, p = _render_outputs(self.af, oh, ow, spec, on_device)
        self._chk(self.lib.af_edit_frame(e, int(f), oh, ow, *[p(k) for k in self.OUTPUTS + ("edit_u8",)], int(on_device)))
        return out

    def usage(self):
        """(use_fg, use_bg): the (res, res) float32 usage masks accumulated so far (texture_masks' definitions)."""
        e = self._open()
        u1, u2 = np.empty((self.res, self.res), np.float32), np.empty((self.res, self.res), np.float32)
        self._chk(self.lib.af_edit_usage(e, _ptr(u1), _ptr(u2)))
        return u1, u2

    def reset_usage(self):
        e = self._open()
        self._chk(self.lib.af_edit_reset_usage(e))

    def close(self):
        if self.e is not None:
            self.lib.af_edit_destroy(self.e)
            self.e = None
            if self in getattr(self.af, "_sessions", ()):
                self.af._sessions.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
