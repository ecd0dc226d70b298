"""Fixture of stage 2 (include/atlasfit.h: af_filter_*), computed by the REFERENCE's own modules on the CPU:
UNet from src/models/network_filter.py and TransformNet from src/models/network_local.py (both import torch only; the stage-2
script and src/models/utils.py import cv2 and are not imported).  The frame loop of src/neural_filter_and_refinement.py:89-121 is
restated below (`run_loop`).

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_stage2.py
        -> tests/golden/stage2.npz       (byte-identical on every run)

Weights (the real checkpoints are not public here): `synthetic_state_dicts()` fills both state_dicts in their own key order; key i
draws from torch.Generator().manual_seed(2023 + i): a weight of fan-in n is U(-b, b) with b = SCALE[key] * sqrt(6 / n) (He-uniform,
SCALE 1 unless listed), a bias is U(-0.05, 0.05); the InstanceNorm buffers keep their initial values.  The listed scales keep the
residual stack, the LSTM gates and the final tanh away from saturation (the fixture records every activation's rms).

Clip: F = 4 frames of 70 x 40 (w x h): padding on both axes (96 x 64, 13 columns left and right, 24 rows at the bottom).  The
content is a smooth moving pattern with a per-frame gain (the flicker), the stage-1 frame ("style") a steadier version of it, both
uint8 at the content's size.

Data:
  filter_keys, local_keys (str), filter_shapes, local_shapes (int64, rows padded with -1)  both state_dicts as the modules define them
  content, style (F, 40, 70, 3) uint8
  pred64_hi, final64_hi (F, 64, 96, 3) float32, *_lo float16    the fp64 twin: value = hi + lo * 2^-20 (float64, within 1e-10 relative)
  pred_err32, final_err32 (F, 2) float64     max and rms of |reference fp32 - fp64 twin| per frame
  act_names (str), act_rms (float64)         rms of every named activation of the fp64 twin on the last frame
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "stage2.npz")
H, W, NF = 40, 70, 4
LO_SCALE = 2.0 ** 20
SCALE = {"conv.weight": 0.5, "convlstm.Gates.weight": 0.5, "deconv3.conv2d.weight": 0.25}
SCALE.update({"ResBlocks.%d.conv2.conv2d.weight" % b: 0.3 for b in range(5)})


def load_reference_modules(ref):
    mods = []
    for name in ("network_filter", "network_local"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref, "src", "models", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods


def synthetic_state_dicts(filter_sd, local_sd):
    """The documented deterministic fill (module docstring), applied in place to two state_dicts (any dtype)."""
    for sd in (filter_sd, local_sd):
        for i, (k, v) in enumerate(sd.items()):
            if "norm_layer" in k:
                continue
            g = torch.Generator().manual_seed(2023 + i)
            u = torch.rand(v.shape, generator=g, dtype=torch.float64) * 2.0 - 1.0
            if k.endswith("weight"):
                fan_in = int(np.prod(v.shape[1:]))
                u = u * (SCALE.get(k, 1.0) * np.sqrt(6.0 / fan_in))
            else:
                u = u * 0.05
            v.copy_(u.to(v.dtype))


def pad_other(x):
    """InputPadder mode 'other' (src/models/utils.py:600-612) with replicate padding, NCHW."""
    ht, wd = x.shape[-2:]
    ph = (((ht // 32) + 1) * 32 - ht) % 32
    pw = (((wd // 32) + 1) * 32 - wd) % 32
    return F.pad(x, [pw // 2, pw - pw // 2, 0, ph], mode="replicate")


def run_loop(filter_net, local_net, contents, styles, dtype):
    """neural_filter_and_refinement.py:89-121 on NCHW tensors: returns [(pred, final)] padded, unclamped."""
    outs, o1, p1 = [], None, None
    with torch.no_grad():
        for t, (c, s) in enumerate(zip(contents, styles)):
            c, s = pad_other(c.to(dtype)), pad_other(s.to(dtype))
            pred = filter_net(torch.cat([c, s], dim=1))
            if t == 0:
                o1 = p1 = final = pred
            else:
                y, _ = local_net(torch.cat((pred, o1, pred, p1), dim=1), None)
                final = pred + y
                p1, o1 = pred, final
            outs.append((pred, final))
    return outs


def synthetic_clip(seed=2023):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    content, style = [], []
    for t in range(NF):
        base = np.stack([0.5 + 0.3 * np.sin(2 * np.pi * ((xx + 2.0 * t) / W * (1.5 + c) + yy / H * (1 + 0.5 * c)) + c)
                         for c in range(3)], axis=-1)
        gain = 1.0 + 0.2 * rng.standard_normal(3)
        noise = 0.02 * rng.standard_normal((H, W, 3))
        content.append(np.clip(base * gain + noise, 0, 1))
        style.append(np.clip(base * (1.0 + 0.03 * rng.standard_normal(3)), 0, 1))
    q = lambda a: np.round(np.stack(a) * 255).astype(np.uint8)     # noqa: E731
    return q(content), q(style)


def to_nchw(u8):
    """load_image (src/models/utils.py:583-598): uint8 / 255 in fp64, then the float tensor of the script (fp32)."""
    return [torch.from_numpy(a / 255.0).permute(2, 0, 1).unsqueeze(0).float() for a in u8]


def _shape_table(sd):
    rows = [list(v.shape) for v in sd.values()]
    n = max(len(r) for r in rows)
    return np.array([r + [-1] * (n - len(r)) for r in rows], np.int64)


def main():
    ref = os.environ.get("AF_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "src", "models", "network_local.py")):
        raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/network_local.py)")
    sys.dont_write_bytecode = True
    torch.set_num_threads(8)
    NFm, NLm = load_reference_modules(ref)
    fnet = NFm.UNet(in_channels=6, out_channels=3, init_features=32).eval()
    lnet = NLm.TransformNet(types.SimpleNamespace(nf=32, norm="IN", model="TransformNet", blocks=5), nc_in=12, nc_out=3).eval()
    fsd, lsd = fnet.state_dict(), lnet.state_dict()
    synthetic_state_dicts(fsd, lsd)
    content, style = synthetic_clip()
    cs, ss = to_nchw(content), to_nchw(style)
    out32 = run_loop(fnet, lnet, cs, ss, torch.float32)
    f64, l64 = fnet.double(), lnet.double()
    acts = {}
    hooks = []
    for name, mod in (("enc1", f64.encoder1), ("enc2", f64.encoder2), ("enc3", f64.encoder3), ("enc4", f64.encoder4),
                      ("bottleneck", f64.bottleneck), ("dec4", f64.decoder4), ("dec3", f64.decoder3), ("dec2", f64.decoder2),
                      ("dec1", f64.decoder1), ("E3", l64.conv3), ("RB", l64.ResBlocks[4])):
        hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: acts.__setitem__(name, o)))
    out64 = run_loop(f64, l64, cs, ss, torch.float64)
    for h in hooks:
        h.remove()
    res = {"filter_keys": np.array(list(fsd.keys())), "local_keys": np.array(list(lsd.keys())),
           "filter_shapes": _shape_table(fsd), "local_shapes": _shape_table(lsd), "content": content, "style": style}
    for which, idx in (("pred", 0), ("final", 1)):
        v64 = np.stack([o[idx][0].permute(1, 2, 0).numpy() for o in out64])
        v32 = np.stack([o[idx][0].permute(1, 2, 0).numpy() for o in out32]).astype(np.float64)
        hi = v64.astype(np.float32)
        lo = ((v64 - hi.astype(np.float64)) * LO_SCALE).astype(np.float16)
        assert (np.abs(hi + lo.astype(np.float64) / LO_SCALE - v64) <= 1e-10 * np.maximum(np.abs(v64), 1.0)).all()     # far below fp32 rounding
        res[which + "64_hi"], res[which + "64_lo"] = hi, lo
        d = np.abs(v32 - v64).reshape(NF, -1)
        res[which + "_err32"] = np.stack([d.max(1), np.sqrt((d ** 2).mean(1))], 1)
    res["act_names"] = np.array(sorted(acts))
    res["act_rms"] = np.array([float(acts[k].pow(2).mean().sqrt()) for k in sorted(acts)])
    pre_tanh = None
    for k, r in zip(res["act_names"], res["act_rms"]):
        print("rms %-10s %.4f" % (k, r))
    y = (out64[-1][1] - out64[-1][0])
    print("Y (tanh output) rms %.4f, max |Y| %.4f" % (float(y.pow(2).mean().sqrt()), float(y.abs().max())), pre_tanh or "")
    print("pred rms %.4f, err32 pred %s final %s" % (float(out64[-1][0].pow(2).mean().sqrt()), res["pred_err32"][:, 0], res["final_err32"][:, 0]))
    tmp = OUT + ".tmp"
    with zipfile.ZipFile(tmp, "w", compression=zipfile.ZIP_DEFLATED) as z:      # a fixed date in every entry: byte-identical reruns
        for name in sorted(res):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(res[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    os.replace(tmp, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
