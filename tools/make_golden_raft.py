"""Fixture of the native RAFT forward (include/atlasfit.h: af_raft_*), computed by the REFERENCE's own modules on the CPU:
RAFT("basic", small=False) from src/models/stage_1/core/raft.py in fp32 (on a CPU torch.cuda.amp.autocast is a no-op) and an fp64
twin of it.  raft_wrapper.py imports cv2 and is not imported; its compute_flow is InputPadder('sintel').pad + forward(iters=20,
test_mode=True) without unpad: `pad_sintel` + `ref_run`.

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_raft.py
        -> tests/golden/raft.npz       (byte-identical on every run)

The fp64 twin: the model is cast with .double(), and because RAFT.forward / CorrBlock cast with .float() inside, torch.Tensor.float
is replaced by torch.Tensor.double around the call (`as_double`).

Weights (raft-things.pth is not available here): `synthetic_state_dict(sd)` fills a state_dict in its own key order; key i draws
from torch.Generator().manual_seed(4100 + i): a conv weight of fan-in n is U(-b, b) with b = SCALE[key] * sqrt(6 / n), a conv bias
U(-0.05, 0.05); BatchNorm weight and running_var U(0.5, 1.5), BatchNorm bias and running_mean U(-0.2, 0.2); num_batches_tracked
keeps its value; cnet's downsample.1.* are the same tensors as norm3.* and both keys end with the former's draw.  The tests regenerate the weights from the recorded key list; none are stored.

Frames: 197 x 130 (w x h) -> padded 200 x 136, 1/8 grid 25 x 17, pyramid 12 x 8, 6 x 4, 3 x 2: padding on both axes and odd
sizes at every level.  Frame 2 is frame 1's smooth pattern shifted by a few pixels.

`raft_forward` is a pure-torch functional restatement of the same forward pass (any dtype, written from the description of the
layers in DESIGN.md 2.10); the tests hold it against this fixture and use it for the tensors too large to store.

Data:
  keys (str), shapes (int64, rows padded with -1)      the reference's state_dict
  im1, im2 (130, 197, 3) uint8
  up12_hi, up21_hi (136, 200, 2) float32, *_lo float16  the fp64 twin of the saved flow: value = hi + lo * 2^-20
  lo12_hi, lo21_hi (4, 17, 25, 2) float32, *_lo        the twin's 1/8 flow after ITERS = 1, 4, 12, 20 iterations
  names (str), err32 (len(names), 2), rms64 (len(names),)   max / rms of |reference fp32 - fp64 twin| and the twin's rms for:
      up12, up21, lo12_<k>, lo21_<k>, the named intermediates of iteration 1 of direction 1->2 (fmap1, fmap2, net0, inp, corr_l0..3,
      motion, net, delta, mask, corr_vol) and of one teacher-forced update step (step_net, step_delta: from the twin's state after
      11 iterations rounded to fp32, see `teacher_state`)
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "raft.npz")
H, W = 130, 197
ITERS = (1, 4, 12, 20)
STEP_FROM = 11
LO_SCALE = 2.0 ** 20
SCALE = {"update_block.flow_head.conv2.weight": 0.05, "cnet.conv2.weight": 0.1}


def synthetic_state_dict(sd):
    """The documented deterministic fill (module docstring), applied in place (any float dtype)."""
    for i, (k, v) in enumerate(sd.items()):
        if k.endswith("num_batches_tracked"):
            continue
        g = torch.Generator().manual_seed(4100 + i)
        u = torch.rand(v.shape, generator=g, dtype=torch.float64)
        if v.dim() == 4:
            u = (u * 2.0 - 1.0) * (SCALE.get(k, 1.0) * np.sqrt(6.0 / int(np.prod(v.shape[1:]))))
        elif ".norm" in k or "downsample.1" in k:
            u = u + 0.5 if (k.endswith("weight") or k.endswith("running_var")) else (u * 2.0 - 1.0) * 0.2
        else:
            u = (u * 2.0 - 1.0) * 0.05
        v.copy_(u.to(v.dtype))
        if "downsample.1." in k:        # the module's state_dict lists a strided block's norm3 twice: the later fill is the one it keeps
            sd[k.replace("downsample.1.", "norm3.")].copy_(v)


def synthetic_frames():
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def frame(dx, dy):
        x, y = xx - dx, yy - dy
        ch = [0.5 + 0.25 * np.sin(2 * np.pi * (x / 37.0 * (1 + 0.3 * c) + y / 53.0) + c) + 0.2 * np.cos(2 * np.pi * (y / 29.0 - x / 71.0 * (1 + c)))
              for c in range(3)]
        return np.round(np.clip(np.stack(ch, -1), 0, 1) * 255).astype(np.uint8)
    return frame(0.0, 0.0), frame(3.0, -2.0)


def to_nchw(u8, dtype=torch.float32):
    return torch.from_numpy(u8.astype(np.float64)).permute(2, 0, 1).unsqueeze(0).to(dtype)


def pad_sintel(x):
    """InputPadder mode 'sintel' (core/utils/utils.py): replicate, pad // 2 before and the rest after on both axes, to multiples of 8."""
    ht, wd = x.shape[-2:]
    ph = (((ht // 8) + 1) * 8 - ht) % 8
    pw = (((wd // 8) + 1) * 8 - wd) % 8
    return F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], mode="replicate")


# ---- functional restatement (NCHW, any dtype; sd without the DataParallel prefix) ------------------------------------------
def _encoder(sd, p, x, norm):
    def nrm(v, name):
        if norm == "instance":
            return F.instance_norm(v, eps=1e-5)
        return F.batch_norm(v, sd[p + name + ".running_mean"], sd[p + name + ".running_var"], sd[p + name + ".weight"], sd[p + name + ".bias"], False, 0.0, 1e-5)

    def conv(v, name, stride=1, pad=0):
        return F.conv2d(v, sd[p + name + ".weight"], sd[p + name + ".bias"], stride, pad)
    x = F.relu(nrm(conv(x, "conv1", 2, 3), "norm1"))
    for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
        for b in (0, 1):
            q = "%s.%d." % (layer, b)
            s = stride if b == 0 else 1
            y = F.relu(nrm(conv(x, q + "conv1", s, 1), q + "norm1"))
            y = F.relu(nrm(conv(y, q + "conv2", 1, 1), q + "norm2"))
            if s != 1:
                x = nrm(conv(x, q + "downsample.0", s, 0), q + "norm3")
            x = F.relu(x + y)
    return conv(x, "conv2")


def corr_volume(f1, f2):
    """(1, C, h, w) x 2 -> (h * w, h, w): all-pairs dot products / sqrt(C)."""
    _, c, h, w = f1.shape
    v = torch.matmul(f1.reshape(c, h * w).t(), f2.reshape(c, h * w))
    return (v / torch.sqrt(torch.tensor(float(c), dtype=f1.dtype))).reshape(h * w, h, w)


def corr_pyramid(vol):
    pyr = [vol[:, None]]
    for _ in range(3):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


def corr_lookup(pyr, coords, r=4):
    """coords (1, 2, h, w) (x, y) -> (1, 324, h, w); channel 81 l + 9 a + b samples level l at (x / 2^l + a - 4, y / 2^l + b - 4)."""
    _, _, h, w = coords.shape
    c = coords.permute(0, 2, 3, 1).reshape(h * w, 1, 1, 2)
    d = torch.linspace(-r, r, 2 * r + 1, dtype=coords.dtype, device=coords.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    out = []
    for l, vol in enumerate(pyr):
        hh, ww = vol.shape[-2:]
        p = c / 2 ** l + delta
        gx = 2 * p[..., 0:1] / (ww - 1) - 1
        gy = 2 * p[..., 1:2] / (hh - 1) - 1
        s = F.grid_sample(vol, torch.cat([gx, gy], -1), align_corners=True)
        out.append(s.view(1, h, w, -1))
    return torch.cat(out, -1).permute(0, 3, 1, 2).contiguous()


def update_step(sd, net, inp, corr, flow, want_mask=True):
    """BasicUpdateBlock: returns (net, mask or None, delta, motion)."""
    p = "update_block."

    def conv(v, name, pad):
        return F.conv2d(v, sd[p + name + ".weight"], sd[p + name + ".bias"], 1, pad)
    cor = F.relu(conv(F.relu(conv(corr, "encoder.convc1", 0)), "encoder.convc2", 1))
    flo = F.relu(conv(F.relu(conv(flow, "encoder.convf1", 3)), "encoder.convf2", 1))
    motion = torch.cat([F.relu(conv(torch.cat([cor, flo], 1), "encoder.conv", 1)), flow], 1)
    x = torch.cat([inp, motion], 1)
    for n, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([net, x], 1)
        z = torch.sigmoid(conv(hx, "gru.convz" + n, pad))
        r = torch.sigmoid(conv(hx, "gru.convr" + n, pad))
        q = torch.tanh(conv(torch.cat([r * net, x], 1), "gru.convq" + n, pad))
        net = (1 - z) * net + z * q
    delta = conv(F.relu(conv(net, "flow_head.conv1", 1)), "flow_head.conv2", 1)
    mask = 0.25 * conv(F.relu(conv(net, "mask.0", 1)), "mask.2", 0) if want_mask else None
    return net, mask, delta, motion


def upsample_flow(flow, mask):
    n, _, h, w = flow.shape
    m = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    u = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    u = torch.sum(m * u, dim=2).permute(0, 1, 4, 2, 5, 3)
    return u.reshape(n, 2, 8 * h, 8 * w)


def coords_grid(h, w, dtype):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([xx, yy], 0)[None].to(dtype)      # callers move it to their device


def raft_forward(sd, im1, im2, iters=20, acts=None, state=None, amp=False):
    """im1, im2 (1, 3, Hp, Wp) with values 0..255 in the dtype of sd.  Returns (flow_lo (1, 2, h, w), flow_up (1, 2, Hp, Wp)).
    acts (a dict) receives the named intermediates of the LAST iteration run; state = (net, coords1) replaces the initial state.
    amp: the encoders and the update block under fp16 autocast, as the reference runs them on a GPU (tools/raft_bench.py only)."""
    cast = lambda: torch.autocast(device_type=im1.device.type, dtype=torch.float16, enabled=amp)     # noqa: E731
    with torch.no_grad():
        a, b = 2 * (im1 / 255.0) - 1.0, 2 * (im2 / 255.0) - 1.0
        with cast():
            f1, f2 = _encoder(sd, "fnet.", a, "instance"), _encoder(sd, "fnet.", b, "instance")
            c = _encoder(sd, "cnet.", a, "batch")
            net, inp = torch.tanh(c[:, :128]), torch.relu(c[:, 128:])
        f1, f2 = f1.to(a.dtype), f2.to(a.dtype)
        vol = corr_volume(f1, f2)
        pyr = corr_pyramid(vol)
        h, w = f1.shape[-2:]
        coords0 = coords_grid(h, w, a.dtype).to(a.device)
        coords1 = coords0.clone()
        if acts is not None:
            acts.update(fmap1=f1, fmap2=f2, net0=net, inp=inp, corr_vol=vol[None])
        if state is not None:
            net, coords1 = state
        mask = None
        for it in range(iters):
            corr = corr_lookup(pyr, coords1)
            flow = coords1 - coords0
            with cast():
                net, mask, delta, motion = update_step(sd, net, inp, corr, flow, want_mask=(it == iters - 1))
            coords1 = coords1 + delta
            if acts is not None and it == iters - 1:
                acts.update(motion=motion, net=net, delta=delta, mask=mask, coords1=coords1)
                for l in range(4):
                    acts["corr_l%d" % l] = corr[:, 81 * l:81 * (l + 1)]
        return coords1 - coords0, upsample_flow(coords1 - coords0, mask.to(a.dtype))


# ---- the reference ------------------------------------------------------------------------------------------------------
class as_double:
    """torch.Tensor.float -> torch.Tensor.double while active: neutralises the .float() casts inside the reference's forward."""
    def __enter__(self):
        self.saved = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self.saved


def load_reference(ref):
    sys.path.insert(0, ref)
    from src.models.stage_1.core.raft import RAFT
    return RAFT(argparse.Namespace(small=False, mixed_precision=False)).eval()


def ref_run(model, im1, im2, iters, acts=None):
    """(flow_lo, flow_up) of the reference's forward in test mode; acts receives iteration `iters`' intermediates through hooks."""
    hooks, calls = [], []
    if acts is not None:
        hooks.append(model.fnet.register_forward_hook(lambda m, i, o: acts.update(fmap1=o[0], fmap2=o[1])))
        hooks.append(model.cnet.register_forward_hook(lambda m, i, o: acts.update(net0=torch.tanh(o[:, :128]), inp=torch.relu(o[:, 128:]))))
        hooks.append(model.update_block.encoder.register_forward_hook(lambda m, i, o: acts.update(motion=o)))

        def ub(m, i, o):
            calls.append(1)
            if len(calls) == iters:
                acts.update(net=o[0], mask=o[1], delta=o[2])
                for l in range(4):
                    acts["corr_l%d" % l] = i[2][:, 81 * l:81 * (l + 1)]
        hooks.append(model.update_block.register_forward_hook(ub))
    with torch.no_grad():
        lo, up = model(im1, im2, iters=iters, test_mode=True)
    for h in hooks:
        h.remove()
    return lo, up


def teacher_state(sd64, im1, im2):
    """The fp64 restatement's (net, coords1) after STEP_FROM iterations, rounded to fp32: the start of the teacher-forced step."""
    acts = {}
    raft_forward(sd64, im1.double(), im2.double(), iters=STEP_FROM, acts=acts)
    return acts["net"].float(), acts["coords1"].float()


def teacher_step(sd, im1, im2, state):
    """One update iteration from `state` in the dtype of sd: (net, delta)."""
    acts = {}
    dt = next(iter(sd.values())).dtype
    raft_forward(sd, im1.to(dt), im2.to(dt), iters=1, acts=acts, state=(state[0].to(dt), state[1].to(dt)))
    return acts["net"], acts["delta"]


def split_hi_lo(v64):
    hi = v64.astype(np.float32)
    lo = ((v64 - hi.astype(np.float64)) * LO_SCALE).astype(np.float16)
    assert (np.abs(hi + lo.astype(np.float64) / LO_SCALE - v64) <= 1e-10 * np.maximum(np.abs(v64), 1.0)).all()
    return hi, lo


def hwc(t):
    return t[0].permute(1, 2, 0).double().numpy()


def main():
    ref = os.environ.get("AF_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "src", "models", "stage_1", "core", "raft.py")):
        raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/stage_1/core/raft.py)")
    sys.dont_write_bytecode = True
    torch.set_num_threads(8)
    model = load_reference(ref)
    sd = model.state_dict()
    synthetic_state_dict(sd)
    u1, u2 = synthetic_frames()
    im = [pad_sintel(to_nchw(u)) for u in (u1, u2)]
    res = {"keys": np.array(list(sd.keys())), "im1": u1, "im2": u2}
    rows = [list(v.shape) for v in sd.values()]
    res["shapes"] = np.array([r + [-1] * (4 - len(r)) for r in rows], np.int64)
    names, err, rms = [], [], []

    def record(name, v32, v64):
        d = np.abs(v32 - v64).ravel()
        names.append(name); err.append([d.max(), np.sqrt((d ** 2).mean())]); rms.append(np.sqrt((v64 ** 2).mean()))
        print("%-12s rms %.4g  err32 max %.3g rms %.3g" % (name, rms[-1], err[-1][0], err[-1][1]))

    out32 = {}
    acts32 = {}
    for d, (a, b) in (("12", (0, 1)), ("21", (1, 0))):
        for k in ITERS:
            out32[d, k] = ref_run(model, im[a], im[b], k, acts32 if (d == "12" and k == 1) else None)
    vol32 = corr_volume(acts32["fmap1"], acts32["fmap2"])[None]
    sd32 = {k: v.clone() for k, v in sd.items()}
    st = None
    model.double()
    sd64 = model.state_dict()
    acts64 = {}
    with as_double():
        for d, (a, b) in (("12", (0, 1)), ("21", (1, 0))):
            los = []
            for k in ITERS:
                lo, up = ref_run(model, im[a].double(), im[b].double(), k, acts64 if (d == "12" and k == 1) else None)
                assert lo.dtype == torch.float64 and up.dtype == torch.float64
                los.append(hwc(lo))
                record("lo%s_%d" % (d, k), hwc(out32[d, k][0]), los[-1])
            record("up" + d, hwc(out32[d, 20][1]), hwc(up))
            res["up%s_hi" % d], res["up%s_lo" % d] = split_hi_lo(hwc(up))
            res["lo%s_hi" % d], res["lo%s_lo" % d] = split_hi_lo(np.stack(los))
    acts32["corr_vol"], acts64["corr_vol"] = vol32, corr_volume(acts64["fmap1"], acts64["fmap2"])[None]
    for n in ("fmap1", "fmap2", "net0", "inp", "corr_vol", "corr_l0", "corr_l1", "corr_l2", "corr_l3", "motion", "net", "delta", "mask"):
        assert acts64[n].dtype == torch.float64 and acts32[n].dtype == torch.float32
        record(n, hwc(acts32[n]), hwc(acts64[n]))
    # the restatement against the reference (fp64) and the teacher-forced step
    chk = {}
    lo_r, up_r = raft_forward(sd64, im[0].double(), im[1].double(), iters=20, acts=chk)
    print("restatement vs twin: up12 max |diff| %.3g" % np.abs(hwc(up_r) - (res["up12_hi"] + res["up12_lo"].astype(np.float64) / LO_SCALE)).max())
    st = teacher_state(sd64, im[0], im[1])
    n32, d32 = teacher_step(sd32, im[0], im[1], st)
    n64, d64 = teacher_step(sd64, im[0], im[1], st)
    record("step_net", hwc(n32), hwc(n64))
    record("step_delta", hwc(d32), hwc(d64))
    res["names"], res["err32"], res["rms64"] = np.array(names), np.array(err, np.float64), np.array(rms, np.float64)
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
