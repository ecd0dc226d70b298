"""The error level of the REFERENCE's own stage-2 nets under fp16 autocast, for stage 2's precision mode "fp16" (DESIGN.md 2.9): the
reference's UNet and TransformNet modules (loaded as tools/make_golden_stage2.py loads them) run the frame loop on the CPU under
torch.autocast("cpu", dtype=torch.float16), on the clip and synthetic weights of tools/make_golden_stage2.py, against the fp64 twin
stored in tests/golden/stage2.npz and, for the activations, the same modules in fp64.

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_stage2_amp.py
        -> tests/golden/stage2_amp.npz

Data (a few kilobytes; no tensors: the twins come from stage2.npz and the fp64 modules):
  names (str), err16 (len(names), 2)   max / rms of |reference under fp16 autocast - fp64 twin| for pred_<t>, final_<t> (t = frame
      0..3) and, on the last frame, enc1..enc4, bottleneck, dec4..dec1, E3, RB
  torch_version (str)                  the torch that wrote the file (CPU half kernels differ between versions)
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_stage2 as G  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "stage2_amp.npz")
ACTS = ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec4", "dec3", "dec2", "dec1", "E3", "RB")


def hwc(t):
    return t[0].permute(1, 2, 0).double().numpy()


def main():
    ref = os.environ.get("AF_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "src", "models", "network_local.py")):
        raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/network_local.py)")
    sys.dont_write_bytecode = True
    torch.set_num_threads(8)
    g = np.load(os.path.join(G.ROOT, "tests", "golden", "stage2.npz"))
    twin = {w: g[w + "64_hi"].astype(np.float64) + g[w + "64_lo"].astype(np.float64) / G.LO_SCALE for w in ("pred", "final")}
    NFm, NLm = G.load_reference_modules(ref)
    fnet = NFm.UNet(in_channels=6, out_channels=3, init_features=32).eval()
    lnet = NLm.TransformNet(types.SimpleNamespace(nf=32, norm="IN", model="TransformNet", blocks=5), nc_in=12, nc_out=3).eval()
    G.synthetic_state_dicts(fnet.state_dict(), lnet.state_dict())
    content, style = G.synthetic_clip()
    assert np.array_equal(content, g["content"]) and np.array_equal(style, g["style"])
    cs, ss = G.to_nchw(content), G.to_nchw(style)
    acts = {}
    for name, mod in (("enc1", fnet.encoder1), ("enc2", fnet.encoder2), ("enc3", fnet.encoder3), ("enc4", fnet.encoder4),
                      ("bottleneck", fnet.bottleneck), ("dec4", fnet.decoder4), ("dec3", fnet.decoder3), ("dec2", fnet.decoder2),
                      ("dec1", fnet.decoder1), ("E3", lnet.conv3), ("RB", lnet.ResBlocks[4])):
        mod.register_forward_hook(lambda m, i, o, name=name: acts.__setitem__(name, o))
    with torch.autocast("cpu", dtype=torch.float16):
        out16 = G.run_loop(fnet, lnet, cs, ss, torch.float32)
    acts16 = dict(acts)
    if not all(t.dtype == torch.float16 for o in out16 for t in o) or not all(acts16[n].dtype == torch.float16 for n in ACTS):
        raise SystemExit("the autocast run did not produce fp16 tensors: nothing written")
    out64 = G.run_loop(fnet.double(), lnet.double(), cs, ss, torch.float64)
    acts64 = dict(acts)
    err = {}

    def record(name, v16, v64):
        d = np.abs(v16 - v64).ravel()
        err[name] = [d.max(), np.sqrt((d ** 2).mean())]
        print("%-12s err16 max %.3g rms %.3g" % (name, err[name][0], err[name][1]))

    for t in range(G.NF):
        for idx, w in enumerate(("pred", "final")):
            assert np.abs(hwc(out64[t][idx]) - twin[w][t]).max() < 1e-9      # the fp64 modules are the stored twin
            record("%s_%d" % (w, t), hwc(out16[t][idx]), twin[w][t])
    for n in ACTS:
        record(n, hwc(acts16[n]), hwc(acts64[n]))
    if not (5e-4 < err["pred_%d" % (G.NF - 1)][0] < 2e-2):
        raise SystemExit("pred err16 %s is not near 3e-3: the autocast did not take" % (err["pred_%d" % (G.NF - 1)],))
    names = list(err)
    res = {"names": np.array(names), "err16": np.array([err[n] for n in names], np.float64), "torch_version": np.array(torch.__version__)}
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
