"""The error level of the REFERENCE's own RAFT under fp16 autocast, for the native path's precision mode "fp16" (DESIGN.md 2.10):
the reference's modules (src/models/stage_1/core/raft.py, mixed_precision=True as raft_wrapper.py builds them) run on the CPU with
the module-level name `autocast` of core/raft.py rebound to torch.autocast("cpu", dtype=torch.float16), on the frames and synthetic
weights of tools/make_golden_raft.py, against the fp64 twin stored in tests/golden/raft.npz and the fp64 restatement.

    AF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_raft_amp.py
        -> tests/golden/raft_amp.npz

Data (a few kilobytes; no tensors: the twins come from raft.npz and make_golden_raft.raft_forward in fp64):
  names (str), err16 (len(names), 2)   max / rms of |reference under fp16 autocast - fp64 twin| for raft.npz's names: up12, up21,
      lo12_<k>, lo21_<k> (k = 1, 4, 12, 20 iterations), the intermediates of iteration 1 of direction 1->2 and the teacher-forced
      step (step_net, step_delta: make_golden_raft.update_step under the same autocast, from the twin's state after 11 iterations
      rounded to fp16, against the fp64 step from that rounded state)
  torch_version (str)                  the torch that wrote the file (CPU half kernels differ between versions)
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_raft as G  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "raft_amp.npz")


def cpu_autocast(enabled=True):
    return torch.autocast("cpu", dtype=torch.float16, enabled=enabled)


def load_reference_amp(ref):
    model = G.load_reference(ref)
    import src.models.stage_1.core.raft as core_raft
    core_raft.autocast = cpu_autocast         # torch.cuda.amp.autocast is a no-op on a CPU
    model.args.mixed_precision = True
    return model


def main():
    ref = os.environ.get("AF_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "src", "models", "stage_1", "core", "raft.py")):
        raise SystemExit("set AF_REFERENCE to a checkout of the reference repository (the directory holding src/models/stage_1/core/raft.py)")
    sys.dont_write_bytecode = True
    torch.set_num_threads(8)
    g = dict(np.load(os.path.join(G.ROOT, "tests", "golden", "raft.npz")))
    twin = {k: g[k + "_hi"].astype(np.float64) + g[k + "_lo"].astype(np.float64) / G.LO_SCALE for k in ("up12", "up21", "lo12", "lo21")}
    model = load_reference_amp(ref)
    sd = model.state_dict()
    G.synthetic_state_dict(sd)
    assert [str(k) for k in g["keys"]] == list(sd.keys())
    u1, u2 = G.synthetic_frames()
    assert np.array_equal(u1, g["im1"]) and np.array_equal(u2, g["im2"])
    im = [G.pad_sintel(G.to_nchw(u)) for u in (u1, u2)]
    err = {}

    def record(name, v16, v64):
        d = np.abs(v16 - v64).ravel()
        err[name] = [d.max(), np.sqrt((d ** 2).mean())]
        print("%-12s err16 max %.3g rms %.3g" % (name, err[name][0], err[name][1]))

    acts16 = {}
    for d, (a, b) in (("12", (0, 1)), ("21", (1, 0))):
        for i, k in enumerate(G.ITERS):
            lo, up = G.ref_run(model, im[a], im[b], k, acts16 if (d == "12" and k == 1) else None)
            record("lo%s_%d" % (d, k), G.hwc(lo), twin["lo" + d][i])
            if k == 20:
                record("up" + d, G.hwc(up), twin["up" + d])
    assert acts16["fmap1"].dtype == torch.float16, "the autocast rebinding did not take"
    if not (0.015 < err["up12"][0] < 0.06 and 0.004 < err["up12"][1] < 0.016):
        raise SystemExit("up12 err16 %s is not near max 3.0e-2, rms 7.8e-3: the autocast rebinding did not take" % (err["up12"],))
    sd32 = {k: v.clone() for k, v in sd.items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    acts64 = {}
    G.raft_forward(sd64, im[0].double(), im[1].double(), iters=1, acts=acts64)
    acts16["corr_vol"] = G.corr_volume(acts16["fmap1"].float(), acts16["fmap2"].float())[None]
    for n in ("fmap1", "fmap2", "net0", "inp", "corr_vol", "corr_l0", "corr_l1", "corr_l2", "corr_l3", "motion", "net", "delta", "mask"):
        record(n, G.hwc(acts16[n]), G.hwc(acts64[n]))
    st = G.teacher_state(sd64, im[0], im[1])
    st = (st[0].half().float(), st[1])
    s16 = {}
    G.raft_forward(sd32, im[0], im[1], iters=1, acts=s16, state=st, amp=True)
    n64, d64 = G.teacher_step(sd64, im[0], im[1], st)
    record("step_net", G.hwc(s16["net"]), G.hwc(n64))
    record("step_delta", G.hwc(s16["delta"]), G.hwc(d64))
    names = [str(n) for n in g["names"]]
    assert sorted(names) == sorted(err), sorted(set(names) ^ set(err))
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
