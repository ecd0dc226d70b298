#!/usr/bin/env python
"""Cost of one mask propagation step on one MI355X (MEASUREMENTS.md Part U).

    python tools/maskprop_bench.py [--calls 20] [--out maskprop_bench.json]

af_mask_step (csrc/maskprop.hip) with device pointers at 768x432 and 1920x1080 (the stage-1 size of a 4x-downsampled 4K clip and a
full-HD plane): the host clock around the call (it is host-synchronous: launch, synchronise), median of --calls calls after a warm-up;
beside it, in the same run, a device-to-device copy of the same byte count (torch's copy_ between two synchronisations).  The step
reads two planes and two flows and writes two planes: 8 fp32 planes of traffic, so the copy moves 4 planes to 4 planes.  The flows are
a smooth field of about a pixel with noise whose round trips close: nearly every pixel takes the gather branch, the dearer one (the
pixels that leave the frame are held; their share is in the record); the result of the timed call is checked against the numpy
restatement (tests/maskprop_ref.py).

The step is off the pipeline's critical path (at most 2 (n - 1) launches per clip): the figure is a record and asserts nothing about
speed.  The board's clocks as `rocm-smi --showclocks` reads them right after the timed calls go into the record.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shots_bench import _clocks, _median_ms  # noqa: E402


def rows(calls):
    import aiod_amd
    import maskprop_ref as R
    lib = aiod_amd.load_library()
    out = []
    rng = np.random.default_rng(0)
    for w, h in ((768, 432), (1920, 1080)):
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        f = np.stack([1.2 + 0.5 * np.sin(ys / 40.0), -0.7 + 0.4 * np.cos(xs / 55.0)], -1)
        f_ts = (f + rng.uniform(-0.3, 0.3, f.shape)).astype(np.float32)
        f_st = (-f + rng.uniform(-0.5, 0.5, f.shape)).astype(np.float32)
        m_s, c_s = rng.random((h, w)).astype(np.float32), rng.random((h, w)).astype(np.float32)
        dev = [torch.from_numpy(a).cuda() for a in (m_s, c_s, f_ts, f_st)]
        m_t, c_t = torch.empty((h, w), device="cuda"), torch.empty((h, w), device="cuda")
        ptr = [C.c_void_p(t.data_ptr()) for t in dev + [m_t, c_t]]

        def step():
            rc = lib.af_mask_step(0, ptr[0], ptr[1], ptr[2], ptr[3], h, w, 1.0, ptr[4], ptr[5], 1)
            assert rc == 0, lib.af_last_error(None).decode()

        nbytes = 8 * h * w * 4
        src, dst = torch.empty(nbytes // 8, device="cuda"), torch.empty(nbytes // 8, device="cuda")      # 4 planes each way
        ms, lo, hi = _median_ms(step, calls)
        cms, clo, chi = _median_ms(lambda: dst.copy_(src), calls)
        want_m, want_c = R.step(m_s, c_s, f_ts, f_st)
        assert np.array_equal(m_t.cpu().numpy(), want_m) and np.array_equal(c_t.cpu().numpy(), want_c)
        out.append({"size": "%dx%d" % (w, h), "calls": calls, "bytes_read_plus_written": nbytes, "held_fraction": round(float((want_c == 0).mean()), 3),
                    "mask_step": {"ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "GBps_read_plus_written": round(nbytes / ms / 1e6, 1)},
                    "d2d_copy_same_bytes": {"ms": round(cms, 4), "ms_min_max": [round(clo, 4), round(chi, 4)], "GBps_read_plus_written": round(nbytes / cms / 1e6, 1)},
                    "clocks_after": _clocks()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing here can be timed without one")
    res = {"device": torch.cuda.get_device_name(0), "kernels": rows(a.calls)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
