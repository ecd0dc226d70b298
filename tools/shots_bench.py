#!/usr/bin/env python
"""Cost of the cut detector on one MI355X (MEASUREMENTS.md Part P).

    python tools/shots_bench.py [--calls 20] [--block 8] [--pipeline] [--out shots_bench.json]

1. af_luma_grid (csrc/shots.hip) with device input at 1920x1080 and 3840x2160, 16 x 16 cells: the host clock around the call (it is
   host-synchronous: launch, synchronise, partial sums copied back and added), median of --calls calls after a warm-up, for one frame
   per call (what Deflicker.run does) and for a contiguous block of --block frames per call; beside it, in the same run, a
   device-to-device copy of the same bytes (torch's copy_ between two synchronisations) as the yardstick.  Effective GB/s = the bytes of
   the frames over the time: the kernel reads every byte once and writes next to nothing, the copy reads and writes them.
2. --pipeline: deflicker.py on the 80-frame 768x432 synthetic clip of tools/pipeline_bench.py, the shipped config, --down 4, --seed 1,
   once with --cuts auto and once with --cuts none, each a fresh child process; the `seconds` of both records.

The board's clocks as `rocm-smi --showclocks` reads them right after the timed calls go into the record.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _median_ms(fn, calls, warm=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def _clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
        return [ln.strip() for ln in r.splitlines() if "sclk" in ln or "mclk" in ln][:16]
    except Exception as e:      # the figure is a note beside the timings, not one of them
        return ["not read: %s" % e]


def kernel_rows(calls, block):
    import aiod_amd
    rows = []
    gen = torch.Generator().manual_seed(0)
    for w, h in ((1920, 1080), (3840, 2160)):
        clip = torch.randint(0, 256, (block, h, w, 3), dtype=torch.uint8, generator=gen).cuda()
        dst = torch.empty_like(clip)
        nbytes = h * w * 3
        row = {"size": "%dx%d" % (w, h), "grid": "16x16", "calls": calls, "bytes_per_frame": nbytes}
        for name, src, d, n in (("one_frame", clip[0], dst[0], 1), ("block", clip, dst, block)):
            ms, lo, hi = _median_ms(lambda: aiod_amd.luma_grids(src[None] if src.dim() == 3 else src), calls)
            cms, clo, chi = _median_ms(lambda: d.copy_(src), calls)
            row[name] = {"frames_per_call": n, "luma_ms_per_frame": round(ms / n, 4), "luma_ms_min_max_per_call": [round(lo, 4), round(hi, 4)],
                         "luma_GBps": round(n * nbytes / ms / 1e6, 1), "d2d_copy_ms_per_frame": round(cms / n, 4),
                         "d2d_copy_ms_min_max_per_call": [round(clo, 4), round(chi, 4)], "d2d_copy_GBps_of_frame_bytes": round(n * nbytes / cms / 1e6, 1)}
        sums, counts = aiod_amd.luma_grids(clip[:1])
        ref = (clip[0].cpu().numpy().astype(np.int64) * np.array([77, 150, 29])).sum()
        assert int(sums.sum()) == int(ref) and int(counts.sum()) == h * w      # what was timed computes the right thing
        row["clocks_after"] = _clocks()
        rows.append(row)
    return rows


def pipeline_rows(timeout):
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tempfile.mkdtemp(prefix="af_shots_")
    cfg_path = os.path.join(d, "config.json")
    with open(cfg_path, "w") as f:
        json.dump(dict(REFERENCE_CONFIG), f)
    paths = PB.write_weights(os.path.join(d, "weights"), PB.synthetic_weights())
    PB.write_clip(os.path.join(d, "clip"), PB.synthetic_clip(80, 432, 768, seed=1))
    out = {}
    for arm in ("auto", "none", "auto again", "none again"):      # alternating: the spread beside the difference
        res = os.path.join(d, "res_" + arm.replace(" ", "_"))
        wall = PB.child(PB.in_process_command(os.path.join(d, "clip"), res, cfg_path, 4, 1, paths, extra=["--cuts", arm.split()[0]]), d, timeout)
        with open(os.path.join(res, "deflicker.json")) as f:
            rec = json.load(f)
        out[arm] = {"wall_s": round(wall, 3), "seconds": rec["seconds"], "shots": rec["shots"],
                    "cut_scores_min": min(rec["cut_scores"]) if rec["cut_scores"] else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing here can be timed without one")
    res = {"device": torch.cuda.get_device_name(0), "luma_grid": kernel_rows(a.calls, a.block)}
    if a.pipeline:
        res["pipeline_80x768x432"] = pipeline_rows(a.timeout)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
