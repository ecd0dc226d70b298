#!/usr/bin/env python
"""Cost of the YUV4MPEG2 route on one MI355X (MEASUREMENTS.md Part Q).

    python tools/y4m_bench.py [--calls 20] [--pipeline 768x432[,1920x1080]] [--runs 3] [--out y4m_bench.json]

1. af_yuv_to_rgb and af_rgb_to_yuv (csrc/yuv.hip) with device pointers at 1920x1080 and 3840x2160, 420jpeg, BT.709, limited range: the
   host clock around the call (it is host-synchronous: launch, synchronise), median of --calls calls after a warm-up; beside it, in the
   same run, a device-to-device copy of the bytes the kernel moves (payload + image: torch's copy_ between two synchronisations) as the
   yardstick.  Effective GB/s = (payload bytes + image bytes) over the time: each kernel reads one and writes the other.
2. --pipeline: deflicker.py on the 80-frame synthetic clip of tools/pipeline_bench.py at each given size, the shipped config, --down 4,
   --seed 1: PNG in / PNG out (--frames_dir, final/output/%05d.png) against Y4M in / Y4M out (--video, --video_out, files), alternating,
   --runs fresh child processes each; the child's wall clock and the `seconds` of its record, median and spread.

The board's clocks as `rocm-smi --showclocks` reads them right after the timed calls go into the record.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shots_bench import _clocks, _median_ms  # noqa: E402


def kernel_rows(calls):
    import aiod_amd
    import y4m_ref
    rows = []
    gen = torch.Generator().manual_seed(0)
    layout, matrix, full = "420jpeg", "bt709", False
    for w, h in ((1920, 1080), (3840, 2160)):
        nyuv, nrgb = aiod_amd.y4m.frame_bytes(h, w, layout), h * w * 3
        payload = torch.randint(0, 256, (nyuv,), dtype=torch.uint8, generator=gen).cuda()
        img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).cuda()
        both = torch.empty(nyuv + nrgb, dtype=torch.uint8, device="cuda")
        half = torch.empty((nyuv + nrgb) // 2, dtype=torch.uint8, device="cuda")
        row = {"size": "%dx%d" % (w, h), "layout": layout, "calls": calls, "payload_bytes": nyuv, "image_bytes": nrgb}
        for name, fn in (("yuv_to_rgb", lambda: aiod_amd.yuv_to_rgb_device(payload, h, w, layout, matrix, full)),
                         ("rgb_to_yuv", lambda: aiod_amd.rgb_to_yuv_device(img, layout, matrix, full))):
            ms, lo, hi = _median_ms(fn, calls)
            row[name] = {"ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "GBps_read_plus_written": round((nyuv + nrgb) / ms / 1e6, 1)}
        cms, clo, chi = _median_ms(lambda: half.copy_(both[:half.numel()]), calls)      # reads and writes (nyuv + nrgb) / 2 each: the same traffic
        row["d2d_copy_same_traffic"] = {"ms": round(cms, 4), "ms_min_max": [round(clo, 4), round(chi, 4)], "GBps_read_plus_written": round(2 * half.numel() / cms / 1e6, 1)}
        # what was timed computes the right thing (a band of the frame: the whole-array restatement of a 4K frame takes seconds)
        hb = 64
        band = payload.cpu().numpy()
        y, cb, cr = y4m_ref.split(band, h, w, layout)
        small = np.concatenate([y[:hb].reshape(-1), cb[:hb // 2].reshape(-1), cr[:hb // 2].reshape(-1)])
        got = aiod_amd.yuv_to_rgb_device(torch.from_numpy(small).cuda(), hb, w, layout, matrix, full).cpu().numpy()
        assert np.array_equal(got, y4m_ref.yuv_to_rgb(small, hb, w, layout, matrix, full))
        sub = img[:hb].contiguous()
        assert np.array_equal(aiod_amd.rgb_to_yuv_device(sub, layout, matrix, full).cpu().numpy(), y4m_ref.rgb_to_yuv(sub.cpu().numpy(), layout, matrix, full))
        row["clocks_after"] = _clocks()
        rows.append(row)
    return rows


def _summary(vals):
    return {"median": round(statistics.median(vals), 3), "min": round(min(vals), 3), "max": round(max(vals), 3)}


def pipeline_rows(sizes, runs, timeout):
    import aiod_amd
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    out = {}
    for size in sizes:
        w, h = (int(v) for v in size.split("x"))
        d = tempfile.mkdtemp(prefix="af_y4m_")
        cfg_path = os.path.join(d, "config.json")
        with open(cfg_path, "w") as f:
            json.dump(dict(REFERENCE_CONFIG), f)
        paths = PB.write_weights(os.path.join(d, "weights"), PB.synthetic_weights())
        frames = PB.synthetic_clip(80, h, w, seed=1)
        PB.write_clip(os.path.join(d, "clip"), frames)
        matrix = aiod_amd.resolve_matrix("auto", h, w)
        with aiod_amd.Y4MWriter(os.path.join(d, "clip.y4m"), w, h, "25", "420jpeg", False) as wr:
            for fr in frames:
                wr.write(aiod_amd.rgb_to_yuv(fr, "420jpeg", matrix, False))
        samples = {"png": [], "y4m": []}
        for k in range(runs):
            for arm in ("png", "y4m"):                            # alternating: the spread beside the difference
                res = os.path.join(d, "res_%s_%d" % (arm, k))
                cmd = PB.in_process_command(os.path.join(d, "clip"), res, cfg_path, 4, 1, paths)
                if arm == "y4m":
                    i = cmd.index("--frames_dir")
                    cmd[i:i + 2] = ["--video", os.path.join(d, "clip.y4m"), "--video_out", os.path.join(d, "out_%d.y4m" % k)]
                wall = PB.child(cmd, d, timeout)
                with open(os.path.join(res, "deflicker.json")) as f:
                    rec = json.load(f)
                samples[arm].append({"wall_s": round(wall, 3), "seconds": rec["seconds"]})
        row = {"frames": 80, "runs": runs, "yuv_matrix": matrix, "bytes_in": {"png": sum(os.path.getsize(os.path.join(d, "clip", n)) for n in os.listdir(os.path.join(d, "clip"))),
                                                                                 "y4m": os.path.getsize(os.path.join(d, "clip.y4m"))}}
        for arm, ss in samples.items():
            row[arm] = {"wall_s": _summary([s["wall_s"] for s in ss]),
                        "seconds": {k: _summary([s["seconds"][k] for s in ss]) for k in ss[0]["seconds"]},
                        "outside_run_s": _summary([s["wall_s"] - s["seconds"]["total"] for s in ss]), "samples": ss}
        out[size] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pipeline", default=None, help="comma-separated WxH sizes of the 80-frame synthetic clip, e.g. 768x432,1920x1080")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing here can be timed without one")
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernel_rows(a.calls)}
    if a.pipeline:
        res["pipeline"] = pipeline_rows(a.pipeline.split(","), a.runs, a.timeout)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
