#!/usr/bin/env python
"""Cost of the deep-video route on one MI355X (MEASUREMENTS.md Part Z).

    python tools/deep_video_bench.py [--calls 20] [--pipeline 1920x1080] [--runs 3] [--out deep_video_bench.json]

1. af_yuv_to_rgb16, af_rgb_to_yuv16 (csrc/yuv16.hip; 420jpeg, BT.709, limited range, 10 bits), af_depth_reduce and af_guided_apply16
   (csrc/guided.hip; planes of the frame's own size, the deep route's common case) with device pointers at 1920x1080 and 3840x2160: the
   host clock around the wrapper call (host-synchronous: launch, synchronise), median of --calls calls after a warm-up; beside each, in
   the same run, a device-to-device copy that moves the same number of bytes (torch's copy_ of half the kernel's traffic, which reads and
   writes that much each).
2. --pipeline: deflicker.py on the 80-frame synthetic clip of tools/pipeline_bench.py at each given size, the shipped config, --down 4,
   --seed 1: the clip as 8-bit Y4M in and out on the default route (--video, --video_out: the parent's) against the clip as 10-bit Y4M
   (4 * frame + seeded noise in 0..3) in and out with --video_depth keep, alternating, --runs fresh child processes each; the child's wall
   clock and the `seconds` of its record, median and spread.

The board's clocks as `rocm-smi --showclocks` reads them right after the timed calls go into the record.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shots_bench import _clocks, _median_ms  # noqa: E402
from y4m_bench import _summary  # noqa: E402

BITS = 10


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _host16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _timed(fn, nbytes, calls):
    """The call and a device-to-device copy of the same traffic, in the same run."""
    ms, lo, hi = _median_ms(fn, calls)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cms, clo, chi = _median_ms(lambda: dst.copy_(src), calls)
    return {"bytes_read_plus_written": nbytes, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "GBps": round(nbytes / ms / 1e6, 1),
            "d2d_copy_ms": round(cms, 4), "d2d_copy_ms_min_max": [round(clo, 4), round(chi, 4)], "ratio_to_copy": round(ms / cms, 2)}


def kernel_rows(calls):
    import aiod_amd
    import depth_transfer_ref
    import y4m16_ref
    rows = []
    rng = np.random.default_rng(0)
    layout, matrix, full = "420jpeg", "bt709", False
    for w, h in ((1920, 1080), (3840, 2160)):
        nyuv, nrgb = aiod_amd.y4m.frame_bytes(h, w, layout), h * w * 3                  # samples
        payload = _dev16(rng.integers(0, 1 << BITS, nyuv).astype(np.uint16))
        img = _dev16(rng.integers(0, 1 << BITS, (h, w, 3)).astype(np.uint16))
        a = torch.from_numpy(rng.uniform(-0.2, 0.2, (h, w, 3)).astype(np.float32)).cuda()
        b = torch.from_numpy(rng.uniform(-20, 20, (h, w, 3)).astype(np.float32)).cuda()
        row = {"size": "%dx%d" % (w, h), "layout": layout, "bits": BITS, "calls": calls}
        row["yuv_to_rgb16"] = _timed(lambda: aiod_amd.yuv_to_rgb16_device(payload, h, w, layout, matrix, full, BITS), 2 * (nyuv + nrgb), calls)
        row["rgb16_to_yuv"] = _timed(lambda: aiod_amd.rgb16_to_yuv_device(img, layout, matrix, full, BITS), 2 * (nyuv + nrgb), calls)
        row["depth_reduce"] = _timed(lambda: aiod_amd.reduce_depth_device(img, BITS), 3 * nrgb, calls)
        row["guided_apply16"] = _timed(lambda: aiod_amd.guided_apply16_device(img, BITS, a, b), (2 + 2 + 8) * nrgb, calls)      # frame in, frame out, two fp32 planes in
        # what was timed computes the right thing (a band of the frame: the whole-array restatements of a 4K frame take seconds)
        hb = 64
        y, cb, cr = (x.astype(np.uint16) for x in y4m16_ref.split(_host16(payload), h, w, layout, BITS))
        small = np.concatenate([y[:hb].reshape(-1), cb[:hb // 2].reshape(-1), cr[:hb // 2].reshape(-1)])
        assert np.array_equal(_host16(aiod_amd.yuv_to_rgb16_device(_dev16(small), hb, w, layout, matrix, full, BITS)), y4m16_ref.yuv_to_rgb(small, hb, w, layout, matrix, full, BITS))
        sub = _host16(img)[:hb]
        assert np.array_equal(_host16(aiod_amd.rgb16_to_yuv_device(_dev16(sub), layout, matrix, full, BITS)), y4m16_ref.rgb_to_yuv(sub, layout, matrix, full, BITS))
        assert np.array_equal(aiod_amd.reduce_depth_device(_dev16(sub), BITS).cpu().numpy(), y4m16_ref.reduce_depth(sub, BITS))
        pa, pb = a[:hb].contiguous(), b[:hb].contiguous()
        assert np.array_equal(_host16(aiod_amd.guided_apply16_device(_dev16(sub), BITS, pa, pb)), depth_transfer_ref.apply16(sub, BITS, pa.cpu().numpy(), pb.cpu().numpy()))
        row["clocks_after"] = _clocks()
        rows.append(row)
    return rows


def pipeline_rows(sizes, runs, timeout):
    import aiod_amd
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    out = {}
    for size in sizes:
        w, h = (int(v) for v in size.split("x"))
        d = tempfile.mkdtemp(prefix="af_deep_")
        cfg_path = os.path.join(d, "config.json")
        with open(cfg_path, "w") as f:
            json.dump(dict(REFERENCE_CONFIG), f)
        paths = PB.write_weights(os.path.join(d, "weights"), PB.synthetic_weights())
        frames = PB.synthetic_clip(80, h, w, seed=1)
        matrix = aiod_amd.resolve_matrix("auto", h, w)
        rng = np.random.default_rng(2)
        with aiod_amd.Y4MWriter(os.path.join(d, "clip8.y4m"), w, h, "25", "420jpeg", False) as w8, \
                aiod_amd.Y4MWriter(os.path.join(d, "clip10.y4m"), w, h, "25", "420jpeg", False, bits=BITS) as w10:
            for fr in frames:
                w8.write(aiod_amd.rgb_to_yuv(fr, "420jpeg", matrix, False))
                deep = (4 * fr.astype(np.uint16) + rng.integers(0, 4, fr.shape).astype(np.uint16)).astype(np.uint16)
                w10.write(aiod_amd.rgb16_to_yuv(deep, "420jpeg", matrix, False, BITS))
        arms = {"y4m_8bit": ["--video", os.path.join(d, "clip8.y4m")], "y4m_10bit_keep": ["--video", os.path.join(d, "clip10.y4m"), "--video_depth", "keep"]}
        samples = {arm: [] for arm in arms}
        for k in range(runs):
            for arm, flags in arms.items():                      # alternating: the spread beside the difference
                res = os.path.join(d, "res_%s_%d" % (arm, k))
                cmd = PB.in_process_command(os.path.join(d, "unused"), res, cfg_path, 4, 1, paths)
                i = cmd.index("--frames_dir")
                cmd[i:i + 2] = flags + ["--video_out", os.path.join(d, "out_%s.y4m" % arm)]
                wall = PB.child(cmd, d, timeout)
                print("%s run %d: %.1f s" % (arm, k, wall), file=sys.stderr, flush=True)
                with open(os.path.join(res, "deflicker.json")) as f:
                    rec = json.load(f)
                samples[arm].append({"wall_s": round(wall, 3), "seconds": rec["seconds"]})
        row = {"frames": 80, "runs": runs, "yuv_matrix": matrix,
               "bytes_in": {"y4m_8bit": os.path.getsize(os.path.join(d, "clip8.y4m")), "y4m_10bit_keep": os.path.getsize(os.path.join(d, "clip10.y4m"))}}
        for arm, ss in samples.items():
            row[arm] = {"wall_s": _summary([s["wall_s"] for s in ss]),
                        "seconds": {k: _summary([s["seconds"][k] for s in ss]) for k in ss[0]["seconds"]},
                        "outside_run_s": _summary([s["wall_s"] - s["seconds"]["total"] for s in ss]), "samples": ss}
        out[size] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pipeline", default=None, help="comma-separated WxH sizes of the 80-frame synthetic clip, e.g. 1920x1080")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child")
    ap.add_argument("--no_kernels", action="store_true", help="skip part 1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing here can be timed without one")
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.no_kernels:
        res["kernels"] = kernel_rows(a.calls)
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
