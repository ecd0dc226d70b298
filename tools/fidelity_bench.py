#!/usr/bin/env python
"""Cost of the fidelity report on one MI355X (MEASUREMENTS.md Part Y): af_fidelity, and deflicker.py with and without --fidelity.

    python tools/fidelity_bench.py [--calls 20] [--frames 80] [--size 768x432] [--runs 3] [--iters_num N] [--timeout 600]
                                   [--skip_pipeline] [--skip_kernels] [--out fidelity_bench.json]

Kernel: af_fidelity (csrc/fidelity.hip) with device pointers at 1920x1080 and 3840x2160, 1 and 8 frames per call, window 7, for the SSE
alone and for SSE + SSIM (no map): the host clock around each call (host-synchronous: it stages its partial sums, launches, synchronises,
copies the partials back and adds them), median of --calls calls after a warm-up; beside each, in the same run, a device-to-device copy
of the bytes the call reads (both sequences: 6 bytes per pixel; torch's copy_ between two synchronisations), and the ratio of the two.
The timed result is checked against the numpy restatement (tests/fidelity_ref.py) on a 270-row crop of the first frame.

Pipeline: deflicker.py on the synthetic clip of tools/pipeline_bench.py (--frames frames at --size) with the synthetic weights, once with
--fidelity and once without, alternating, each the median of --runs fresh child processes, every child under its own time limit; the
final frames of the two arms are compared byte for byte.  Prints one JSON line."""
import argparse
import ctypes as C
import hashlib
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
import pipeline_bench as PB  # noqa: E402
from shots_bench import _median_ms  # noqa: E402


def kernel_rows(calls, win=7):
    import aiod_amd
    import fidelity_ref as R
    lib = aiod_amd.load_library()
    rows = []
    gen = torch.Generator().manual_seed(0)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for w, h in ((1920, 1080), (3840, 2160)):
        a = torch.randint(0, 256, (8, h, w, 3), dtype=torch.uint8, generator=gen).cuda()
        b = (a.float() * 1.05 + torch.randint(-4, 5, a.shape, generator=gen).cuda()).clamp(0, 255).round().to(torch.uint8)
        for n in (1, 8):
            nbytes = 2 * n * h * w * 3
            src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            sse, ssim = np.zeros((n, 3), np.uint64), np.zeros((n, 3))
            row = {"size": "%dx%d" % (w, h), "frames_per_call": n, "window": win, "calls": calls, "bytes_read": nbytes}
            cms, clo, chi = _median_ms(lambda: dst.copy_(src), calls)
            row["d2d_copy_same_bytes"] = {"ms": round(cms, 4), "ms_min_max": [round(clo, 4), round(chi, 4)], "GBps_of_bytes_read": round(nbytes / cms / 1e6, 1)}
            for name, ssim_ptr in (("sse", None), ("sse_ssim", ssim.ctypes.data_as(C.c_void_p))):
                def call():
                    rc = lib.af_fidelity(0, q(a), q(b), n, h, w, win, sse.ctypes.data_as(C.c_void_p), ssim_ptr, None, 1)
                    assert rc == 0, lib.af_last_error(None).decode()
                ms, lo, hi = _median_ms(call, calls)
                row[name] = {"ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "ms_per_frame": round(ms / n, 4),
                             "GBps_of_bytes_read": round(nbytes / ms / 1e6, 1), "ratio_to_copy": round(ms / cms, 2)}
            rows.append(row)
        crop_a, crop_b = a[0, :270].contiguous(), b[0, :270].contiguous()
        r = aiod_amd.frame_fidelity_device(crop_a, crop_b, win, want_map=True)
        want = R.ssim_map(crop_a.cpu().numpy(), crop_b.cpu().numpy(), win)
        assert np.array_equal(r["map"][0].cpu().numpy().view(np.uint64), want.view(np.uint64)) and np.array_equal(r["sse"][0], R.sse(crop_a.cpu().numpy(), crop_b.cpu().numpy()))
        rows[-1]["equal_to_restatement_on_a_270_row_crop"] = True
    return rows


def _digest(folder):
    h = hashlib.sha256()
    for name in sorted(os.listdir(folder)):
        with open(os.path.join(folder, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def pipeline(frames, size, runs, iters_num, down, seed, timeout):
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    w, h = (int(v) for v in size.split("x"))
    d = tempfile.mkdtemp(prefix="af_fidelity_")
    cfg = dict(REFERENCE_CONFIG)
    if iters_num is not None:
        cfg.update(iters_num=iters_num, evaluate_every=iters_num - 1)
    cfg_path = os.path.join(d, "config.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    paths = PB.write_weights(os.path.join(d, "weights"), PB.synthetic_weights())
    clip = os.path.join(d, "clip")
    PB.write_clip(clip, PB.synthetic_clip(frames, h, w, seed=seed))
    res = {"frames": frames, "size": size, "runs": runs, "iters_num": cfg["iters_num"], "down": down, "seed": seed}
    arms = {"fidelity": ["--fidelity"], "plain": []}
    samples = {arm: [] for arm in arms}
    for k in range(runs):                                     # alternating: a drift of the machine touches both arms alike
        for arm, extra in arms.items():
            out = os.path.join(d, "%s_%d" % (arm, k))
            wall = PB.child(PB.in_process_command(clip, out, cfg_path, down, seed, paths, extra=extra), d, timeout)      # each child under its own limit
            with open(os.path.join(out, "deflicker.json")) as f:
                samples[arm].append((wall, out, json.load(f)))
            print("[fidelity_bench] %s child %d: %.1f s" % (arm, k, wall), file=sys.stderr, flush=True)
    digests = {}
    for arm, ss in samples.items():
        digests[arm] = {_digest(os.path.join(out, "final", "output")) for _, out, _ in ss}
        wall, out, rec = sorted(ss, key=lambda s: s[0])[(len(ss) - 1) // 2]
        res[arm] = {"wall_s": round(statistics.median(s[0] for s in ss), 3), "wall_s_all": [round(s[0], 3) for s in ss], "seconds_inside": rec["seconds"]}
        if "fidelity" in rec:
            res[arm]["record"] = {"window": rec["fidelity"]["window"], "size": rec["fidelity"]["size"],
                                  "psnr_mean": rec["fidelity"]["final_vs_input"]["psnr"]["mean"], "ssim_mean": rec["fidelity"]["final_vs_input"]["ssim"]["mean"]}
    res["final_frames_equal_in_both_arms"] = len(digests["fidelity"] | digests["plain"]) == 1
    lap = res["fidelity"]["seconds_inside"]
    res["fidelity_share_of_run"] = round(lap["fidelity"] / lap["total"], 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--size", default="768x432")
    ap.add_argument("--runs", type=int, default=3, help="child processes per arm; the median is reported")
    ap.add_argument("--iters_num", type=int, default=None, help="shorten the stage-1 schedule (default: the shipped 10001)")
    ap.add_argument("--down", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    ap.add_argument("--skip_pipeline", action="store_true", help="the kernels only")
    ap.add_argument("--skip_kernels", action="store_true", help="the pipeline arms only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing here can be timed without one")
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_kernels:
        res["kernels"] = kernel_rows(a.calls)
    if not a.skip_pipeline:
        res["pipeline"] = pipeline(a.frames, a.size, a.runs, a.iters_num, a.down, a.seed, a.timeout)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
