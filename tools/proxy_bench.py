#!/usr/bin/env python
"""Cost of the proxy route on one MI355X (MEASUREMENTS.md Part X): the guided-transfer kernels, and deflicker.py with and without
--proxy_long_edge.

    python tools/proxy_bench.py [--calls 20] [--frames 80] [--size 3840x2160] [--proxy_long_edge 1920] [--runs 3] [--iters_num N]
                                [--guide channel|colour] [--timeout 900] [--skip_pipeline] [--out proxy_bench.json]

Kernels: af_guided_coeffs (two launches: coefficients, box means; csrc/guided.hip) and af_guided_apply with device pointers at
1920x1080 -> 3840x2160 and 960x540 -> 1920x1080, r = 8: the host clock around each call (host-synchronous: launch, synchronise), median of
--calls calls after a warm-up; beside each, in the same run, a device-to-device copy of the same byte count (torch's copy_ between two
synchronisations).  The byte counts are the compulsory traffic: coeffs reads two uint8 images, writes and reads back the two unsmoothed
fp32 planes and writes the two smoothed ones (78 bytes per proxy pixel); apply reads and writes one full-size uint8 image and reads the
two planes once (6 bytes per full-size pixel + 24 per proxy pixel).  The timed result is checked against the numpy restatement
(tests/guided_transfer_ref.py) at the smaller size.  With --guide colour (MEASUREMENTS.md Part XII) the kernels are those of the colour guide,
af_guided_coeffs_colour (three launches: window sums, solve, box means), af_guided_apply_colour and af_guided_apply_colour16 at 10 bits, and
the pipeline's proxy arm runs with --proxy_guide colour.  Their compulsory traffic: coeffs reads two uint8 images, writes and reads back the
21 int32 planes of sums and the 12 unsmoothed fp32 planes and writes the 12 smoothed ones (6 + 168 + 96 + 48 = 318 bytes per proxy pixel);
apply reads and writes one full-size image and reads the 12 planes once (6, or 12 at 16-bit samples, bytes per full-size pixel + 48 per
proxy pixel).  --guide channel also times af_guided_apply16.

Pipeline: deflicker.py on the synthetic clip of tools/pipeline_bench.py (--frames frames at --size) with the synthetic weights, once with
--proxy_long_edge and once without, each the median of --runs fresh child processes, every child under its own time limit; the seconds
each arm reports per stage are those of its median child.  The PSNR of the proxy arm's final frames against the full-size arm's (same
clip, same seed) is a record and never an assertion: the weights are synthetic.  Prints one JSON line."""
import argparse
import ctypes as C
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
from shots_bench import _clocks, _median_ms  # noqa: E402


def kernel_rows(calls, radius=8, eps=64.0, guide="channel"):
    import aiod_amd
    import guided_colour_ref as RC
    import guided_transfer_ref as R
    lib = aiod_amd.load_library()
    colour = guide == "colour"
    f_coeffs = lib.af_guided_coeffs_colour if colour else lib.af_guided_coeffs
    f_apply, f_apply16 = (lib.af_guided_apply_colour, lib.af_guided_apply_colour16) if colour else (lib.af_guided_apply, lib.af_guided_apply16)
    na, per_proxy, bits = (9, 318, 10) if colour else (3, 78, 10)
    rows = []
    gen = torch.Generator().manual_seed(0)
    for (w, h), (W, H) in (((1920, 1080), (3840, 2160)), ((960, 540), (1920, 1080))):
        full = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=gen).cuda()
        pin = aiod_amd.resize_area_device(full, h, w)
        pout = (pin.float() * 1.05 + torch.randint(-4, 5, pin.shape, generator=gen).cuda()).clamp(0, 255).round().to(torch.uint8)
        a, b = torch.empty((h, w, na), device="cuda"), torch.empty((h, w, 3), device="cuda")
        work, out = torch.empty((33 if colour else 6) * h * w, device="cuda"), torch.empty_like(full)
        full16 = (full.to(torch.int16) * 4).view(torch.uint16)      # the frame at 10 bits
        out16 = torch.empty_like(full16)
        q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

        def coeffs():
            rc = f_coeffs(0, q(pin), q(pout), h, w, radius, eps, q(a), q(b), q(work), 1)
            assert rc == 0, lib.af_last_error(None).decode()

        def apply():
            rc = f_apply(0, q(full), H, W, q(a), q(b), h, w, q(out), 1)
            assert rc == 0, lib.af_last_error(None).decode()

        def apply16():
            rc = f_apply16(0, q(full16), H, W, bits, q(a), q(b), h, w, q(out16), 1)
            assert rc == 0, lib.af_last_error(None).decode()

        row = {"guide": guide, "proxy": "%dx%d" % (w, h), "full": "%dx%d" % (W, H), "radius": radius, "calls": calls}
        plane_bytes = 4 * (na + 3) * h * w
        for name, fn, nbytes in (("coeffs", coeffs, per_proxy * h * w), ("apply", apply, 6 * H * W + plane_bytes), ("apply16", apply16, 12 * H * W + plane_bytes)):
            src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            ms, lo, hi = _median_ms(fn, calls)
            cms, clo, chi = _median_ms(lambda: dst.copy_(src), calls)
            row[name] = {"bytes_read_plus_written": nbytes, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                         "GBps_read_plus_written": round(nbytes / ms / 1e6, 1),
                         "d2d_copy_same_bytes": {"ms": round(cms, 4), "ms_min_max": [round(clo, 4), round(chi, 4)],
                                                 "GBps_read_plus_written": round(nbytes / cms / 1e6, 1)}}
        if h <= 540:      # the restatement is numpy: checked at the smaller size only
            want = (RC if colour else R).transfer(full.cpu().numpy(), pin.cpu().numpy(), pout.cpu().numpy(), radius, eps)
            assert np.array_equal(out.cpu().numpy(), want)
            row["equal_to_restatement"] = True
        row["clocks_after"] = _clocks()
        rows.append(row)
    return rows


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return None if mse == 0 else round(10.0 * np.log10(255.0 ** 2 / mse), 3)


def pipeline(frames, size, edge, runs, iters_num, down, seed, timeout, guide="channel"):
    from PIL import Image
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    w, h = (int(v) for v in size.split("x"))
    d = tempfile.mkdtemp(prefix="af_proxy_")
    cfg = dict(REFERENCE_CONFIG)
    if iters_num is not None:
        cfg.update(iters_num=iters_num, evaluate_every=iters_num - 1)
    cfg_path = os.path.join(d, "config.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    paths = PB.write_weights(os.path.join(d, "weights"), PB.synthetic_weights())
    clip = os.path.join(d, "clip")
    PB.write_clip(clip, PB.synthetic_clip(frames, h, w, seed=seed))
    print("[proxy_bench] wrote %d frames of %s" % (frames, size), file=sys.stderr, flush=True)
    res = {"frames": frames, "size": size, "proxy_long_edge": edge, "guide": guide, "runs": runs, "iters_num": cfg["iters_num"], "down": down, "seed": seed}
    for arm, extra in (("proxy", ["--proxy_long_edge", str(edge)] + (["--proxy_guide", guide] if guide != "channel" else [])), ("full", [])):
        samples = []
        for k in range(runs):
            out = os.path.join(d, "%s_%d" % (arm, k))
            wall = PB.child(PB.in_process_command(clip, out, cfg_path, down, seed, paths, extra=extra), d, timeout)      # each child under its own limit
            with open(os.path.join(out, "deflicker.json")) as f:
                samples.append((wall, out, json.load(f)))
            print("[proxy_bench] %s child %d: %.1f s" % (arm, k, wall), file=sys.stderr, flush=True)
        samples.sort(key=lambda s: s[0])
        wall, out, rec = samples[(len(samples) - 1) // 2]
        res[arm] = {"wall_s": round(statistics.median(s[0] for s in samples), 3), "wall_s_all": [round(s[0], 3) for s in samples],
                    "seconds_inside": rec["seconds"], "out": out}
        if "proxy" in rec:
            res[arm]["record"] = rec["proxy"]
    fin = [os.path.join(res[arm].pop("out"), "final", "output") for arm in ("proxy", "full")]
    names = sorted(os.listdir(fin[0]))
    assert names == sorted(os.listdir(fin[1])) and len(names) == frames
    psnr = [_psnr(np.asarray(Image.open(os.path.join(fin[0], n))), np.asarray(Image.open(os.path.join(fin[1], n)))) for n in names]
    finite = [p for p in psnr if p is not None]
    res["psnr_proxy_final_vs_full_final"] = {"mean": round(float(np.mean(finite)), 3) if finite else None, "min": min(finite) if finite else None,
                                             "identical_frames": len(psnr) - len(finite)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--proxy_long_edge", type=int, default=1920)
    ap.add_argument("--runs", type=int, default=3, help="child processes per arm; the median is reported")
    ap.add_argument("--iters_num", type=int, default=None, help="shorten the stage-1 schedule (default: the shipped 10001)")
    ap.add_argument("--down", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--guide", default="channel", choices=("channel", "colour"), help="the guide of the transfer: the kernels timed, and the proxy arm's --proxy_guide")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--skip_pipeline", action="store_true", help="the kernels only")
    ap.add_argument("--skip_kernels", action="store_true", help="the pipeline arms only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing here can be timed without one")
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_kernels:
        res["kernels"] = kernel_rows(a.calls, guide=a.guide)
    if not a.skip_pipeline:
        res["pipeline"] = pipeline(a.frames, a.size, a.proxy_long_edge, a.runs, a.iters_num, a.down, a.seed, a.timeout, a.guide)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
