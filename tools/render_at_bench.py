#!/usr/bin/env python
"""Cost of rendering the fitted atlas at the clip's own size on one MI355X (MEASUREMENTS.md Part M).

    python tools/render_at_bench.py [--frames 8] [--rounds 5] [--pipeline [--clip_frames 80] [--iters_num N]] [--out render_at_bench.json]

A 768x432 handle (seeded nn.Linear init, the shipped architecture, a random uploaded video: the render's time does not depend on the
weights) renders frame 0..frames-1 through AtlasFit.render_frame_device (the stage-1 lattice: the per-row yardstick) and through
AtlasFit.render_frame_at_device at 768x432, 1920x1080 and 3840x2160, float and uint8 outputs and a uint8 reference as deflicker.py
--style_size full asks for them.  Both calls return host-synchronous, so a sample is the host clock around one call; per size the
median over rounds x frames calls after one untimed round, and the ns per evaluated pixel.

With --pipeline also the stage seconds of deflicker.py on Part K's synthetic clip (tools/pipeline_bench.py: 80 frames of 768x432,
synthetic weights, the shipped config, --down 4, --seed 1) with --style_size stage1 and with --style_size full, one fresh child each.
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESX, RESY = 768, 432
SIZES = [(432, 768), (1080, 1920), (2160, 3840)]


def _median_ms(fn, frames, rounds):
    for f in range(frames):
        fn(f)
    samples = []
    for _ in range(rounds):
        for f in range(frames):
            t0 = time.perf_counter()
            fn(f)
            samples.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(samples)), float(min(samples)), float(max(samples))


def renders(frames, rounds, two_layer=False):
    import aiod_amd
    from aiod_amd import stage1 as S
    g = torch.Generator().manual_seed(1)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(RESX, RESY, frames, two_layer=two_layer))
    out = {}
    try:
        S.init_networks(af, {"pretrain_mapping1": False, "pretrain_mapping2": False}, two_layer, g)
        dev = torch.device("cuda", 0)
        video = torch.rand((RESY, RESX, 3, frames), generator=g).to(dev)
        zeros, ones = torch.zeros((RESY, RESX, 2, frames), device=dev), torch.ones((RESY, RESX, frames), device=dev)
        af.upload_video(video, zeros, zeros, ones, ones, *((torch.rand((RESY, RESX, frames), generator=g).to(dev),) if two_layer else ()))
        med, lo, hi = _median_ms(lambda f: af.render_frame_device(f), frames, rounds)
        out["render_frame_device %dx%d" % (RESX, RESY)] = {"ms": med, "min": lo, "max": hi, "ns_per_pixel": med * 1e6 / (RESX * RESY)}
        for oh, ow in SIZES:
            ref = torch.randint(0, 256, (oh, ow, 3), generator=g, dtype=torch.uint8).to(dev)
            med, lo, hi = _median_ms(lambda f: af.render_frame_at_device(f, oh, ow, ref=ref), frames, rounds)
            out["render_frame_at_device %dx%d" % (ow, oh)] = {"ms": med, "min": lo, "max": hi, "ns_per_pixel": med * 1e6 / (oh * ow)}
    finally:
        af.close()
    return out


def pipeline(clip_frames, iters_num, timeout):
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tempfile.mkdtemp(prefix="af_render_at_")
    cfg = dict(REFERENCE_CONFIG)
    if iters_num is not None:
        cfg["iters_num"] = int(iters_num)
        cfg["evaluate_every"] = int(iters_num) - 1
    cfg_path = os.path.join(d, "config.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    paths = PB.write_weights(os.path.join(d, "weights"), PB.synthetic_weights())
    PB.write_clip(os.path.join(d, "clip"), PB.synthetic_clip(clip_frames, RESY, RESX, seed=5))
    out = {}
    for arm in ("stage1", "full"):
        res = os.path.join(d, "out_" + arm)
        wall = PB.child(PB.in_process_command(os.path.join(d, "clip"), res, cfg_path, 4, 1, paths, extra=["--style_size", arm]), d, timeout)
        rec = json.load(open(os.path.join(res, "deflicker.json")))
        out[arm] = {"wall": round(wall, 3), "seconds": rec["seconds"], "psnr": rec["psnr"], "psnr_full": rec["psnr_full"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--two_layer", action="store_true", help="the renders on a fg/bg two-layer handle")
    ap.add_argument("--pipeline", action="store_true", help="also deflicker.py --style_size stage1 against full on Part K's clip")
    ap.add_argument("--clip_frames", type=int, default=80)
    ap.add_argument("--iters_num", type=int, default=None, help="shorten the stage-1 schedule of --pipeline (default: the shipped 10001)")
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child of --pipeline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found")
    res = {"device": torch.cuda.get_device_name(0), "handle": "%dx%d" % (RESX, RESY), "two_layer": a.two_layer, "renders": renders(a.frames, a.rounds, a.two_layer)}
    if a.pipeline:
        res["pipeline"] = pipeline(a.clip_frames, a.iters_num, a.timeout)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
