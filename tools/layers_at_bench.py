#!/usr/bin/env python
"""Cost of the layer products and of texture-edit propagation at any size on one MI355X (MEASUREMENTS.md Part O).

    python tools/layers_at_bench.py [--frames 4] [--rounds 3] [--res 1000 4000] [--out layers_at_bench.json]

A 768x432x80 two-layer handle (seeded nn.Linear init, the shipped architecture, no video: none of these calls reads one; the time does
not depend on the weights) with a random texture pair of side `res` on the windows fg (0, 0, 1), bg (-1, -1, 1).  Per row the median,
minimum and maximum over rounds x frames calls after one untimed round; every call returns host-synchronous, so a sample is the host
clock around one call.  Rows:
    render_edit at the lattice          AtlasFit.render_edit: both textures uploaded on every call (the route before edit sessions; baseline)
    session at the lattice              EditSession.frame: the textures resident
    session at 1920x1080 / 3840x2160    float32 edit to the host, uint8 edit to the host (what atlas_edit.py writes), uint8 edit on the device
    render_layers / render_layers_at    the five layer outputs (and alpha_u8 off the lattice) to the host and on the device
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESX, RESY, FRAMES = 768, 432, 80
SIZES = [(1080, 1920), (2160, 3840)]
WIN_FG, WIN_BG = (0.0, 0.0, 1.0), (-1.0, -1.0, 1.0)


def _stats(fn, frames, rounds):
    for f in range(frames):
        fn(f)
    samples = []
    for _ in range(rounds):
        for f in range(frames):
            t0 = time.perf_counter()
            fn(f)
            samples.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(samples)), "min": float(min(samples)), "max": float(max(samples)), "n": len(samples)}


def run(frames, rounds, sides):
    import aiod_amd
    from aiod_amd import stage1 as S
    g = torch.Generator().manual_seed(1)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(RESX, RESY, FRAMES, two_layer=True))
    out = {}
    try:
        S.init_networks(af, {"pretrain_mapping1": False, "pretrain_mapping2": False}, True, g)
        out["render_layers %dx%d host" % (RESX, RESY)] = _stats(lambda f: af.render_layers(f), frames, rounds)
        for oh, ow in [(RESY, RESX)] + SIZES:
            r = _stats(lambda f: af.render_layers_at(f, oh, ow, alpha_u8=True), frames, rounds)
            r["ns_per_pixel"] = r["ms"] * 1e6 / (oh * ow)
            out["render_layers_at %dx%d host" % (ow, oh)] = r
            r = _stats(lambda f: af.render_layers_at_device(f, oh, ow, alpha_u8=True), frames, rounds)
            r["ns_per_pixel"] = r["ms"] * 1e6 / (oh * ow)
            out["render_layers_at %dx%d device" % (ow, oh)] = r
        for res in sides:
            t1 = torch.rand((res, res, 3), generator=g).numpy()
            t2 = torch.rand((res, res, 3), generator=g).numpy()
            out["render_edit %dx%d res %d (textures uploaded per call)" % (RESX, RESY, res)] = _stats(
                lambda f: af.render_edit(f, res, t1, WIN_FG, t2, WIN_BG, outputs=("edit",)), frames, rounds)
            t0 = time.perf_counter()
            s = af.edit_session(res, t1, WIN_FG, t2, WIN_BG)
            out["edit_session create res %d" % res] = {"ms": (time.perf_counter() - t0) * 1e3, "n": 1}
            with s:
                out["session %dx%d res %d float host" % (RESX, RESY, res)] = _stats(lambda f: s.frame(f), frames, rounds)
                for oh, ow in SIZES:
                    for tag, fn in (("float host", lambda f: s.frame(f, oh, ow)), ("u8 host", lambda f: s.frame(f, oh, ow, outputs=(), u8=True)),
                                    ("u8 device", lambda f: s.frame_device(f, oh, ow, outputs=(), u8=True))):
                        r = _stats(fn, frames, rounds)
                        r["ns_per_pixel"] = r["ms"] * 1e6 / (oh * ow)
                        out["session %dx%d res %d %s" % (ow, oh, res, tag)] = r
    finally:
        af.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--res", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found")
    res = {"device": torch.cuda.get_device_name(0), "handle": "%dx%dx%d two_layer" % (RESX, RESY, FRAMES), "frames": a.frames, "rounds": a.rounds,
           "rows": run(a.frames, a.rounds, a.res)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
