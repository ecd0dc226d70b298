"""Wall-clock cost of the warping error (include/atlasfit.h af_warp_error / af_warp_error_pair) at the reference's evaluation size,
768x432 (resx x resy) with 80 frames, single-atlas handle with nn.Linear-initialised nets and a synthetic clip (random frames, a
constant (1.5, 0.5) flow and its negation backwards):
  * af_warp_error on the input (one launch over the 79 pairs, straight from the record table);
  * af_warp_error on the reconstruction, against F x one af_render_frame (the renders dominate);
  * one 1920x1080 af_warp_error_pair call on device pointers (maps off, and with noc + warped written).
Prints one JSON line (milliseconds per call) with the bytes each call must read at least (HBM lower bound, for a rocprofv3 run).

    python tools/warp_error_bench.py [--frames 80] [--resx 768] [--resy 432] [--reps 5]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aiod_amd  # noqa: E402


def handle(W, H, F):
    af = aiod_amd.AtlasFit(aiod_amd.default_config(W, H, F))
    g = torch.Generator().manual_seed(0)
    for net in af.nets:
        sd = {}
        for i, (o, k) in enumerate(aiod_amd.atlasfit.imlp_shapes(net, af.cfg)):
            w, b = torch.empty(o, k), torch.empty(o)
            torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5), generator=g)
            torch.nn.init.uniform_(b, -1 / math.sqrt(k), 1 / math.sqrt(k), generator=g)
            sd["hidden.%d.weight" % i], sd["hidden.%d.bias" % i] = w, b
        af.load_state_dict(net, sd)
    rng = np.random.default_rng(0)
    flow = np.zeros((H, W, 2, F, 1), np.float32); flow[:, :, 0] = 1.5; flow[:, :, 1] = 0.5
    fmask = np.ones((H, W, F, 1), np.float32); fmask[:, :, -1] = 0
    af.upload_video(rng.random((H, W, 3, F), np.float32), flow, -flow, fmask, fmask)
    return af


def timed(fn, reps, sync):
    fn()                                  # warm-up (scratch growth, code-object load)
    sync()
    s = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - s) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--resx", type=int, default=768)
    ap.add_argument("--resy", type=int, default=432)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    W, H, F = a.resx, a.resy, a.frames
    res = {"shape": [F, H, W]}
    af = handle(W, H, F)
    res["mlp_mode"] = af.arithmetic["mlp_mode"]
    res["input_ms"] = timed(lambda: af.warp_error("input"), a.reps, af.sync)
    res["input_min_bytes"] = F * H * W * 64                     # every pixel record once (frame t and t+1 share them through the L2)
    res["reconstruction_ms"] = timed(lambda: af.warp_error("reconstruction"), a.reps, af.sync)
    res["render_all_frames_ms"] = timed(lambda: [af.render_frame(f) for f in range(F)], a.reps, af.sync)
    res["reconstruction_over_renders"] = res["reconstruction_ms"] / res["render_all_frames_ms"]
    af.close()
    h2, w2 = 1080, 1920
    g = torch.Generator(device="cuda").manual_seed(1)
    i1, i2 = (torch.rand((h2, w2, 3), device="cuda", generator=g) for _ in range(2))
    f12 = torch.rand((h2, w2, 2), device="cuda", generator=g) * 4 - 2
    f21 = -f12
    res["pair_1080p_ms"] = timed(lambda: aiod_amd.warp_error_pair(i1, i2, f12, f21), a.reps * 4, torch.cuda.synchronize)
    res["pair_1080p_maps_ms"] = timed(lambda: aiod_amd.warp_error_pair(i1, i2, f12, f21, return_maps=True), a.reps * 4, torch.cuda.synchronize)
    res["pair_1080p_min_bytes"] = h2 * w2 * (12 + 12 + 8 + 8)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
