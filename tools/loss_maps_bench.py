"""Wall-clock cost of one frame's per-pixel loss maps (include/atlasfit.h af_render_loss_maps, every map of the handle's path)
against one af_render_frame, on both paths at the reference's evaluation size: 768x432 (resx x resy) with 80 frames,
nn.Linear-initialised nets, a synthetic clip (zero frames, a constant (1.5, 0.5) flow with the mask on, a fg mask on the left half).
Prints one JSON line (milliseconds per frame).

    python tools/loss_maps_bench.py [--frames 80] [--resx 768] [--resy 432] [--reps 5]
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


def handle(W, H, F, two_layer):
    af = aiod_amd.AtlasFit(aiod_amd.default_config(W, H, F, two_layer=two_layer))
    g = torch.Generator().manual_seed(0)
    for net in af.nets:
        sd = {}
        for i, (o, k) in enumerate(aiod_amd.atlasfit.imlp_shapes(net, af.cfg)):
            w, b = torch.empty(o, k), torch.empty(o)
            torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5), generator=g)
            torch.nn.init.uniform_(b, -1 / math.sqrt(k), 1 / math.sqrt(k), generator=g)
            sd["hidden.%d.weight" % i], sd["hidden.%d.bias" % i] = w, b
        af.load_state_dict(net, sd)
    z = np.zeros
    flow = z((H, W, 2, F, 1), np.float32); flow[:, :, 0] = 1.5; flow[:, :, 1] = 0.5
    fmask = np.ones((H, W, F, 1), np.float32); fmask[:, :, -1] = 0
    fg = z((H, W, F), np.float32); fg[:, : W // 2] = 1
    af.upload_video(z((H, W, 3, F), np.float32), flow, -flow, fmask, fmask, fg if two_layer else None)
    return af


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--resx", type=int, default=768)
    ap.add_argument("--resy", type=int, default=432)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    W, H, F = a.resx, a.resy, a.frames
    frames = list(range(0, F - 1, max(1, (F - 1) // a.reps)))[: a.reps]      # not the last frame: its flow maps need no flow rows
    res = {"shape": [F, H, W]}
    for tag, two in (("single", False), ("seg", True)):
        af = handle(W, H, F, two)
        res["mlp_mode"] = af.arithmetic["mlp_mode"]

        def t(fn):
            fn(frames[0])                   # warm-up (scratch growth, code-object load)
            af.sync()
            s = time.perf_counter()
            for f in frames:
                fn(f)
            af.sync()
            return (time.perf_counter() - s) * 1e3 / len(frames)
        res[tag + "_render_frame_ms"] = t(af.render_frame)
        res[tag + "_loss_maps_ms"] = t(af.loss_maps)
        res[tag + "_render_frame_ms_2"] = t(af.render_frame)          # again, after the maps: order effects
        res[tag + "_loss_maps_over_frame"] = res[tag + "_loss_maps_ms"] / res[tag + "_render_frame_ms"]
        af.close()
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
