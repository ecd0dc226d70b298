"""Wall-clock cost of the layer-decomposition calls (include/atlasfit.h af_render_layers, af_mapping_area, af_render_atlas_texture,
af_render_edit) at the reference's evaluation size: a two_layer handle at 768x432 (resx x resy) with 80 frames, nn.Linear-initialised
nets, a synthetic clip (zero frames and flows, a fg mask on the left half).  Prints one JSON line (milliseconds).

    python tools/layers_bench.py [--frames 80] [--resx 768] [--resy 432] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--resx", type=int, default=768)
    ap.add_argument("--resy", type=int, default=432)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    W, H, F = a.resx, a.resy, a.frames
    af = aiod_amd.AtlasFit(aiod_amd.default_config(W, H, F, two_layer=True))
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
    mask = z((H, W, F), np.float32); mask[:, : W // 2] = 1
    af.upload_video(z((H, W, 3, F), np.float32), z((H, W, 2, F, 1), np.float32), z((H, W, 2, F, 1), np.float32),
                    z((H, W, F, 1), np.float32), z((H, W, F, 1), np.float32), mask)

    def t(fn, reps=a.reps):
        fn()
        af.sync()
        s = time.perf_counter()
        for _ in range(reps):
            fn()
        af.sync()
        return (time.perf_counter() - s) * 1e3 / reps

    frames = list(range(0, F, max(1, F // a.reps)))[: a.reps]
    res = {"shape": [F, H, W], "mlp_mode": af.arithmetic["mlp_mode"]}
    res["render_frame_ms"] = t(lambda: [af.render_frame(f) for f in frames], 1) / len(frames)
    res["render_layers_ms"] = t(lambda: [af.render_layers(f) for f in frames], 1) / len(frames)
    res["render_frame_ms_2"] = t(lambda: [af.render_frame(f) for f in frames], 1) / len(frames)    # again, after the layers: order effects
    res["mapping_area_bg_ms"] = t(lambda: af.mapping_area(1), 2)
    res["mapping_area_fg_ms"] = t(lambda: af.mapping_area(0), 2)
    res["atlas_texture_1000_ms"] = t(lambda: af.atlas_texture(1000, (0.0, 0.0, 1.0)), 3)
    tex = np.full((1000, 1000, 3), 0.5, np.float32)
    win = af.area_window(af.mapping_area(1))
    u1, u2 = np.zeros((1000, 1000), np.float32), np.zeros((1000, 1000), np.float32)
    res["render_edit_ms"] = t(lambda: af.render_edit(F // 2, 1000, tex, (0, 0, 1), tex, win, use_fg=u1, use_bg=u2), 3)
    res["render_edit_masks_only_ms"] = t(lambda: af.render_edit(F // 2, 1000, None, (0, 0, 1), None, win, use_fg=u1, use_bg=u2, outputs=()), 3)
    res["layers_over_frame"] = res["render_layers_ms"] / res["render_frame_ms"]
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))
    af.close()


if __name__ == "__main__":
    main()
