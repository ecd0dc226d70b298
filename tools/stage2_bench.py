"""Wall clock of stage 2 per frame (MEASUREMENTS.md Part I): af_filter_frame (both nets, device inputs and outputs) against the same
two nets as torch modules on the same GPU (NCHW, MIOpen: in fp32 and under torch.autocast("cuda", dtype=torch.float16)), at 640x384
(the reference's sample clip, padded size) and 1920x1088.  Prints one JSON line per size: ms per frame of each, the nominal TFLOP per
frame (2 * MACs of every convolution, counted from the layer shapes), the achieved TF/s and the fraction of the 157.3 TF fp32 matrix
peak, and a sha256 of the native path's last pred and final (to compare two builds on the same frames).

    python tools/stage2_bench.py [--frames 10] [--warmup 3] [--sizes 384x640,1088x1920] [--precision fp32|fp16] [--no_torch]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK_TF = 157.3


def conv_flops(H, W):
    """Per frame, both nets (the refinement net runs on every frame but the first): {layer: FLOP}."""
    f = {}
    c = 6
    for lv, n in enumerate((32, 64, 128, 256, 512)):
        p = (H >> lv) * (W >> lv)
        f["enc%d.conv1" % lv] = 2 * p * n * c * 9
        f["enc%d.conv2" % lv] = 2 * p * n * n * 9
        c = n
    for lv, n in zip((3, 2, 1, 0), (256, 128, 64, 32)):
        p = (H >> lv) * (W >> lv)
        f["up%d" % lv] = 2 * p * n * 2 * n * 9
        f["dec%d.conv1" % lv] = 2 * p * n * 2 * n * 9
        f["dec%d.conv2" % lv] = 2 * p * n * n * 9
    P = H * W
    f["out1x1"] = 2 * P * 3 * 32
    f["conv1a+b"] = 2 * 2 * P * 32 * 6 * 49
    f["conv2a+b"] = 2 * 2 * (P // 4) * 64 * 32 * 9
    f["conv3"] = 2 * (P // 16) * 128 * 128 * 9
    f["resblocks"] = 10 * 2 * (P // 16) * 128 * 128 * 9
    f["gates"] = 2 * (P // 16) * 512 * 128 * 9
    f["deconv1"] = 2 * (P // 4) * 64 * 128 * 9
    f["deconv2"] = 2 * P * 32 * 128 * 9
    f["deconv3"] = 2 * P * 3 * 64 * 49
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="384x640,1088x1920")
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32", help="arithmetic of the native path (NeuralFilter(precision=...))")
    ap.add_argument("--no_torch", action="store_true", help="skip the two torch columns")
    a = ap.parse_args()
    import aiod_amd
    from make_golden_stage2 import synthetic_state_dicts
    from aiod_amd.stage2 import filter_keys, local_keys
    fsd = {k: torch.zeros(s) for k, s in filter_keys()}
    lsd = {k: torch.zeros(s) for k, s in local_keys()}
    synthetic_state_dicts(fsd, lsd)
    from test_gpu_stage2 import unet_ref, local_ref
    dev = torch.device("cuda:0")
    gf = {k: v.to(dev) for k, v in fsd.items()}
    gl = {k: v.to(dev) for k, v in lsd.items()}
    for size in a.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        g = torch.Generator(device="cpu").manual_seed(1)
        frames = [(torch.rand(h, w, 3, generator=g).to(dev), torch.rand(h, w, 3, generator=g).to(dev)) for _ in range(4)]
        nf = aiod_amd.NeuralFilter(h, w) if a.precision == "fp32" else aiod_amd.NeuralFilter(h, w, precision=a.precision)
        nf.load_state_dicts(fsd, lsd)
        n = a.warmup + a.frames
        for i in range(a.warmup):
            nf.frame(*frames[i % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            last = nf.frame(*frames[i % 4])
        torch.cuda.synchronize()
        hip_ms = (time.perf_counter() - t0) * 1e3 / a.frames
        digest = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in last)).hexdigest()[:16]
        nf.close()
        # the same nets as torch modules on the GPU (the script's own loop: UNet, then the refinement on every later frame)
        torch_ms = {}
        for col, amp in (() if a.no_torch else (("fp32", False), ("autocast_fp16", True))):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                from make_golden_stage2 import pad_other
                o1 = p1 = None
                for i in range(n):
                    if i == a.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    c, s = (pad_other(t.permute(2, 0, 1)[None]) for t in frames[i % 4])
                    pred = unet_ref(gf, torch.cat((c, s), 1), {})
                    if i == 0:
                        o1 = p1 = pred
                    else:
                        fin = pred + local_ref(gl, torch.cat((pred, o1, pred, p1), 1), {})
                        p1, o1 = pred, fin
                torch.cuda.synchronize()
                torch_ms[col] = (time.perf_counter() - t0) * 1e3 / a.frames
        Hp, Wp, _ = aiod_amd.stage2.padded_size(h, w)
        fl = conv_flops(Hp, Wp)
        tot = sum(fl.values())
        r3 = lambda v: None if v is None else round(v, 3)      # noqa: E731
        print(json.dumps({"size": "%dx%d" % (w, h), "padded": "%dx%d" % (Wp, Hp), "precision": a.precision, "hip_ms_per_frame": round(hip_ms, 3),
                          "torch_miopen_ms_per_frame": r3(torch_ms.get("fp32")), "torch_miopen_autocast_fp16_ms_per_frame": r3(torch_ms.get("autocast_fp16")),
                          "tflop_per_frame": round(tot / 1e12, 4),
                          "hip_tflops": round(tot / hip_ms / 1e9, 2), "hip_frac_of_peak": round(tot / hip_ms / 1e9 / PEAK_TF, 4),
                          "torch_tflops": None if a.no_torch else round(tot / torch_ms["fp32"] / 1e9, 2), "out_sha256": digest,
                          "top3_layers_tflop": sorted(((k, round(v / 1e12, 4)) for k, v in fl.items()), key=lambda kv: -kv[1])[:3]}),
              flush=True)


if __name__ == "__main__":
    main()
