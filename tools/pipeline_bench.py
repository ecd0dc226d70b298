#!/usr/bin/env python
"""Wall clock of the whole pipeline on one MI355X (MEASUREMENTS.md Part K): all-in-one-deflicker_amd/deflicker.py (one process, device
hand-offs) against the three drop-in CLIs chained through the file system (preprocess_optical_flow.py, stage1.py --skip_preprocess,
neural_filter.py), on the same synthetic clip with the same synthetic weights, seed and config.

    python tools/pipeline_bench.py [--frames 80] [--size 768x432] [--down 4] [--seed 1] [--iters_num N] [--two_layer] [--out pipeline_bench.json]

With --two_layer both arms fit the fg/bg pair of atlases on synthetic masks (synthetic_masks): deflicker.py --masks_dir against
preprocess_optical_flow.py, stage1_seg.py --skip_preprocess, neural_filter.py.

The clip is built the way tools/raft_bench.py builds its frames (the smooth pattern of the RAFT fixture, shifted by a constant motion per
frame) with a seeded per-frame gain as the flicker; the weights are the fixtures' deterministic fills (tools/make_golden_raft.py,
tools/make_golden_stage2.py).  Both arms run in this session as fresh child processes, one after the other, each on a frame folder of
its own; a sample is the host clock around the child.  Seconds per stage: the in-process arm reports its own (deflicker.json, between
device synchronisations); the chained arm is one child per stage.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")


def synthetic_clip(n, h, w, seed=0, motion=(1.5, -1.0)):
    """n frames (h, w, 3) uint8: the RAFT fixture's smooth pattern moving by `motion` pixels per frame, each frame times a seeded
    per-channel gain (the flicker)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        x, y = xx - motion[0] * t, yy - motion[1] * t
        ch = [0.5 + 0.25 * np.sin(2 * np.pi * (x / 37.0 * (1 + 0.3 * c) + y / 53.0) + c) + 0.2 * np.cos(2 * np.pi * (y / 29.0 - x / 71.0 * (1 + c)))
              for c in range(3)]
        gain = 1.0 + 0.1 * rng.standard_normal(3)
        out.append(np.round(np.clip(np.stack(ch, -1) * gain, 0, 1) * 255).astype(np.uint8))
    return out


def synthetic_masks(n, h, w, motion=(1.5, -1.0)):
    """n foreground masks (h, w) uint8 for synthetic_clip's frames: a soft-edged elliptical blob (255 inside, 0 outside, a linear ramp
    about a tenth of the blob's radius wide between them) whose centre moves by `motion` pixels per frame, as the clip's pattern does."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rx, ry = 0.22 * w, 0.28 * h
    edge = 0.1
    out = []
    for t in range(n):
        cx, cy = 0.35 * w + motion[0] * t, 0.6 * h + motion[1] * t
        r = np.sqrt(((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2)
        out.append(np.round(np.clip((1.0 - r) / edge + 0.5, 0, 1) * 255).astype(np.uint8))
    return out


FLOW_HEAD_SCALE = 2.0 ** -4


def synthetic_weights():
    """(raft, filter, local) state dicts with the fixtures' deterministic fills.  RAFT's last flow-head convolution is scaled by
    FLOW_HEAD_SCALE: with the fill as it is the flows are ~14 px rms of noise, no pixel passes the forward/backward consistency test of
    the input builder, every stage-1 batch has no valid flow pixel and the loss is NaN by the reference's own rule (a mean over an empty
    set), on any route.  Scaled, the flows are below one pixel and every pixel is valid, so the atlas fit can run."""
    import aiod_amd  # noqa: F401
    import make_golden_raft
    import make_golden_stage2
    from aiod_amd.raft import raft_keys
    from aiod_amd.stage2 import filter_keys, local_keys
    rsd = {k: torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, s in raft_keys()}
    make_golden_raft.synthetic_state_dict(rsd)
    for k in ("update_block.flow_head.conv2.weight", "update_block.flow_head.conv2.bias"):
        rsd[k] *= FLOW_HEAD_SCALE
    fsd = {k: torch.zeros(s) for k, s in filter_keys()}
    lsd = {k: torch.zeros(s) for k, s in local_keys()}
    make_golden_stage2.synthetic_state_dicts(fsd, lsd)
    return rsd, fsd, lsd


def write_clip(folder, frames):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(folder, "%05d.png" % i))


def write_weights(folder, weights):
    os.makedirs(folder, exist_ok=True)
    paths = [os.path.join(folder, n) for n in ("raft.pth", "filter.pth", "local.pth")]
    for p, sd in zip(paths, weights):
        torch.save(sd, p)
    return paths


def write_masks(folder, masks):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, m in enumerate(masks):
        Image.fromarray(m).save(os.path.join(folder, "%05d.png" % i))


def chained_commands(vid, cfg, down, seed, paths, py=None, two_layer=False):
    """The three CLIs of the disk route, run from the folder that holds data/test/<vid> (two_layer: and data/test/<vid>_seg, with
    stage1_seg.py in the middle)."""
    py = py or sys.executable
    return [("flow", [py, os.path.join(PKG, "preprocess_optical_flow.py"), "--vid-path", os.path.join("data", "test", vid), "--model", paths[0], "--gpu", "0"]),
            ("stage 1", [py, os.path.join(PKG, "stage1_seg.py" if two_layer else "stage1.py"), "--vid_name", vid, "--config", cfg, "--down", str(down),
                         "--seed", str(seed), "--skip_preprocess", "--gpu", "0"]),
            ("stage 2", [py, os.path.join(PKG, "neural_filter.py"), "--video_name", vid, "--ckpt_filter", paths[1], "--ckpt_local", paths[2], "--gpu", "0"])]


def in_process_command(frames_dir, out, cfg, down, seed, paths, extra=(), py=None, masks_dir=None):
    return [py or sys.executable, os.path.join(PKG, "deflicker.py"), "--frames_dir", frames_dir, "--out", out, "--config", cfg, "--down", str(down),
            "--seed", str(seed), "--model", paths[0], "--ckpt_filter", paths[1], "--ckpt_local", paths[2], "--gpu", "0"] + \
        (["--masks_dir", masks_dir] if masks_dir is not None else []) + list(extra)


def child(cmd, cwd, timeout):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("child failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--size", default="768x432")
    ap.add_argument("--down", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--iters_num", type=int, default=None, help="shorten the stage-1 schedule (default: the shipped 10001)")
    ap.add_argument("--two_layer", action="store_true", help="both arms on the fg/bg two-layer path, with synthetic masks")
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    w, h = (int(v) for v in a.size.split("x"))
    d = tempfile.mkdtemp(prefix="af_pipeline_")
    cfg = dict(REFERENCE_CONFIG)
    if a.iters_num is not None:
        cfg.update(iters_num=a.iters_num, evaluate_every=a.iters_num - 1)
    cfg_path = os.path.join(d, "config.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    paths = write_weights(os.path.join(d, "weights"), synthetic_weights())
    frames = synthetic_clip(a.frames, h, w, seed=a.seed)
    roots = {arm: os.path.join(d, arm) for arm in ("in_process", "chained")}
    for r in roots.values():
        write_clip(os.path.join(r, "data", "test", "clip"), frames)
        if a.two_layer:
            write_masks(os.path.join(r, "data", "test", "clip_seg"), synthetic_masks(a.frames, h, w))
    res = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "frames": a.frames, "size": a.size, "down": a.down,
           "iters_num": cfg["iters_num"], "seed": a.seed, "two_layer": a.two_layer}
    out = os.path.join(roots["in_process"], "results", "clip")
    masks_dir = os.path.join(roots["in_process"], "data", "test", "clip_seg") if a.two_layer else None
    wall = child(in_process_command(os.path.join(roots["in_process"], "data", "test", "clip"), out, cfg_path, a.down, a.seed, paths, masks_dir=masks_dir),
                 roots["in_process"], a.timeout)
    with open(os.path.join(out, "deflicker.json")) as f:
        rec = json.load(f)
    res["in_process"] = {"wall_s": round(wall, 3), "seconds_inside": rec["seconds"], "psnr": rec["psnr"],
                         "start_imports_checkpoints_and_png_tail_s": round(wall - rec["seconds"]["total"], 3)}
    per = {}
    for name, cmd in chained_commands("clip", cfg_path, a.down, a.seed, paths, two_layer=a.two_layer):
        per[name] = round(child(cmd, roots["chained"], a.timeout), 3)
    res["chained"] = {"wall_s": round(sum(per.values()), 3), "seconds_per_child": per}
    from PIL import Image
    fin = [os.path.join(r, "results", "clip", "final", "output") for r in (roots["in_process"], roots["chained"])]
    names = sorted(os.listdir(fin[0]))
    res["final_frames_identical"] = names == sorted(os.listdir(fin[1])) and all(
        np.array_equal(np.asarray(Image.open(os.path.join(fin[0], n))), np.asarray(Image.open(os.path.join(fin[1], n)))) for n in names)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
