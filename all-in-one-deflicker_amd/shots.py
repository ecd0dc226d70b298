"""Scene cuts: where a clip's content changes, so that the pipeline can fit each shot on its own.

    python all-in-one-deflicker_amd/shots.py --frames_dir data/test/X [--grid 16x16] [--cut_threshold 0.5] [--cut_margin 0.25]
        [--cut_radius 4] [--min_shot_frames 5] [--gpu 0]

prints one JSON line (scores, cuts, shots, the parameters) and needs no checkpoint: the cuts of a clip can be reviewed before a long
run, and passed to deflicker.py --cuts I,J,K if they need correcting.

The device computes exact integer luminance sums over a coarse grid of every frame (af_luma_grid, csrc/shots.hip: 77 R + 150 G + 29 B
per pixel, 64-bit totals); everything after that is numpy in fp64 on (n, GH, GW) numbers.  The score of a pair of consecutive frames is
the zero-mean normalised cross-correlation of their grids: a frame-wide gain or offset - which is what flicker is - leaves it at 1,
where absolute differences or histograms would call every flicker a cut.  A pair is a cut when its score is low (`threshold`) AND lower
by `margin` than the median of its neighbours (`radius` pairs to each side): sustained fast motion lowers every score alike and is not
cut.  The four defaults are policy: nobody has measured them on footage."""
import argparse
import json
import os
import sys

import numpy as np

if __package__:      # run as a script this file only re-imports itself as part of the package (below)
    from ._residence import Device, Host

_HERE = os.path.dirname(os.path.abspath(__file__))
GRID = (16, 16)
CUT_DEFAULTS = {"threshold": 0.5, "margin": 0.25, "radius": 4, "min_shot_frames": 5}
LUMA_WEIGHTS = (77, 150, 29)      # sum 256: a cell's mean luminance is sum / (256 * count)


def cell_counts(h, w, grid=GRID):
    """Pixels per cell (GH, GW) int64 of af_luma_grid's grid over an h x w frame: GH = min(gh, h), GW = min(gw, w), cell (i, j) is rows
    [i*h // GH, (i+1)*h // GH) by columns [j*w // GW, (j+1)*w // GW)."""
    gh, gw = min(int(grid[0]), int(h)), min(int(grid[1]), int(w))
    rows = np.diff(np.arange(gh + 1, dtype=np.int64) * int(h) // gh)
    cols = np.diff(np.arange(gw + 1, dtype=np.int64) * int(w) // gw)
    return rows[:, None] * cols[None, :]


def _grid_block(block, gh, gw, device):
    """One af_luma_grid call on a contiguous block (N, H, W, 3) of uint8 frames, numpy (host pointer) or CUDA tensor (device pointer)."""
    from .atlasfit import load_library, _util_chk, _ptr
    n, h, w = int(block.shape[0]), int(block.shape[1]), int(block.shape[2])
    out = np.empty((n, min(gh, h), min(gw, w)), np.uint64)
    if hasattr(block, "is_cuda") and not block.is_cuda:
        raise ValueError("luma_grids: tensors must be CUDA tensors (pass host frames as numpy arrays)")
    res = Device(block.device) if hasattr(block, "is_cuda") else Host(device)      # the tensor's own device: that is where its producers ran
    block = res.contiguous(block)
    res.sync()
    _util_chk(load_library().af_luma_grid(res.ordinal, res.ptr(block), n, h, w, int(gh), int(gw), _ptr(out), res.on_device))
    return out.astype(np.int64)


def luma_grids(frames, grid=GRID, device=0):
    """-> (sums int64 (n, GH, GW), counts int64 (GH, GW)) of a clip: a list of (H, W, 3) uint8 numpy arrays or CUDA tensors, or one
    (N, H, W, 3) array or tensor.  One af_luma_grid call per contiguous block: one for a 4-D input, one per frame of a list.  `device` is
    where host frames are staged; a CUDA tensor is summed on the device it lives on."""
    gh, gw = int(grid[0]), int(grid[1])
    blocks = [frames] if hasattr(frames, "ndim") and frames.ndim == 4 else [f[None] for f in frames]
    if not blocks:
        raise ValueError("luma_grids: no frames")
    shape = tuple(blocks[0].shape[1:])
    for i, b in enumerate(blocks):
        if b.ndim != 4 or b.shape[3] != 3 or str(b.dtype) not in ("uint8", "torch.uint8"):
            raise ValueError("luma_grids: frames must be (H, W, 3) uint8, got %s %s at block %d" % (tuple(b.shape[1:]), b.dtype, i))
        if tuple(b.shape[1:]) != shape:
            raise ValueError("luma_grids: frame %d is %dx%d, the first frame %dx%d" % (i, b.shape[2], b.shape[1], shape[1], shape[0]))
    sums = np.concatenate([_grid_block(b, gh, gw, device) for b in blocks])
    return sums, cell_counts(shape[0], shape[1], (gh, gw))


def cut_scores(sums, counts):
    """n - 1 float64 scores of the consecutive pairs of a clip from its luminance grids: the zero-mean normalised cross-correlation of
    the two grids' cell means (sum / (256 * count)) over the cells.  Two flat grids (zero variance both) score 1.0, a flat one against a
    textured one 0.0."""
    sums, counts = np.asarray(sums), np.asarray(counts)
    if sums.ndim != 3 or sums.shape[1:] != counts.shape:
        raise ValueError("cut_scores: sums must be (n, GH, GW) and counts (GH, GW), got %s and %s" % (sums.shape, counts.shape))
    mean = sums.astype(np.float64) / (256.0 * counts.astype(np.float64))
    dev = mean.reshape(len(mean), -1)
    dev = dev - dev.mean(axis=1, keepdims=True)
    var = (dev * dev).sum(axis=1)
    out = np.empty(max(len(dev) - 1, 0), np.float64)
    for t in range(len(out)):
        va, vb = var[t], var[t + 1]
        if va == 0.0 and vb == 0.0:
            out[t] = 1.0
        elif va == 0.0 or vb == 0.0:
            out[t] = 0.0
        else:
            out[t] = float((dev[t] * dev[t + 1]).sum() / np.sqrt(va * vb))
    return out


def detect_cuts(scores, threshold=CUT_DEFAULTS["threshold"], margin=CUT_DEFAULTS["margin"], radius=CUT_DEFAULTS["radius"],
                min_shot_frames=CUT_DEFAULTS["min_shot_frames"]):
    """Sorted first-frame indices of the new shots of a clip with these pair scores.  Pair t (frames t, t + 1) is a candidate iff
    scores[t] < threshold and the median of the scores at distance 1..radius from t (t itself excluded, clipped to the clip) exceeds
    scores[t] by at least margin; a pair without a neighbour is never one.  Candidates are taken in ascending (score, t) order, and one
    is accepted iff both shots it creates - against the cuts accepted so far and the clip's ends - have min_shot_frames frames."""
    if int(min_shot_frames) < 2:
        raise ValueError("detect_cuts: min_shot_frames must be at least 2 (a shot needs a flow pair), got %d" % int(min_shot_frames))
    if int(radius) < 1:
        raise ValueError("detect_cuts: radius must be at least 1, got %d" % int(radius))
    s = np.asarray(scores, np.float64).reshape(-1)
    n = len(s) + 1
    cands = []
    for t in range(len(s)):
        near = np.concatenate([s[max(t - int(radius), 0):t], s[t + 1:t + 1 + int(radius)]])
        if len(near) and s[t] < threshold and np.median(near) - s[t] >= margin:
            cands.append((float(s[t]), t))
    cuts = []
    for _, t in sorted(cands):
        c = t + 1
        before = max([b for b in cuts if b < c] + [0])
        after = min([b for b in cuts if b > c] + [n])
        if c - before >= int(min_shot_frames) and after - c >= int(min_shot_frames):
            cuts.append(c)
    return sorted(cuts)


def plan_shots(n, cuts):
    """[(start, stop)] of the shots of an n-frame clip cut at `cuts`, the first-frame indices of the new shots: strictly increasing
    integers in 1..n-1, every shot at least 2 frames (a shot needs a flow pair).  ValueError naming the cut and the shot otherwise."""
    n = int(n)
    out, start = [], 0
    for k, c in enumerate(list(cuts)):
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError("plan_shots: cut %d is %r: cuts are integer first-frame indices of new shots" % (k, c))
        c = int(c)
        if c < 1 or c > n - 1:
            raise ValueError("plan_shots: cut %d at frame %d is outside 1..%d (a clip of %d frames)" % (k, c, n - 1, n))
        if k and c <= start:
            raise ValueError("plan_shots: cut %d at frame %d does not follow cut %d at frame %d: cuts must be strictly increasing" % (k, c, k - 1, start))
        if c - start < 2:
            raise ValueError("plan_shots: cut %d at frame %d leaves shot %d (frames %d..%d) with %d frame: a shot needs at least 2"
                             % (k, c, k, start, c - 1, c - start))
        out.append((start, c))
        start = c
    if n - start < 2:
        if not out:
            raise ValueError("plan_shots: a clip needs at least 2 frames, got %d" % n)
        raise ValueError("plan_shots: cut %d at frame %d leaves shot %d (frames %d..%d) with %d frame: a shot needs at least 2"
                         % (len(out) - 1, start, len(out), start, n - 1, n - start))
    out.append((start, n))
    return out


def cut_pairs(shots):
    """The pairs (t, t + 1), named by t, that straddle a cut."""
    return [b - 1 for _, b in shots[:-1]]


# ---------------------------------------------------------------------------------------------
def parse_grid(text):
    try:
        gh, gw = (int(v) for v in str(text).lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("expected GHxGW, e.g. 16x16, got %r" % text)
    if not (1 <= gh <= 64 and 1 <= gw <= 64):
        raise argparse.ArgumentTypeError("grid sides must be 1..64, got %r" % text)
    return gh, gw


def add_cut_arguments(p):
    """The four policy knobs, shared by this CLI, deflicker.py and run_pipeline.py."""
    p.add_argument("--cut_threshold", type=float, default=CUT_DEFAULTS["threshold"], help="a pair is a cut candidate when its score is below this")
    p.add_argument("--cut_margin", type=float, default=CUT_DEFAULTS["margin"], help="... and lower than the median of its neighbours by at least this")
    p.add_argument("--cut_radius", type=int, default=CUT_DEFAULTS["radius"], help="neighbours: the pairs at distance 1..radius on each side")
    p.add_argument("--min_shot_frames", type=int, default=CUT_DEFAULTS["min_shot_frames"], help="no detected shot is shorter than this (at least 2)")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="score the consecutive frame pairs of a frame folder on the MI355X and list its scene cuts")
    p.add_argument("--frames_dir", type=str, required=True, help="folder of *.png / *.jpg frames")
    p.add_argument("--grid", type=parse_grid, default=GRID, help="luminance grid GHxGW, sides 1..64 (default 16x16)")
    add_cut_arguments(p)
    p.add_argument("--gpu", type=int, default=0)
    return p.parse_args(argv)


def main(argv=None):
    opts = parse_args(argv)
    import torch
    from .neural_filter import read_png
    from .warp_error import list_frames
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: the luminance grids have no CPU path")
    files = list_frames(opts.frames_dir)
    if len(files) < 2:
        raise SystemExit("%d frames (*.jpg / *.png) under %s: a clip needs at least 2" % (len(files), opts.frames_dir))
    frames = []
    for f in files:
        img = read_png(str(f))
        if img.dtype != np.uint8:
            raise SystemExit("%s: only 8-bit images are handled" % f)
        frames.append(img)
    try:
        sums, counts = luma_grids(frames, opts.grid, device=opts.gpu)
        scores = cut_scores(sums, counts)
        cuts = detect_cuts(scores, opts.cut_threshold, opts.cut_margin, opts.cut_radius, opts.min_shot_frames)
        shots = plan_shots(len(frames), cuts)
    except ValueError as e:
        raise SystemExit("%s: %s" % (opts.frames_dir, e))
    print(json.dumps({"frames": len(frames), "grid": [int(v) for v in sums.shape[1:]], "scores": [float(v) for v in scores], "cuts": cuts,
                      "shots": [list(s) for s in shots], "cut_threshold": opts.cut_threshold, "cut_margin": opts.cut_margin,
                      "cut_radius": opts.cut_radius, "min_shot_frames": opts.min_shot_frames}))
    return 0


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import shots as _s
        sys.exit(_s.main())
    sys.exit(main())
