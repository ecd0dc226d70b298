"""Seeded synthetic flicker: a clean clip plus a random gain and offset per frame and channel, so that fidelity.py has a ground truth to
measure a deflicker result against.

    python all-in-one-deflicker_amd/flicker.py --frames_dir D --out D2 [--kind local] [--strength 0.1] [--grid 4x4] [--seed 0] [--gpu 0]

Frame f gets a gain plane a and an offset plane b, each (gh, gw, 3) float32: `global` 1 x 1 (the whole frame brightens or darkens),
`local` the `grid` (a smooth field: the planes are sampled bilinearly at the pixel centres).  The draws come from
np.random.default_rng(seed) in this order: for f = 0, 1, ...: a = rng.uniform(-strength, strength, (gh, gw, 3)), then
b = rng.uniform(-64 strength, 64 strength, (gh, gw, 3)), both rounded to float32.  The planes are applied by guided.guided_apply, so the
output bytes are af_guided_apply's contract: out = clamp(rint(F + (a F + b)), 0, 255).  Writes %05d.png and flicker.json (the parameters).

The distributions are policy for a test bed, not a model of real flicker."""
import argparse
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("global", "local")
OFFSET_LEVELS = 64.0      # the offset range in 8-bit levels at strength 1


def check_flicker(kind, strength, grid):
    """(kind, strength, (gh, gw)) or ValueError: kind global | local, strength finite and >= 0, grid two integers in 1..64."""
    if kind not in KINDS:
        raise ValueError("synth_flicker: kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    try:
        s = float(strength)
    except (TypeError, ValueError):
        raise ValueError("synth_flicker: strength must be a number, got %r" % (strength,))
    if not np.isfinite(s) or s < 0:
        raise ValueError("synth_flicker: strength must be finite and >= 0, got %r" % (strength,))
    try:
        gh, gw = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError("synth_flicker: grid must be two integers (rows, columns), got %r" % (grid,))
    if not (1 <= gh <= 64 and 1 <= gw <= 64):
        raise ValueError("synth_flicker: grid must be two integers in 1..64, got %r" % (grid,))
    return kind, s, (gh, gw)


def draw_planes(n, kind="global", strength=0.1, grid=(4, 4), seed=0):
    """[(a, b)] for n frames, each (gh, gw, 3) float32, in the documented order of draws."""
    kind, s, (gh, gw) = check_flicker(kind, strength, grid)
    if kind == "global":
        gh = gw = 1
    rng = np.random.default_rng(seed)
    planes = []
    for _ in range(int(n)):
        a = rng.uniform(-s, s, (gh, gw, 3)).astype(np.float32)
        b = rng.uniform(-OFFSET_LEVELS * s, OFFSET_LEVELS * s, (gh, gw, 3)).astype(np.float32)
        planes.append((a, b))
    return planes


def synth_flicker(frames, kind="global", strength=0.1, grid=(4, 4), seed=0, device=0):
    """frames: a sequence of (H, W, 3) uint8 numpy arrays (or one (N, H, W, 3) array), each at least as large as the grid.  Returns
    (flickered frames as one (N, H, W, 3) uint8 array, [(a, b)] the planes of every frame)."""
    from .guided import guided_apply
    frames = list(frames)
    if not frames:
        raise ValueError("synth_flicker: no frames")
    planes = draw_planes(len(frames), kind, strength, grid, seed)
    out = []
    for i, (f, (a, b)) in enumerate(zip(frames, planes)):
        if not hasattr(f, "shape") or len(f.shape) != 3 or f.shape[2] != 3 or str(f.dtype) != "uint8":
            raise ValueError("synth_flicker: frame %d must be (H, W, 3) uint8, got %s %s" % (i, tuple(getattr(f, "shape", ())), getattr(f, "dtype", type(f).__name__)))
        if f.shape[0] < a.shape[0] or f.shape[1] < a.shape[1]:
            raise ValueError("synth_flicker: frame %d (%dx%d) is smaller than the grid (%dx%d)" % (i, f.shape[1], f.shape[0], a.shape[1], a.shape[0]))
        out.append(guided_apply(f, a, b, device=device))
    return np.stack(out), planes


def parse_grid(text):
    try:
        gh, gw = (int(v) for v in str(text).lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("expected ROWSxCOLUMNS, got %r" % text)
    return gh, gw


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="flicker a clean clip with seeded random gains and offsets (a test bed for fidelity.py)")
    p.add_argument("--frames_dir", type=str, required=True)
    p.add_argument("--out", type=str, required=True)
    p.add_argument("--kind", type=str, default="global", choices=KINDS)
    p.add_argument("--strength", type=float, default=0.1)
    p.add_argument("--grid", type=parse_grid, default=(4, 4), metavar="ROWSxCOLUMNS")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--gpu", type=int, default=0)
    return p.parse_args(argv)


def main(argv=None, apply_fn=None):
    """apply_fn: a replacement for synth_flicker (the host tests')."""
    from PIL import Image
    from .fidelity import read_u8
    from .warp_error import list_frames
    opts = parse_args(argv)
    try:
        check_flicker(opts.kind, opts.strength, opts.grid)
    except ValueError as e:
        raise SystemExit(str(e))
    files = list_frames(opts.frames_dir)
    if not files:
        raise SystemExit("no frames (*.jpg / *.png) under %s" % opts.frames_dir)
    try:
        out, _ = (apply_fn or synth_flicker)([read_u8(f) for f in files], kind=opts.kind, strength=opts.strength, grid=opts.grid, seed=opts.seed, device=opts.gpu)
    except ValueError as e:
        raise SystemExit(str(e))
    os.makedirs(opts.out, exist_ok=True)
    for i, f in enumerate(out):
        Image.fromarray(f).save(os.path.join(opts.out, "%05d.png" % i))
    with open(os.path.join(opts.out, "flicker.json"), "w") as fh:
        json.dump({"frames_dir": opts.frames_dir, "frames": len(files), "kind": opts.kind, "strength": opts.strength, "grid": list(opts.grid),
                   "seed": opts.seed, "offset_levels": OFFSET_LEVELS}, fh, indent=2)
    print("wrote %d flickered frames to %s" % (len(files), opts.out))
    return 0


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import flicker as _f
        sys.exit(_f.main())
    sys.exit(main())
