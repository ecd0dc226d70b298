"""Fidelity report: PSNR and SSIM between two uint8 RGB sequences of one size, per frame and per clip, computed on the device
(include/atlasfit.h af_fidelity, csrc/fidelity.hip).  E_warp (warp_error.py) measures temporal stability alone and a
blurred output lowers it; these say how far a result moved from the frames it should preserve.

    python all-in-one-deflicker_amd/fidelity.py --vid_name <name> [--root data/test/] [--results results] [--reference_dir D]
        [--ssim_window 7] [--gpu 0]

Sequences compared, each if it exists: <results>/<vid>/neural_filter/output and <results>/<vid>/final/output against the input frames
<root>/<vid>/*.png|jpg; with --reference_dir (a clean clip: a processed video's source, or the clip flicker.py flickered) also the input,
the filtered and the final frames against it.  A sequence whose size differs from the input's (stage_1/output) is listed as skipped with
its size: nothing is resized.  Prints one line per comparison and writes <results>/<vid>/fidelity.json (layout: report()).

The PSNR is skimage.metrics.peak_signal_noise_ratio's over the whole RGB frame, 10 log10(255^2 * 3 * pixels / SSE), from the exact integer
SSE of the device.  The SSIM is skimage.metrics.structural_similarity's at its defaults for uint8 (uniform 7 x 7 window, sample covariance,
K1 0.01, K2 0.03, data range 255, channel_axis: the mean of the three channels), every window that lies wholly inside the frame; the
device computes it from exact integer window sums in one fixed order of fp64 operations, so it equals a numpy restatement bit for bit.
No Gaussian window, no MS-SSIM, no perceptual distance."""
import argparse
import json
import math
import os
import sys
from pathlib import Path

import numpy as np

if __package__:      # run as a script this file only re-imports itself as part of the package (below)
    from ._residence import Host, one_device

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_WINDOW = 7
MIN_WINDOW, MAX_WINDOW, MAX_SIDE = 3, 15, 16384
COMPARED = ("neural_filter", "final")      # the stages of warp_error.STAGES that are compared with the input


def check_window(win, what="fidelity"):
    """win as an int, or ValueError: an odd integer in 3..15."""
    if isinstance(win, bool) or not isinstance(win, (int, np.integer)) or not MIN_WINDOW <= int(win) <= MAX_WINDOW or int(win) % 2 == 0:
        raise ValueError("%s: win must be an odd integer in %d..%d, got %r" % (what, MIN_WINDOW, MAX_WINDOW, win))
    return int(win)


def _check_pair(a, b, win, what, res):
    """(n, h, w, squeeze) of two sequences (N, H, W, 3) or frames (H, W, 3) of one shape, uint8."""
    dt = "torch.uint8" if res.on_device else "uint8"
    for name, x in (("a", a), ("b", b)):
        if not hasattr(x, "shape") or len(x.shape) not in (3, 4) or x.shape[-1] != 3 or str(x.dtype) != dt:
            raise ValueError("%s: %s must be (H, W, 3) or (N, H, W, 3) uint8, got %s %s" % (what, name, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x).__name__)))
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("%s: a is %s, b %s" % (what, tuple(a.shape), tuple(b.shape)))
    squeeze = len(a.shape) == 3
    n, h, w = (1,) + tuple(a.shape[:2]) if squeeze else tuple(a.shape[:3])
    if n < 1:
        raise ValueError("%s: no frames" % what)
    for name, v in (("height", h), ("width", w)):
        if not win <= v <= MAX_SIDE:
            raise ValueError("%s: the %s must be in win..%d (win %d), got %d" % (what, name, MAX_SIDE, win, v))
    return int(n), int(h), int(w)


def _fidelity(what, res, a, b, win, want_map, want_ssim):
    """One af_fidelity call over a residence (_residence.py); the per-frame sums are host memory on either side."""
    from .atlasfit import load_library, _util_chk, _ptr
    win = check_window(win, what)
    res = res or one_device([a, b], "%s: the frames must be CUDA tensors on one device (host arrays go through frame_fidelity)" % what)
    n, h, w = _check_pair(a, b, win, what, res)
    if want_map and not want_ssim:
        raise ValueError("%s: the map is the SSIM's: want_map needs want_ssim" % what)
    x, y = res.contiguous(a), res.contiguous(b)
    sse = np.zeros((n, 3), np.uint64)
    ssim = np.zeros((n, 3), np.float64) if want_ssim else None
    smap = res.empty((n, h - win + 1, w - win + 1, 3), "float64") if want_map else None
    res.sync()
    _util_chk(load_library().af_fidelity(res.ordinal, res.ptr(x), res.ptr(y), n, h, w, win, _ptr(sse), _ptr(ssim), res.ptr(smap), res.on_device))
    out = {"sse": sse, "ssim": ssim}
    if want_map:
        out["map"] = smap
    return out


def frame_fidelity(a, b, win=DEFAULT_WINDOW, want_map=False, want_ssim=True, device=0):
    """a, b: numpy (H, W, 3) or (N, H, W, 3) uint8 of one shape, through host pointers (the library stages the call on GPU `device`).
    Returns {"sse": uint64 (N, 3), "ssim": float64 (N, 3)} and with want_map "map": float64 (N, H - win + 1, W - win + 1, 3), the SSIM of
    every window; want_ssim False: the SSE alone ("ssim" None)."""
    return _fidelity("frame_fidelity", Host(device), a, b, win, want_map, want_ssim)


def frame_fidelity_device(a, b, win=DEFAULT_WINDOW, want_map=False, want_ssim=True):
    """frame_fidelity on CUDA tensors (device pointers, no host copy of a frame): "sse" and "ssim" are numpy arrays (the per-frame sums
    land in host memory), "map" a float64 tensor on the frames' device."""
    return _fidelity("frame_fidelity_device", None, a, b, win, want_map, want_ssim)


def psnr_from_sse(sse, pixels):
    """10 log10(255^2 * 3 * pixels / sum_c sse) in fp64 of one frame's three sums (skimage's PSNR over the whole RGB frame); inf at 0."""
    total = int(sum(int(v) for v in np.asarray(sse).reshape(-1)))
    if total == 0:
        return math.inf
    return 10.0 * math.log10(255.0 * 255.0 * 3.0 * float(pixels) / float(total))


def summarise(sse, ssim, h, w):
    """{"psnr": {"mean", "per_frame", "identical_frames"}, "ssim": {"mean", "per_frame"}} of (N, 3) sums: a frame's SSIM is the mean of its
    three channels (skimage's channel_axis rule); the mean PSNR skips the infinite frames (a == b) and counts them in identical_frames
    (None when every frame is identical).  Infinite frames are written as the JSON token Infinity."""
    sse, ssim = np.asarray(sse).reshape(-1, 3), np.asarray(ssim, np.float64).reshape(-1, 3)
    psnr = [psnr_from_sse(row, int(h) * int(w)) for row in sse]
    finite = [p for p in psnr if math.isfinite(p)]
    per_ssim = [float((float(r[0]) + float(r[1]) + float(r[2])) / 3.0) for r in ssim]
    return {"psnr": {"mean": float(np.mean(finite)) if finite else None, "per_frame": psnr, "identical_frames": len(psnr) - len(finite)},
            "ssim": {"mean": float(np.mean(per_ssim)), "per_frame": per_ssim}}


# ---- the stand-alone report over the chained CLIs' results tree -----------------------------------------------------------------------
def read_u8(path):
    """A frame file as (H, W, 3) uint8 RGB (grey tiled, alpha dropped); anything deeper than 8 bits is a ValueError."""
    from PIL import Image
    im = np.array(Image.open(str(path)))
    if im.dtype != np.uint8:
        raise ValueError("%s: only 8-bit images are handled" % path)
    if im.ndim == 2:
        im = np.tile(im[:, :, None], [1, 1, 3])
    return np.ascontiguousarray(im[:, :, :3])


def frame_size(path):
    from PIL import Image
    with Image.open(str(path)) as im:
        return int(im.size[1]), int(im.size[0])


def plan_comparisons(root, results, vid_name, reference_dir=None):
    """(comparisons, skipped, (h, w)): comparisons = [(name, files a, files b)] in report order, skipped = [{"stage", "path", "height",
    "width", "frames", "reason"}] for every sequence that exists but does not match the input's size or length.  Reads file headers only."""
    from .warp_error import discover_sequences, list_frames
    seqs = {stage: (folder, files) for stage, folder, files in discover_sequences(root, results, vid_name)}
    if "input" not in seqs:
        raise SystemExit("no input frames under %s" % (Path(root) / vid_name))
    inputs = seqs["input"][1]
    hw = frame_size(inputs[0])
    if reference_dir is not None:
        ref = list_frames(reference_dir) if Path(reference_dir).is_dir() else []
        if not ref:
            raise SystemExit("no reference frames (*.jpg / *.png) under %s (--reference_dir)" % reference_dir)
        seqs["reference"] = (Path(reference_dir), ref)
    usable, skipped = {"input": inputs}, []
    for stage, (folder, files) in seqs.items():
        if stage == "input":
            continue
        size = frame_size(files[0])
        reason = None
        if size != hw:
            reason = "size differs from the input's %dx%d (nothing is resized)" % (hw[1], hw[0])
        elif len(files) != len(inputs):
            reason = "%d frames, the input has %d" % (len(files), len(inputs))
        if reason is not None:
            if stage == "reference":
                raise SystemExit("%s: %dx%d, %d frames: %s" % (folder, size[1], size[0], len(files), reason))
            skipped.append({"stage": stage, "path": str(folder), "height": size[0], "width": size[1], "frames": len(files), "reason": reason})
        else:
            usable[stage] = files
    plan = [("%s_vs_input" % s, usable[s], inputs) for s in COMPARED if s in usable]
    if "reference" in usable:
        plan += [("%s_vs_reference" % s, usable[s], usable["reference"]) for s in ("input",) + COMPARED if s in usable]
    return plan, skipped, hw


def measure(files_a, files_b, win=DEFAULT_WINDOW, device=0):
    """summarise() of two file sequences of one size, frame by frame through host pointers."""
    sse, ssim, hw = [], [], None
    for pa, pb in zip(files_a, files_b):
        a, b = read_u8(pa), read_u8(pb)
        if a.shape != b.shape or (hw is not None and a.shape[:2] != hw):
            raise ValueError("%s is %s, %s is %s: a sequence has one size" % (pa, a.shape, pb, b.shape))
        hw = a.shape[:2]
        r = frame_fidelity(a, b, win, device=device)
        sse.append(r["sse"][0])
        ssim.append(r["ssim"][0])
    return summarise(np.stack(sse), np.stack(ssim), hw[0], hw[1])


def report(vid_name, win, hw, measured, skipped):
    """results/<vid>/fidelity.json: {"vid_name", "window", "size": [H, W], "comparisons": {name: summarise() + "frames"}, "skipped": [...]}."""
    return {"vid_name": vid_name, "window": int(win), "size": [int(hw[0]), int(hw[1])],
            "comparisons": {name: dict(rec, frames=len(rec["ssim"]["per_frame"])) for name, rec in measured}, "skipped": list(skipped)}


def run(args, measure_fn=None):
    """measure_fn: a replacement for measure (the host tests')."""
    try:
        win = check_window(args.ssim_window, "--ssim_window")
    except ValueError as e:
        raise SystemExit(str(e))
    plan, skipped, hw = plan_comparisons(args.root, args.results, args.vid_name, args.reference_dir)
    measured = []
    for name, fa, fb in plan:
        rec = (measure_fn or measure)(fa, fb, win, args.gpu)
        measured.append((name, rec))
        p = rec["psnr"]["mean"]
        print("%-28s PSNR %s dB  SSIM %.6f  (%d frames, %dx%d, window %d)" % (name, "inf" if p is None else "%.4f" % p, rec["ssim"]["mean"],
                                                                              len(fa), hw[1], hw[0], win))
    for s in skipped:
        print("%-28s skipped: %dx%d, %s" % (s["stage"], s["width"], s["height"], s["reason"]))
    rep = report(args.vid_name, win, hw, measured, skipped)
    out = Path(args.results) / args.vid_name / "fidelity.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        json.dump(rep, f, indent=2)
    print("wrote", out)
    return rep


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="PSNR and SSIM of the stages of a processed clip against its input frames, and against a clean reference clip")
    p.add_argument("--vid_name", type=str, required=True)
    p.add_argument("--root", type=str, default="data/test/")
    p.add_argument("--results", type=str, default="results")
    p.add_argument("--reference_dir", type=str, default=None, help="folder of clean frames of the input's size and length: also compare input, filtered and final with it")
    p.add_argument("--ssim_window", type=int, default=DEFAULT_WINDOW, help="side of the uniform SSIM window, odd, 3..15 (default 7, skimage's)")
    p.add_argument("--gpu", type=int, default=0)
    return p.parse_args(argv)


def _cli(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import fidelity as _f
        _f._cli()
        sys.exit(0)
    _cli()
