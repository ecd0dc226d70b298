"""Flicker report of a processed clip: the warping error E_warp (Lai et al., ECCV 2018) of every sequence the pipeline wrote, one
line per stage (include/atlasfit.h af_warp_error_pair; the building blocks are the reference's src/models/utils.py:478-572).

    python all-in-one-deflicker_amd/warp_error.py --vid_name <name> [--root data/test/] [--results results] [--geometry exact|reference] [--gpu 0]

Sequences measured, each if it exists: the input frames <root>/<vid>/*.png|jpg, <results>/<vid>/stage_1/output,
<results>/<vid>/neural_filter/output and <results>/<vid>/final/output (frames in sorted file order).  Pair t of every sequence uses the
RAFT flows src/preprocess_optical_flow.py wrote for input frames t and t+1, <root>/<vid>_flow/{fn1}_{fn2}.npy and {fn2}_{fn1}.npy,
resized on the GPU to the sequence's resolution with the vector scales of resize_flow (unwrap_utils.py:33-38).  Frames are read as
read_img does (RGB, float32 / 255, utils.py:211-232).  Writes <results>/<vid>/warp_error.json (layout: report()).

Geometry: "exact" (default) samples with align_corners=True, so zero flow is the identity; "reference" is what the reference's
flow_warping computes under torch >= 1.3 (grid_sample's align_corners=False default).  DESIGN.md §2.8.

stage1.py / stage1_seg.py --warp_error write <iter>/warp_error.json (layout: eval_record()) at each evaluation from the handle
(AtlasFit.warp_error: the uploaded frames and the reconstruction, with the uploaded flows).
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
GEOMETRIES = {"exact": True, "reference": False}
STAGES = (("input", None), ("stage_1", ("stage_1", "output")), ("neural_filter", ("neural_filter", "output")), ("final", ("final", "output")))


def parse_geometry(name):
    """'exact' -> align_corners True, 'reference' -> False; anything else is a ValueError."""
    try:
        return GEOMETRIES[name]
    except KeyError:
        raise ValueError("geometry must be one of %s, got %r" % (", ".join(GEOMETRIES), name)) from None


def geometry_name(align_corners):
    return "exact" if align_corners else "reference"


def list_frames(folder):
    """The frames of a sequence folder in the loaders' order: sorted *.jpg + *.png."""
    folder = Path(folder)
    return sorted(list(folder.glob("*.jpg")) + list(folder.glob("*.png")))


def flow_pairs(input_files, flow_dir):
    """[(flow12 path, flow21 path)] of the consecutive input frames, named as src/preprocess_optical_flow.py writes them.
    FileNotFoundError naming the first missing file."""
    flow_dir = Path(flow_dir)
    out = []
    for a, b in zip(input_files[:-1], input_files[1:]):
        f12, f21 = flow_dir / ("%s_%s.npy" % (a.name, b.name)), flow_dir / ("%s_%s.npy" % (b.name, a.name))
        for p in (f12, f21):
            if not p.exists():
                raise FileNotFoundError("optical flow %s missing: run the reference's src/preprocess_optical_flow.py first" % p)
        out.append((f12, f21))
    return out


def discover_sequences(root, results, vid_name):
    """[(stage, folder, frame files)] of every stage folder that exists and holds at least two frames, in pipeline order."""
    found = []
    for stage, sub in STAGES:
        folder = Path(root) / vid_name if sub is None else Path(results) / vid_name / sub[0] / sub[1]
        files = list_frames(folder) if folder.is_dir() else []
        if len(files) >= 2:
            found.append((stage, folder, files))
    return found


def _record(mean, per_pair):
    return {"mean": float(mean), "per_pair": [float(v) for v in per_pair]}


def eval_record(align_corners, input_result, reconstruction_result):
    """<iter>/warp_error.json of the stage-1 CLIs: {"geometry", "align_corners", "input": {"mean", "per_pair"}, "reconstruction": {...}}."""
    return {"geometry": geometry_name(align_corners), "align_corners": int(bool(align_corners)),
            "input": _record(*input_result), "reconstruction": _record(*reconstruction_result)}


def write_eval_json(af, eval_dir, align_corners=True):
    """Measure the uploaded video and the reconstruction of an AtlasFit and write <eval_dir>/warp_error.json."""
    rec = eval_record(align_corners, af.warp_error("input", align_corners), af.warp_error("reconstruction", align_corners))
    with open(os.path.join(str(eval_dir), "warp_error.json"), "w") as f:
        json.dump(rec, f, indent=2)
    return rec


def report(vid_name, align_corners, sequences):
    """results/<vid>/warp_error.json: {"vid_name", "geometry", "align_corners", "sequences": {stage: {"path", "frames", "height", "width",
    "mean", "per_pair"}}} (sequences: [(stage, path, frames, (h, w), mean, per_pair)])."""
    seqs = {}
    for stage, path, frames, (h, w), mean, per_pair in sequences:
        seqs[stage] = dict(path=str(path), frames=int(frames), height=int(h), width=int(w), **_record(mean, per_pair))
    return {"vid_name": vid_name, "geometry": geometry_name(align_corners), "align_corners": int(bool(align_corners)), "sequences": seqs}


def read_frame(path):
    """read_img (utils.py:211-232): RGB, np.float32(img) / 255."""
    from PIL import Image
    im = np.array(Image.open(str(path)))
    if im.ndim == 2:
        im = np.tile(im[:, :, None], [1, 1, 3])
    return np.ascontiguousarray(np.float32(im[:, :, :3]) / 255.0)


def measure_sequence(files, pairs, align_corners=True, device=0):
    """(mean, per_pair, (h, w)) of one frame sequence; pair t uses pairs[t]'s flows resized to the sequence's resolution on the GPU."""
    import torch
    from .atlasfit import resize_bilinear_device, warp_error_pair
    dev = torch.device("cuda", device)
    n = min(len(files), len(pairs) + 1)
    if n < 2:
        raise ValueError("a sequence needs at least two frames with flows")
    frames = [torch.from_numpy(read_frame(files[0])).to(dev)]
    h, w = frames[0].shape[:2]

    def flow(p):
        f = torch.from_numpy(np.ascontiguousarray(np.load(str(p)).astype(np.float32))).to(dev)
        if f.shape[0] == h and f.shape[1] == w:
            return f
        r = torch.empty((h, w, 2), device=dev)
        resize_bilinear_device(f, r, h, w, 2, 1, 0, scale=(h / f.shape[0], w / f.shape[1]), device=device)   # resize_flow, :33-38
        return r

    per = []
    for t in range(n - 1):
        nxt = torch.from_numpy(read_frame(files[t + 1])).to(dev)
        if tuple(nxt.shape[:2]) != (h, w):
            raise ValueError("%s: frame size %s differs from the sequence's %s" % (files[t + 1], tuple(nxt.shape[:2]), (h, w)))
        per.append(warp_error_pair(frames[-1], nxt, flow(pairs[t][0]), flow(pairs[t][1]), align_corners=align_corners, device=device))
        frames = [nxt]
    return float(np.mean(per)), per, (h, w)


def run(args):
    align = parse_geometry(args.geometry)
    root, results = Path(args.root), Path(args.results)
    seqs = discover_sequences(root, results, args.vid_name)
    if not seqs or seqs[0][0] != "input":
        raise SystemExit("no input frames under %s" % (root / args.vid_name))
    pairs = flow_pairs(seqs[0][2], root / ("%s_flow" % args.vid_name))
    measured = []
    for stage, folder, files in seqs:
        mean, per, hw = measure_sequence(files, pairs, align, args.device_ordinal)
        measured.append((stage, folder, len(per) + 1, hw, mean, per))
        print("%-14s E_warp %.6f  (%d pairs, %dx%d, %s)" % (stage, mean, len(per), hw[1], hw[0], geometry_name(align)))
    rep = report(args.vid_name, align, measured)
    out = results / args.vid_name / "warp_error.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        json.dump(rep, f, indent=2)
    print("wrote", out)
    return rep


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="warping error (flicker) of every stage of a processed clip")
    p.add_argument("--vid_name", type=str, required=True)
    p.add_argument("--root", type=str, default="data/test/")
    p.add_argument("--results", type=str, default="results")
    p.add_argument("--geometry", type=str, default="exact", choices=sorted(GEOMETRIES))
    p.add_argument("--gpu", type=int, default=0)
    args = p.parse_args(argv)
    args.device_ordinal = args.gpu
    return args


def _cli(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import warp_error as _w
        _w._cli()
        sys.exit(0)
    _cli()
