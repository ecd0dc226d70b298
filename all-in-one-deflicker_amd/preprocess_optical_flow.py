"""Drop-in for the reference's flow precompute `src/preprocess_optical_flow.py`: same flags, same input folder, same output files —
`<vid>_flow/{fn1}_{fn2}.npy` and `{fn2}_{fn1}.npy`, float32 (Hp, Wp, 2) at the padded size, for every neighbouring pair of the sorted
`*.*g` frames — but RAFT runs on this package's MI355X path (aiod_amd.RAFT) in fp32, every frame goes through the encoders once, and
only PIL and torch are needed (no cv2, tqdm).

    python <this repo>/all-in-one-deflicker_amd/preprocess_optical_flow.py --vid-path data/test/<vid> [--max_long_edge 2000] [--gpu 0]
        [--model pretrained_weights/raft-things.pth]

A pair is skipped exactly when the reference skips it (its `overwrite=False` rule: it computes only when NEITHER file exists).
Frames whose long edge exceeds --max_long_edge would need the reference's cv2.INTER_AREA resize, which this package does not have:
the CLI exits with a message instead of resizing differently."""
import argparse
import os
import sys
from pathlib import Path

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Preprocess image sequence (RAFT flow on the MI355X)")
    p.add_argument("--vid-path", type=Path, default=Path("./data/"), help="folder to process")
    p.add_argument("--max_long_edge", type=int, default=2000, help="maximum image dimension to process without resizing")
    p.add_argument("--gpu", type=int, default=0, help="gpu id")
    p.add_argument("--model", type=str, default="pretrained_weights/raft-things.pth", help="the RAFT checkpoint")
    return p.parse_args(argv)


def load_image(fn, max_long_edge):
    """RAFTWrapper.load_image before the tensor conversion: the decoded uint8 array; refuses frames that would be resized."""
    import numpy as np
    from PIL import Image
    img = np.array(Image.open(fn)).astype(np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise SystemExit("%s: expected an RGB image, got an array of shape %s" % (fn, img.shape))
    check_long_edge(fn, img.shape[0], img.shape[1], max_long_edge)
    return img


def check_long_edge(fn, h, w, max_long_edge):
    """Refuse a frame the reference would shrink before RAFT (RAFTWrapper.load_image)."""
    if max(h, w) / max_long_edge > 1:
        raise SystemExit("%s is %dx%d: longer than --max_long_edge %d.  The reference would shrink it with cv2.INTER_AREA, which this "
                         "package does not implement; raise --max_long_edge or resize the frames first" % (fn, w, h, max_long_edge))


def plan(files, out_flow_dir):
    """[(i, path12, path21)] of the pairs the reference would compute: those where neither output exists."""
    todo = []
    for i in range(len(files) - 1):
        p12 = out_flow_dir / ("%s_%s.npy" % (files[i].name, files[i + 1].name))
        p21 = out_flow_dir / ("%s_%s.npy" % (files[i + 1].name, files[i].name))
        if not p12.exists() and not p21.exists():
            todo.append((i, p12, p21))
    return todo


def preprocess(args, make_flow=None):
    """make_flow(h, w) -> an object with encode(slot, image) and flow_slots(pairs) (aiod_amd.RAFT by default; the tests pass a stub)."""
    import numpy as np
    files = sorted(args.vid_path.glob("*.*g"))
    out_flow_dir = args.vid_path.parent / ("%s_flow" % args.vid_path.name)
    out_flow_dir.mkdir(exist_ok=True)
    todo = plan(files, out_flow_dir)
    raft, slot_of = None, {}
    for n, (i, p12, p21) in enumerate(todo):
        for j in (i, i + 1):
            if j in slot_of:
                continue
            img = load_image(str(files[j]), args.max_long_edge)
            if raft is None:
                raft = make_flow(img.shape[0], img.shape[1])
            elif img.shape[:2] != (raft.h, raft.w):
                raise SystemExit("frame %s is %dx%d, the first frame %dx%d" % (files[j], img.shape[1], img.shape[0], raft.w, raft.h))
            slot_of = {k: s for k, s in slot_of.items() if k == j - 1}      # two live frames: the slot not holding frame j - 1 is free
            slot_of[j] = 1 - slot_of.get(j - 1, 1)
            raft.encode(slot_of[j], img)
        a, b = slot_of[i], slot_of[i + 1]
        if getattr(raft, "capacity", 1) >= 2:
            f12, f21 = raft.flow_slots([(a, b), (b, a)])
        else:
            f12, f21 = raft.flow_slots([(a, b)])[0], raft.flow_slots([(b, a)])[0]
        np.save(p12, np.asarray(f12, np.float32))
        np.save(p21, np.asarray(f21, np.float32))
        print("computing flow: %d / %d" % (n + 1, len(todo)))
    return len(todo)


def main(argv=None):
    args = parse_args(argv)
    import torch
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    import aiod_amd
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: the native flow precompute has no CPU path")
    if not os.path.exists(args.model):
        raise SystemExit("RAFT checkpoint %s not found (--model)" % args.model)
    ckpt = torch.load(args.model, map_location="cpu")

    def make_flow(h, w):
        r = aiod_amd.RAFT(h, w, capacity=2, device=args.gpu)
        r.load_state_dict(ckpt)
        return r
    preprocess(args, make_flow)
    return 0


if __name__ == "__main__":
    sys.exit(main())
