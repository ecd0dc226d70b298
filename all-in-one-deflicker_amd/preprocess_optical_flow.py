"""Drop-in for the reference's flow precompute `src/preprocess_optical_flow.py`: same flags, same input folder, same output files —
`<vid>_flow/{fn1}_{fn2}.npy` and `{fn2}_{fn1}.npy`, float32 (Hp, Wp, 2) at the padded size, for every neighbouring pair of the sorted
`*.*g` frames — but RAFT runs on this package's MI355X path (aiod_amd.RAFT) in fp32, every frame goes through the encoders once, and
only PIL and torch are needed (no cv2, tqdm).

    python <this repo>/all-in-one-deflicker_amd/preprocess_optical_flow.py --vid-path data/test/<vid> [--max_long_edge 2000] [--gpu 0]
        [--model pretrained_weights/raft-things.pth] [--flow_precision fp32|fp16]

A pair is skipped exactly when the reference skips it (its `overwrite=False` rule: it computes only when NEITHER file exists).
A frame whose long edge exceeds --max_long_edge is shrunk before RAFT as RAFTWrapper.load_image shrinks it: to `shrink_size` (the
reference's own float floor division) with cv2.INTER_AREA's arithmetic on the device (af_resize_area); the saved flows
then have the padded shrunk size, as the reference's do.  `preprocess` without a shrinker (a caller that injects none) refuses such a
frame with a message instead of resizing differently."""
import argparse
import os
import sys
from pathlib import Path

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Preprocess image sequence (RAFT flow on the MI355X)")
    p.add_argument("--vid-path", type=Path, default=Path("./data/"), help="folder to process")
    p.add_argument("--max_long_edge", type=int, default=2000, help="maximum image dimension to process without resizing: a longer frame is shrunk to it (INTER_AREA, on the device) before RAFT")
    p.add_argument("--gpu", type=int, default=0, help="gpu id")
    p.add_argument("--model", type=str, default="pretrained_weights/raft-things.pth", help="the RAFT checkpoint")
    p.add_argument("--flow_precision", choices=("fp32", "fp16"), default="fp32",
                   help="(extension) fp16: the encoders and the update block in the fp16 arithmetic the reference runs on a GPU (autocast); fp32: what it computes on a CPU")
    return p.parse_args(argv)


def decode_image(fn):
    """The decoded uint8 RGB array of a frame file."""
    import numpy as np
    from PIL import Image
    img = np.array(Image.open(fn)).astype(np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise SystemExit("%s: expected an RGB image, got an array of shape %s" % (fn, img.shape))
    return img


def load_image(fn, max_long_edge):
    """RAFTWrapper.load_image before the tensor conversion, without a shrinker: the decoded uint8 array; refuses frames that would be
    resized."""
    img = decode_image(fn)
    check_long_edge(fn, img.shape[0], img.shape[1], max_long_edge)
    return img


def shrink_image(fn, img, max_long_edge, shrink):
    """RAFTWrapper.load_image's resize: img through shrink(img, new_h, new_w) when it is longer than max_long_edge, else img itself."""
    import numpy as np
    try:
        small = shrink_size(img.shape[0], img.shape[1], max_long_edge, name=fn)
    except ValueError as e:
        raise SystemExit(str(e))
    if small is None:
        return img
    out = np.asarray(shrink(img, small[0], small[1]))
    if out.dtype != np.uint8 or out.shape != (small[0], small[1], 3):
        raise SystemExit("%s: the shrinker returned %s %s, expected uint8 %s" % (fn, out.shape, out.dtype, (small[0], small[1], 3)))
    return out


def shrink_size(h, w, max_long_edge, name="frame"):
    """(new_h, new_w) RAFTWrapper.load_image shrinks an h x w frame to before RAFT, or None when it does not (raft_wrapper.py:37-44).
    The expressions are the reference's, float floor division and its quirks included: 4096 wide at 2000 gives 1999, and 9x10 at 9
    gives 8x8.  A result with a zero side is a ValueError naming the frame."""
    if max_long_edge < 1:
        raise ValueError("--max_long_edge must be positive, got %d" % max_long_edge)
    factor = max(w, h) / max_long_edge
    if factor <= 1:
        return None
    new_w = int(w // factor)
    new_h = int(h // factor)
    if new_h < 1 or new_w < 1:
        raise ValueError("%s is %dx%d: shrinking it to --max_long_edge %d would leave %dx%d" % (name, w, h, max_long_edge, new_w, new_h))
    return new_h, new_w


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


def preprocess(args, make_flow=None, shrink=None):
    """make_flow(h, w) -> an object with encode(slot, image) and flow_slots(pairs) (main passes aiod_amd.RAFT; the tests pass a stub).
    shrink(img_u8, new_h, new_w) -> uint8 array: the INTER_AREA resize of a frame longer than --max_long_edge (main passes the device
    kernel); every such frame goes through it once, before encode, and RAFT is opened at the shrunk size.  With shrink None such a
    frame is refused."""
    import numpy as np
    files = sorted(args.vid_path.glob("*.*g"))
    out_flow_dir = args.vid_path.parent / ("%s_flow" % args.vid_path.name)
    out_flow_dir.mkdir(exist_ok=True)
    todo = plan(files, out_flow_dir)
    raft, slot_of, first = None, {}, None
    for n, (i, p12, p21) in enumerate(todo):
        for j in (i, i + 1):
            if j in slot_of:
                continue
            img = load_image(str(files[j]), args.max_long_edge) if shrink is None else decode_image(str(files[j]))
            size = img.shape[:2]
            if first is None:
                first = size
            elif size != first:                                             # the sizes as decoded: equal frames shrink to equal sizes
                raise SystemExit("frame %s is %dx%d, the first frame %dx%d" % (files[j], size[1], size[0], first[1], first[0]))
            if shrink is not None:
                img = shrink_image(str(files[j]), img, args.max_long_edge, shrink)
            if raft is None:
                raft = make_flow(img.shape[0], img.shape[1])
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
        r = aiod_amd.RAFT(h, w, capacity=2, device=args.gpu, precision=args.flow_precision)
        r.load_state_dict(ckpt)
        return r

    def shrink(img, h, w):
        return aiod_amd.resize_area(img, h, w, device=args.gpu)
    preprocess(args, make_flow, shrink)
    return 0


if __name__ == "__main__":
    sys.exit(main())
