"""Texture-edit propagation of a trained fg/bg stage 1 (reference: the edit videos of src/models/stage_1/evaluate.py:373-438,
edit_<vid>.mp4 at :525-526): paint on texture_orig1.png (and / or texture_orig2.png) and get the edited video back.

    python all-in-one-deflicker_amd/atlas_edit.py --vid_name <name> [--root data/test/] [--down 1] --edit_fg a.png [--edit_bg b.png] [--out DIR]
                                                  [--size stage1|full|HxW]

Reads the stage-1 checkpoint and config of stage1_seg.py (./results/<vid>/stage_1/{checkpoint,config.json}) and the clip's inputs
(frames, flow, masks: the same loader as stage1_seg.py).  An edit image is a res x res RGB(A) PNG over the layer's window: fg (0, 0, 1),
bg the background mapping area (evaluate.py:235-257); a layer without an edit image uses its unedited atlas texture.  Writes
<out>/%05d.png (default ./results/<vid>/stage_1/edit/) with the reference's truncating uint8 cast.  --size: the edited video at the
stage-1 lattice (default), at the decoded frames' size (full) or at HxW, the nets evaluated at those pixels.  One edit session serves the
whole clip: the textures are uploaded once and the library writes the bytes."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _read_texture(path):
    from PIL import Image
    im = np.array(Image.open(path))
    if im.ndim != 3 or im.shape[2] not in (3, 4) or im.shape[0] != im.shape[1]:
        raise SystemExit("%s: need a square RGB / RGBA image, got %s" % (path, im.shape))
    return (im[:, :, :3].astype(np.float64) / 255.0).astype(np.float32)


def run(args):
    from PIL import Image
    from . import atlasfit as A
    from . import stage1 as S
    from .atlas_outputs import FG_WINDOW, parse_size
    results_folder = Path("./results/%s/stage_1" % args.vid_name)
    ckpt = results_folder / "checkpoint"
    if not ckpt.exists():
        raise SystemExit("no stage-1 checkpoint at %s: run stage1_seg.py first" % ckpt)
    with open(results_folder / "config.json") as f:
        config = json.load(f)
    config.pop("atlasfit_arithmetic", None)
    data_folder = Path(args.root) / args.vid_name
    frames = sorted(list(data_folder.glob("*.jpg")) + list(data_folder.glob("*.png")))
    if not frames:
        raise SystemExit("no frames under %s" % data_folder)
    w, h = Image.open(frames[0]).size
    resx, resy = (int(w / args.down), int(h / args.down)) if args.down is not None else (w, h)
    size = parse_size(getattr(args, "size", "stage1"), full=(h, w))
    oh, ow = size if size is not None else (resy, resx)
    F = S.count_input_frames(config["maximum_number_of_frames"], data_folder)
    tex_fg = _read_texture(args.edit_fg) if args.edit_fg else None
    tex_bg = _read_texture(args.edit_bg) if args.edit_bg else None
    res = (tex_fg if tex_fg is not None else tex_bg).shape[0]
    if tex_fg is not None and tex_bg is not None and tex_bg.shape != tex_fg.shape:
        raise SystemExit("--edit_fg and --edit_bg must have the same size")
    af = A.AtlasFit(A.default_config(resx, resy, F, config, two_layer=True))
    try:
        t = S.load_input_data_device(resy, resx, config["maximum_number_of_frames"], data_folder, True, data_folder.parent, args.vid_name, with_masks=True)
        flows_mask, video_frames, flows_rev_mask, flows_rev, flows, mask_frames = t[:6]
        af.upload_video(video_frames, flows, flows_rev, flows_mask, flows_rev_mask, mask_frames)
        S.load_checkpoint(af, ckpt)
        win_bg = af.area_window(af.mapping_area(1))
        if tex_fg is None:
            tex_fg = af.atlas_texture(res, FG_WINDOW)
        if tex_bg is None:
            tex_bg = af.atlas_texture(res, win_bg)
        out = Path(args.out) if args.out else results_folder / "edit"
        out.mkdir(parents=True, exist_ok=True)
        with af.edit_session(res, tex_fg, FG_WINDOW, tex_bg, win_bg) as session:
            for f in range(F):
                Image.fromarray(session.frame(f, oh, ow, outputs=(), u8=True)["edit_u8"]).save(str(out / ("%05d.png" % f)))
        print("wrote %d edited frames to %s" % (F, out))
    finally:
        af.close()


def _cli(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--vid_name", type=str, required=True)
    p.add_argument("--root", type=str, default="data/test/")
    p.add_argument("--down", type=int, default=1)
    p.add_argument("--edit_fg", type=str, default=None, help="edited foreground texture (texture_orig1.png painted on)")
    p.add_argument("--edit_bg", type=str, default=None, help="edited background texture (texture_orig2.png painted on)")
    p.add_argument("--out", type=str, default=None, help="output directory (default ./results/<vid>/stage_1/edit)")
    p.add_argument("--size", type=str, default="stage1", help="size of the edited video: stage1 (the lattice, default), full (the decoded frames' size) or HxW")
    args = p.parse_args(argv)
    if not args.edit_fg and not args.edit_bg:
        p.error("give --edit_fg and / or --edit_bg")
    from .atlas_outputs import parse_size
    try:
        parse_size(args.size, full=(1, 1))
    except ValueError as e:
        p.error(str(e))
    run(args)


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import atlas_edit as _e
        _e._cli()
    else:
        _cli()
