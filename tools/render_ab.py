#!/usr/bin/env python
"""Bytes of everything a trained handle renders, for an A/B run across two builds of the library on one MI355X (MEASUREMENTS.md Part T).

    python tools/render_ab.py --out parent.npz          # on the build to compare against
    python tools/render_ab.py --against parent.npz      # on the other build: every array and scalar must be bit-equal

States: the 40x24x6 golden start states (single and two-layer), tests/golden/ckpt_single.pt and ckpt_seg.pt (as stored, and with the alpha
net's output layer rescaled as tests/test_gpu_layers_at.py does, so that alpha spans its range); every frame; mlp modes 0, 1, 2, 3.
Calls: render_frame (rgb, sse), render_frame_u8, render_frame_device, psnr, warp_error("reconstruction") with both align_corners,
mapping_area(0 / 1), render_layers, render_edit with textures and with usage masks only (masks accumulated over all frames),
render_frame_at_u8 against a fixed uint8 reference, render_layers_at(alpha_u8=True) and EditSession.frame(u8=True) at (resy, resx),
41x67 and 72x120, and the session's usage().  Floats are compared by their bits, so a NaN or a signed zero cannot hide a difference.
--against exits 1 on any difference and prints the names that differ."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
GOLDEN = os.path.join(TESTS, "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

MODES = (0, 1, 2, 3)
SIZES = ((41, 67), (72, 120))      # besides (resy, resx)
EDIT_RES = 64
LAYERS = ("uv1", "uv2", "alpha", "rgb1", "rgb2")
EDITS = ("edit", "edit_fg", "edit_bg")


def _states():
    """[(name, handle, two_layer)]: open handles with the video uploaded."""
    import aiod_amd
    import conftest as T
    from aiod_amd import stage1 as S
    from test_gpu_layers_at import _ckpt_handle, _start_handle, _start_models
    g1, g2 = T._load_single("small"), T._load_seg("small")
    v1, v2 = T._video(g1, "constant"), T._seg_video(g2, "constant")
    ga = dict(np.load(os.path.join(GOLDEN, "atlas_seg.npz")))
    out = [("start_single", _start_handle(g1, v1, False, _start_models(g1, False)), False),
           ("start_seg", _start_handle(g2, v2, True, _start_models(g2, True)), True)]
    for name, g, v, two in (("ckpt_single", g1, v1, False), ("ckpt_seg", g2, v2, True)):
        af = aiod_amd.AtlasFit(aiod_amd.default_config(v.resx, v.resy, v.F, g["config"], two_layer=two))
        af.upload_video(v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, v.optical_flows_reverse_mask,
                        *((v.mask_frames,) if two else ()))
        S.load_checkpoint(af, os.path.join(GOLDEN, name + ".pt"))
        out.append((name, af, two))
    out.append(("ckpt_seg_scaled", _ckpt_handle(g2, v2, ga), True))
    return out, ga


def _edit_cases(ga):
    """{tag: (textures, fg window, bg window)} at side EDIT_RES: the unit windows and the narrowed ones of tests/test_gpu_layers_at.py."""
    from test_gpu_layers_at import FG_NARROW, _textures
    t1, t2 = _textures(ga, EDIT_RES)
    area = ga["area_bg_scaled"]
    return {"unit": (t1, t2, (0.0, 0.0, 1.0), (-1.0, -1.0, 1.0)),
            "narrow": (t1, t2, FG_NARROW, (area[1], area[3], np.float32(area[4]) / np.float32(2)))}


def dump():
    out = {}
    states, ga = _states()
    cases = _edit_cases(ga)
    rng = np.random.default_rng(7)
    for name, af, two in states:
        H, W, F = af.cfg.resy, af.cfg.resx, af.cfg.number_of_frames
        sizes = ((H, W),) + SIZES
        refs = {s: rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes}
        for mode in MODES:
            af.set_mlp_mode(mode)
            key = "%s/m%d/" % (name, mode)
            out[key + "psnr_first"] = np.array(af.psnr()[1])          # fills the cache through af_psnr's own NULL-output renders
            use = {tag: (np.zeros((EDIT_RES, EDIT_RES), np.float32), np.zeros((EDIT_RES, EDIT_RES), np.float32)) for tag in cases}
            sessions = {tag: af.edit_session(EDIT_RES, c[0], c[2], c[1], c[3], track_usage=True) for tag, c in cases.items()} if two else {}
            for f in range(F):
                k = key + "f%d/" % f
                rgb, sse = af.render_frame(f)
                out[k + "render_frame.rgb"], out[k + "render_frame.sse"] = rgb, np.float64(sse)
                rgb, u8, sse = af.render_frame_u8(f)
                out[k + "render_frame_u8.rgb"], out[k + "render_frame_u8.u8"], out[k + "render_frame_u8.sse"] = rgb, u8, np.float64(sse)
                rgb, u8, sse = af.render_frame_device(f)
                out[k + "render_frame_device.rgb"], out[k + "render_frame_device.u8"] = rgb.cpu().numpy(), u8.cpu().numpy()
                out[k + "render_frame_device.sse"] = np.float64(sse)
                for n, a in af.render_layers(f).items():
                    if a is not None:
                        out[k + "render_layers." + n] = a
                for oh, ow in sizes:
                    s = "%dx%d." % (oh, ow)
                    rgb, u8, sse = af.render_frame_at_u8(f, oh, ow, ref=refs[(oh, ow)])
                    out[k + "render_frame_at_u8." + s + "rgb"], out[k + "render_frame_at_u8." + s + "u8"] = rgb, u8
                    out[k + "render_frame_at_u8." + s + "sse"] = np.float64(sse)
                    for n, a in af.render_layers_at(f, oh, ow, alpha_u8=True).items():
                        out[k + "render_layers_at." + s + n] = a
                for tag, (t1, t2, wf, wb) in cases.items():
                    if not two:
                        break
                    for n, a in af.render_edit(f, EDIT_RES, t1, wf, t2, wb).items():
                        out[k + "render_edit." + tag + "." + n] = a
                    af.render_edit(f, EDIT_RES, None, wf, None, wb, use_fg=use[tag][0], use_bg=use[tag][1], outputs=())
                    for oh, ow in sizes:
                        for n, a in sessions[tag].frame(f, oh, ow, outputs=EDITS, u8=True).items():
                            out[k + "session." + tag + ".%dx%d." % (oh, ow) + n] = a
            for tag in sessions:
                out[key + "render_edit." + tag + ".use_fg"], out[key + "render_edit." + tag + ".use_bg"] = use[tag]
                out[key + "session." + tag + ".use_fg"], out[key + "session." + tag + ".use_bg"] = sessions[tag].usage()
                sessions[tag].close()
            mean, per = af.psnr()
            out[key + "psnr.mean"], out[key + "psnr.per_frame"] = np.float64(mean), np.array(per)
            for ac in (False, True):
                mean, per = af.warp_error("reconstruction", align_corners=ac)
                out[key + "warp_error.ac%d.mean" % ac], out[key + "warp_error.ac%d.per_pair" % ac] = np.float64(mean), np.array(per)
            if two:
                for which in (0, 1):
                    out[key + "mapping_area.%d" % which] = np.array(af.mapping_area(which), np.float32)
        af.close()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--against", default=None)
    a = ap.parse_args()
    if not a.out and not a.against:
        raise SystemExit("give --out X.npz or --against X.npz")
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found")
    got = dump()
    nbytes = sum(np.asarray(v).nbytes for v in got.values())
    print("rendered %d arrays and scalars, %d bytes" % (len(got), nbytes))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        np.savez_compressed(a.out, **got)
        print("wrote", a.out)
    if a.against:
        want = dict(np.load(a.against))
        bad = sorted(set(got) ^ set(want))
        for k in sorted(set(got) & set(want)):
            g, w = np.asarray(got[k]), want[k]
            if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(_bits(g), _bits(w)):
                bad.append(k)
        print("compared %d arrays and scalars against %s: %d differ" % (len(want), a.against, len(bad)))
        for k in bad[:40]:
            print("  differs:", k)
        if bad:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
