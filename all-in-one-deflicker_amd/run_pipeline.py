"""Drop-in for the reference's end-to-end driver `test.py` (test.py:1-43): same flags, same three stages, same folders,
run from the root of a checkout of the reference — but stage 1 is this package's MI355X path and `--gpu` is actually
forwarded (the reference parses it and drops it, test.py:36-42).

    python <this repo>/all-in-one-deflicker_amd/run_pipeline.py --video_name data/test/X.mp4 [--fps 10] [--gpu 0] [--class_name C]

Stage 0 (ffmpeg frame extraction) and stage 2 (`src/neural_filter_and_refinement.py`) are the reference's own commands,
unchanged (with --native_stage2, stage 2 is this package's neural_filter.py instead); the flow / mask preprocessors are called by the stage-1 CLI exactly as the reference's stage-1 scripts do
(with --native_flow, the flow precompute is this package's preprocess_optical_flow.py).  With --in_process one deflicker.py command replaces the stage-1 and
stage-2 commands: the three native stages in one process, hand-offs on the device (single-atlas path only: --class_name
would have to run a mask preprocessor; the in-process fg/bg route is deflicker.py --masks_dir on masks that already exist, or
--mask_keys_dir, passed on from here: masks for a few key frames, propagated to the others along the flows)."""
import argparse
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CUT_FLAGS = ("cut_threshold", "cut_margin", "cut_radius", "min_shot_frames")      # deflicker.py's; forwarded when given
MASK_KEY_FLAGS = ("mask_keys_dir", "mask_thresh")                                 # deflicker.py's key-mask route (masks.py); --in_process only
PROXY_FLAGS = ("proxy_long_edge", "proxy_radius", "proxy_eps", "proxy_guide")       # deflicker.py's proxy route (guided.py); --in_process only
FIDELITY_FLAGS = ("reference_dir", "ssim_window")                                 # deflicker.py's fidelity report (fidelity.py), behind --fidelity; --in_process only
VIDEO_FLAGS = ("video", "video_out", "yuv_matrix", "yuv_range")                    # deflicker.py's YUV4MPEG2 route (y4m.py); --in_process only


def build_commands(opts):
    """The shell commands of the three stages, in order (pure function: unit-tested without running anything)."""
    cmds = []
    video = getattr(opts, "video", None)
    if video is not None:                          # a YUV4MPEG2 stream goes to deflicker.py as it is: no ffmpeg frame extraction, no frame folder
        if not getattr(opts, "in_process", False):
            raise ValueError("--video is an option of the one-process pipeline: it needs --in_process")
        base = "stdin" if video == "-" else os.path.splitext(os.path.basename(video))[0]
        folder = None
    elif opts.video_name is not None:
        base = os.path.basename(opts.video_name)[:-4]
        folder = "./data/test/{}".format(base)
        cmds.append(("mkdir", folder))
        cmds.append(("sh", "ffmpeg -i {} -vf fps={} -start_number 0 {}/%05d.png".format(opts.video_name, opts.fps, folder)))
    else:
        base = os.path.basename(opts.video_frame_folder)
        folder = "./data/test/{}".format(base)
        if not os.path.isdir(folder):
            cmds.append(("sh", "mv {} {}".format(base, folder)))
    py = sys.executable or "python"
    if getattr(opts, "in_process", False):         # the three native stages in one process (deflicker.py): no stage-1 / stage-2 commands
        if opts.class_name is not None:
            raise ValueError("--in_process runs the single-atlas path only: drop --class_name or --in_process")
        cmds.append(("sh", "{} {} {} --out ./results/{} --gpu {} --ckpt_filter {} --ckpt_local {}".format(
            py, os.path.join(_HERE, "deflicker.py"), "--video " + video if video is not None else "--frames_dir " + folder, base, opts.gpu,
            getattr(opts, "ckpt_filter", "./pretrained_weights/neural_filter.pth"),
            getattr(opts, "ckpt_local", "./pretrained_weights/local_refinement_net.pth"))))
        if getattr(opts, "style_size", "stage1") != "stage1":
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --style_size " + opts.style_size)
        if getattr(opts, "flow_precision", "fp32") != "fp32":
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --flow_precision " + opts.flow_precision)
        if getattr(opts, "filter_precision", "fp32") != "fp32":
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --filter_precision " + opts.filter_precision)
        if getattr(opts, "cuts", "none") != "none":        # scene cuts: deflicker.py parses and checks the value
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --cuts " + opts.cuts)
        for flag in CUT_FLAGS:
            if getattr(opts, flag, None) is not None:
                cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --%s %s" % (flag, getattr(opts, flag)))
        if getattr(opts, "video_out", None) is not None:
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --video_out " + opts.video_out)
            if video is None:                      # frames from the folder ffmpeg filled at --fps: the stream's rate
                cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --fps %s" % opts.fps)
        for flag in ("yuv_matrix", "yuv_range"):
            if getattr(opts, flag, "auto") != "auto":
                cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --%s %s" % (flag, getattr(opts, flag)))
        if getattr(opts, "video_depth", "8") != "8":      # a stream of more than 8 bits per sample carried at its depth
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --video_depth " + opts.video_depth)
        for flag in MASK_KEY_FLAGS:                # key masks, propagated along the flows: the in-process fg/bg route without a mask per frame
            if getattr(opts, flag, None) is not None:
                cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --%s %s" % (flag, getattr(opts, flag)))
        for flag in PROXY_FLAGS:                   # the run on shrunk frames, its result carried to the full-size frames (guided.py)
            if getattr(opts, flag, None) is not None:
                cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --%s %s" % (flag, getattr(opts, flag)))
        if getattr(opts, "fidelity", False):       # PSNR / SSIM of the final frames against the input (and a clean reference clip)
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --fidelity")
            for flag in FIDELITY_FLAGS:
                if getattr(opts, flag, None) is not None:
                    cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --%s %s" % (flag, getattr(opts, flag)))
        return cmds
    if getattr(opts, "fidelity", False) or any(getattr(opts, flag, None) is not None for flag in FIDELITY_FLAGS):
        raise ValueError("--fidelity, --reference_dir and --ssim_window are options of the one-process pipeline: they need --in_process")
    if any(getattr(opts, flag, None) is not None for flag in PROXY_FLAGS):
        raise ValueError("--proxy_long_edge, --proxy_radius, --proxy_eps and --proxy_guide are options of the one-process pipeline: they need --in_process")
    if any(getattr(opts, flag, None) is not None for flag in MASK_KEY_FLAGS):
        raise ValueError("--mask_keys_dir and --mask_thresh are options of the one-process pipeline: they need --in_process")
    if opts.class_name is None:
        cmds.append(("sh", "{} {} --vid_name {} --gpu {}".format(py, os.path.join(_HERE, "stage1.py"), base, opts.gpu)))
    else:
        cmds.append(("sh", "{} {} --vid_name {} --class_name {} --gpu {}".format(py, os.path.join(_HERE, "stage1_seg.py"), base, opts.class_name, opts.gpu)))
    if getattr(opts, "native_flow", False):        # the stage-1 CLI then calls this package's preprocess_optical_flow.py for the RAFT flows
        cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --native_flow")
        if getattr(opts, "flow_precision", "fp32") != "fp32":
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --flow_precision " + opts.flow_precision)
    if getattr(opts, "style_size", "stage1") != "stage1":      # the stage-1 CLI then writes stage_1/output at the frames' own size
        cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --style_size " + opts.style_size)
    if getattr(opts, "native_stage2", False):      # this package's stage 2 (neural_filter.py), with the checkpoints and --gpu forwarded
        cmds.append(("sh", "{} {} --video_name {} --fps {} --gpu {} --ckpt_filter {} --ckpt_local {}".format(
            py, os.path.join(_HERE, "neural_filter.py"), base, opts.fps, opts.gpu,
            getattr(opts, "ckpt_filter", "./pretrained_weights/neural_filter.pth"),
            getattr(opts, "ckpt_local", "./pretrained_weights/local_refinement_net.pth"))))
        if getattr(opts, "filter_precision", "fp32") != "fp32":
            cmds[-1] = (cmds[-1][0], cmds[-1][1] + " --filter_precision " + opts.filter_precision)
    else:
        cmds.append(("sh", "python src/neural_filter_and_refinement.py --video_name {} --fps {}".format(base, opts.fps)))
    return cmds


def cuts_text(text):
    """--cuts as deflicker.py reads it: none, auto or comma-separated frame indices.  The text goes into a shell command, so nothing else passes."""
    t = str(text).strip().lower()
    if not re.fullmatch(r"none|auto|\d+(,\d+)*", t):
        raise argparse.ArgumentTypeError("expected none, auto or comma-separated first-frame indices of new shots, got %r" % text)
    return t


def shell_path(text):
    """A file name that goes into a shell command unquoted: letters, digits and . _ - / + only (or - alone)."""
    if not re.fullmatch(r"[A-Za-z0-9._/+-]+", str(text)):
        raise argparse.ArgumentTypeError("expected a plain file name (letters, digits, . _ - / +), got %r" % text)
    return str(text)


def parse_opts(argv=None):
    """The wrapper's options (pure: nothing runs)."""
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_filter", default="./pretrained_weights/neural_filter.pth", type=str)
    p.add_argument("--ckpt_local", default="./pretrained_weights/local_refinement_net.pth", type=str)
    p.add_argument("--video_name", default=None, type=str)
    p.add_argument("--video_frame_folder", default=None, type=str)
    p.add_argument("--fps", default=10, type=int)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--class_name", default=None, type=str)
    p.add_argument("--native_stage2", action="store_true", help="run stage 2 on this package's MI355X path (neural_filter.py) instead of the reference's script")
    p.add_argument("--native_flow", action="store_true", help="compute the RAFT flows on this package's MI355X path (preprocess_optical_flow.py) instead of the reference's script")
    p.add_argument("--in_process", action="store_true", help="run RAFT, stage 1 and stage 2 natively in one process (deflicker.py) instead of the stage-1 and stage-2 commands")
    p.add_argument("--style_size", type=str, default="stage1", choices=("stage1", "full"),
                   help="passed on to stage 1 (or to --in_process): full renders the styles at the frames' own size instead of the stage-1 size")
    p.add_argument("--flow_precision", type=str, default="fp32", choices=("fp32", "fp16"),
                   help="passed on to the native flow precompute (--native_flow) or to --in_process: fp16 is the arithmetic the reference's RAFT runs on a GPU")
    p.add_argument("--filter_precision", type=str, default="fp32", choices=("fp32", "fp16"),
                   help="passed on to the native stage 2 (--native_stage2) or to --in_process: fp16 runs both nets as under fp16 autocast")
    p.add_argument("--cuts", type=cuts_text, default="none", metavar="none|auto|I,J,K",
                   help="passed on to --in_process: scene cuts, detected (auto) or given as first-frame indices of the new shots; every shot is fitted on its own")
    p.add_argument("--cut_threshold", type=float, default=None, help="passed on to --in_process with --cuts auto (default: deflicker.py's)")
    p.add_argument("--cut_margin", type=float, default=None, help="passed on to --in_process with --cuts auto")
    p.add_argument("--cut_radius", type=int, default=None, help="passed on to --in_process with --cuts auto")
    p.add_argument("--min_shot_frames", type=int, default=None, help="passed on to --in_process with --cuts auto")
    p.add_argument("--video", type=shell_path, default=None, metavar="FILE|-",
                   help="passed on to --in_process: a YUV4MPEG2 stream (.y4m file, or - for standard input) instead of --video_name / --video_frame_folder; no frames are extracted")
    p.add_argument("--video_out", type=shell_path, default=None, metavar="FILE|-", help="passed on to --in_process: write the final frames as a YUV4MPEG2 stream (- for standard output)")
    p.add_argument("--yuv_matrix", type=str, default="auto", choices=("auto", "bt601", "bt709"), help="passed on to --in_process with --video / --video_out")
    p.add_argument("--yuv_range", type=str, default="auto", choices=("auto", "limited", "full"), help="passed on to --in_process with --video / --video_out")
    p.add_argument("--video_depth", type=str, default="8", choices=("8", "keep"), help="passed on to --in_process with --video: keep carries a 9 to 16-bit stream at its depth (needs --video_out)")
    p.add_argument("--mask_keys_dir", type=shell_path, default=None,
                   help="passed on to --in_process: a folder of key masks (file stems of the frames they belong to); the other frames' masks are propagated along the flows and the fg/bg two-layer path is fitted")
    p.add_argument("--mask_thresh", type=float, default=None, help="passed on to --in_process with --mask_keys_dir (default: deflicker.py's)")
    p.add_argument("--proxy_long_edge", type=int, default=None,
                   help="passed on to --in_process: run the pipeline on frames shrunk to this long edge and carry the result to the full-size frames (guided transfer)")
    p.add_argument("--proxy_radius", type=int, default=None, help="passed on to --in_process with --proxy_long_edge (default: deflicker.py's)")
    p.add_argument("--proxy_eps", type=float, default=None, help="passed on to --in_process with --proxy_long_edge (default: deflicker.py's)")
    p.add_argument("--proxy_guide", type=str, default=None, choices=("channel", "colour"), help="passed on to --in_process with --proxy_long_edge (default: deflicker.py's, channel)")
    p.add_argument("--fidelity", action="store_true", help="passed on to --in_process: add the PSNR and SSIM of the final frames against the input frames to deflicker.json")
    p.add_argument("--reference_dir", type=shell_path, default=None, help="passed on to --in_process with --fidelity: a folder of clean frames to compare the input and the final frames with")
    p.add_argument("--ssim_window", type=int, default=None, help="passed on to --in_process with --fidelity (default: deflicker.py's)")
    opts = p.parse_args(argv)
    if not opts.in_process and (opts.fidelity or any(getattr(opts, f) is not None for f in FIDELITY_FLAGS)):
        p.error("--fidelity, --reference_dir and --ssim_window are options of the one-process pipeline: they need --in_process")
    if not opts.fidelity and any(getattr(opts, f) is not None for f in FIDELITY_FLAGS):
        p.error("--reference_dir and --ssim_window are options of --fidelity")
    if not opts.in_process and any(getattr(opts, f) is not None for f in PROXY_FLAGS):
        p.error("--proxy_long_edge, --proxy_radius, --proxy_eps and --proxy_guide are options of the one-process pipeline: they need --in_process")
    if opts.proxy_long_edge is None and (opts.proxy_radius is not None or opts.proxy_eps is not None or opts.proxy_guide is not None):
        p.error("--proxy_radius, --proxy_eps and --proxy_guide are options of --proxy_long_edge")
    if not opts.in_process and any(getattr(opts, f) is not None for f in MASK_KEY_FLAGS):
        p.error("--mask_keys_dir and --mask_thresh are options of the one-process pipeline: they need --in_process")
    if opts.mask_thresh is not None and opts.mask_keys_dir is None:
        p.error("--mask_thresh is an option of --mask_keys_dir")
    if not opts.in_process and (opts.video is not None or opts.video_out is not None or opts.yuv_matrix != "auto" or opts.yuv_range != "auto"):
        p.error("--video, --video_out, --yuv_matrix and --yuv_range are options of the one-process pipeline: they need --in_process")
    if opts.video_depth != "8" and opts.video is None:
        p.error("--video_depth is an option of --video (and of the one-process pipeline: it needs --in_process)")
    if opts.video is not None and (opts.video_name is not None or opts.video_frame_folder is not None):
        p.error("--video replaces --video_name / --video_frame_folder: give one of them")
    if not opts.in_process and (opts.cuts != "none" or any(getattr(opts, f) is not None for f in CUT_FLAGS)):
        p.error("--cuts and the --cut_* / --min_shot_frames knobs are options of the one-process pipeline: they need --in_process")
    if opts.filter_precision != "fp32" and not (opts.native_stage2 or opts.in_process):
        p.error("--filter_precision is an option of the native stage 2: it needs --native_stage2 (or --in_process)")
    if opts.flow_precision != "fp32" and not (opts.native_flow or opts.in_process):
        p.error("--flow_precision is an option of the native flow precompute: it needs --native_flow (or --in_process)")
    if opts.video_name is None and opts.video_frame_folder is None and opts.video is None:
        p.error("--video_name or --video_frame_folder")
    if opts.in_process and opts.class_name is not None:
        p.error("--in_process runs the single-atlas path only (no --class_name)")
    return opts


def main(argv=None):
    opts = parse_opts(argv)
    log = sys.stderr if opts.video_out == "-" else sys.stdout      # --video_out -: standard output carries the stream and nothing else
    print(opts, file=log)
    for kind, c in build_commands(opts):
        print(c, file=log, flush=True)
        if kind == "mkdir":
            os.makedirs(c, exist_ok=True)
        elif os.system(c) != 0:
            sys.exit("command failed: " + c)


if __name__ == "__main__":
    main()
