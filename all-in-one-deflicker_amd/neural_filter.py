"""Drop-in for the reference's stage-2 script `src/neural_filter_and_refinement.py`: same flags, same input folders, same three
output folders and the same PNG quantisation, run from the root of a processed clip's tree (./data/test/<vid>, ./results/<vid>) —
but both nets run on this package's MI355X path (aiod_amd.NeuralFilter), `--gpu` is honoured (the reference parses it and then
forces device 0, :42), and only PIL and torch are needed (no cv2, easydict, imageio or tqdm).

    python <this repo>/all-in-one-deflicker_amd/neural_filter.py --video_name <vid> [--fps 10] [--gpu 0]
        [--ckpt_filter ./pretrained_weights/neural_filter.pth] [--ckpt_local ./pretrained_weights/local_refinement_net.pth]
        [--filter_precision fp32|fp16]

Per frame (:89-121): content = input PNG / 255, style = stage-1 PNG / 255 resized bilinearly (cv2.resize's INTER_LINEAR geometry,
af_resize_bilinear) to the content's size; pred = UNet(cat(content, style)) and the refinement loop give final, at the padded size;
content, style, pred and final are each resized (not cropped) back to the original size, clipped to [0, 1], times 255, truncated to
uint8 and written as neural_filter/concat (content | style | pred), neural_filter/output (pred) and final/output (final).  The three
mp4 encodes run only when ffmpeg is on PATH."""
import argparse
import os
import shutil
import sys
from glob import glob

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="stage 2 (neural filter + local refinement) on the MI355X")
    p.add_argument("--ckpt_filter", default="./pretrained_weights/neural_filter.pth", type=str, help="the ckpt of neural filter network")
    p.add_argument("--ckpt_local", default="./pretrained_weights/local_refinement_net.pth", type=str, help="the ckpt of local refinement network")
    p.add_argument("--fps", default=10, type=int, help="frame per second")
    p.add_argument("--video_name", default=None, type=str, help="the name of input video")
    p.add_argument("--gpu", type=int, default=0, help="gpu device id")
    p.add_argument("--filter_precision", choices=("fp32", "fp16"), default="fp32",
                   help="fp32, or fp16: both nets as the reference's modules compute them under fp16 autocast (aiod_amd.NeuralFilter(precision=...))")
    return p.parse_args(argv)


def read_png(path):
    """load_image (src/models/utils.py:583-592) before the division: HWC uint8, grey expanded to three channels, alpha dropped."""
    import numpy as np
    from PIL import Image
    img = np.array(Image.open(path))
    if img.ndim == 2:
        img = np.stack([img] * 3, axis=2)
    return np.ascontiguousarray(img[..., :3])


def quantise(img):
    """save_img (src/models/utils.py:234-251): clip to [0, 1], times 255 in fp32, truncated to uint8."""
    import numpy as np
    return (np.clip(img, 0, 1) * np.float32(255.0)).astype(np.uint8)


def main(argv=None):
    opts = parse_args(argv)
    print(opts)
    import numpy as np
    import torch
    from PIL import Image
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    import aiod_amd
    from aiod_amd.atlasfit import resize_bilinear_device

    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: the native stage 2 has no CPU path")
    dev = torch.device("cuda:%d" % opts.gpu)
    torch.cuda.set_device(dev)

    style_root = "./results/{}/stage_1/output".format(opts.video_name)
    content_root = "./data/test/{}".format(opts.video_name)
    style_names = sorted(glob(style_root + "/*"))
    content_names = sorted(glob(content_root + "/*"))
    assert len(style_names) == len(content_names), "the number of style frames is different from the number of content frames"
    num_frames = len(style_names)
    print("Processing {} frames".format(num_frames))

    output_folder = "./results/{}/neural_filter/concat".format(opts.video_name)
    process_filter_dir = "./results/{}/neural_filter/output".format(opts.video_name)
    output_final_dir = os.path.join("results", opts.video_name, "final", "output")
    for d in (output_folder, process_filter_dir, output_final_dir):
        os.makedirs(d, exist_ok=True)
    print("neural filter dir:", process_filter_dir)
    print("output final dir:", output_final_dir)
    print("output dir:", output_folder)
    if num_frames == 0:
        return 0

    nf = None
    ckpt = torch.load(opts.ckpt_filter, map_location="cpu")
    print("Load %s" % opts.ckpt_local)
    ckpt_local = torch.load(opts.ckpt_local, map_location="cpu")

    def to_size(u8_or_f32, h, w):
        """af_resize_bilinear of an HWC image (uint8: / 255 first) to (h, w), on the device."""
        src = torch.from_numpy(u8_or_f32).to(dev) if isinstance(u8_or_f32, np.ndarray) else u8_or_f32.contiguous()
        out = torch.empty((h, w, 3), device=dev)
        resize_bilinear_device(src, out, h, w, 3, 1, 0, device=opts.gpu)
        return out

    for frame_id in range(num_frames):
        content_u8 = read_png(content_names[frame_id])
        h, w = content_u8.shape[:2]
        if nf is None:
            nf = aiod_amd.NeuralFilter(h, w, device=opts.gpu, precision=opts.filter_precision)
            nf.load_state_dicts(ckpt, ckpt_local)
        elif (h, w) != (nf.h, nf.w):
            raise SystemExit("frame %s is %dx%d, the first frame %dx%d" % (content_names[frame_id], w, h, nf.w, nf.h))
        content = to_size(content_u8, h, w)                                  # same size: u8 / 255, as load_image(resize=False)
        style = to_size(read_png(style_names[frame_id]), h, w)               # load_image(size=org_size): cv2.resize to the content's size
        pred, final = nf.frame(content, style)
        padded_in = torch.from_numpy(nf.activation("input")).to(dev)         # the padded content and style the nets saw
        outs = [to_size(t, h, w).cpu().numpy() for t in (padded_in[..., :3], padded_in[..., 3:], pred, final)]
        concat = np.concatenate(outs[:3], axis=1)
        Image.fromarray(quantise(concat)).save("{}/{:05d}.png".format(output_folder, frame_id))
        Image.fromarray(quantise(outs[2])).save("{}/{:05d}.png".format(process_filter_dir, frame_id))
        Image.fromarray(quantise(outs[3])).save("{}/{:05d}.png".format(output_final_dir, frame_id))
        print("frame %d / %d" % (frame_id + 1, num_frames))
    nf.close()

    if shutil.which("ffmpeg") is None:
        print("ffmpeg not on PATH: skipped the three mp4 encodes")
        return 0
    for d in (output_folder, process_filter_dir, output_final_dir):
        cmd = "ffmpeg -y -r %s -i %s -crf 25 -r 12 -qscale 4  %s" % (str(opts.fps), os.path.join(d, "%05d.png"), d + ".mp4")
        os.system(cmd)
    return 0


if __name__ == "__main__":
    sys.exit(main())
