"""The whole pipeline in one process: frames in, deflickered frames out, with every hand-off between the three native stages a device
tensor.

    python all-in-one-deflicker_amd/deflicker.py --frames_dir data/test/X [--masks_dir data/test/X_seg] [--out results/X] [--config F]
        [--down 4] [--seed S] [--gpu 0] [--model pretrained_weights/raft-things.pth] [--ckpt_filter ...] [--ckpt_local ...]
        [--window_overlap K] [--max_long_edge 2000] [--style_size stage1|full] [--flow_precision fp32|fp16] [--filter_precision fp32|fp16]
        [--cuts none|auto|I,J,K [--cut_threshold 0.5] [--cut_margin 0.25] [--cut_radius 4] [--min_shot_frames 5]]
        [--mask_keys_dir data/test/X_keys [--mask_thresh 1.0] [--masks_only]]
        [--proxy_long_edge N [--proxy_radius 8] [--proxy_eps 64] [--proxy_guide channel|colour]]
        [--keep_intermediates]
        [--warp_error [--warp_error_geometry exact|reference]]
        [--fidelity [--reference_dir D] [--ssim_window 7]]
    python all-in-one-deflicker_amd/deflicker.py --video FILE.y4m|- [--video_out FILE.y4m|-] [--yuv_matrix auto|bt601|bt709]
        [--yuv_range auto|limited|full] ...                  (YUV4MPEG2 in and out, files or pipes: y4m.py)
    python all-in-one-deflicker_amd/deflicker.py --frames_dir data/test/X --video_out FILE.y4m|- --fps N[:D] [--yuv_layout 420jpeg] ...

Runs from any directory; needs no checkout of the reference and no ffmpeg.  Writes <out>/final/output/%05d.png and <out>/deflicker.json
(windows, PSNR per window, seconds per stage, the arithmetic in force, the seed, the size RAFT ran at); with --keep_intermediates also the trees the three
drop-in CLIs leave: <frames_dir>_flow/*.npy, <out>/stage_1/output, <out>/neural_filter/output and <out>/neural_filter/concat.

`Deflicker.run` does, in this order: RAFT over the clip as preprocess_optical_flow.preprocess drives it (one encode per frame, two live
slots, both directions per launch; a clip longer than --max_long_edge is shrunk for RAFT alone, frame by frame on the device, to
preprocess_optical_flow.shrink_size with cv2.INTER_AREA's arithmetic, as RAFTWrapper.load_image shrinks it, while the builder, stage 2
and E_warp keep the full-size frames), each flow resized to the stage-1 resolution as soon as it exists; the RAFT handle is closed; per
window (plan_windows) the schedule of stage1.main on an AtlasFit of its own, whose render at the last evaluation iteration is the style
(AtlasFit.render_frame_device: the bytes the stage-1 CLI writes to stage_1/output); one NeuralFilter over the whole clip in frame order
as neural_filter.main drives it, its recurrent state carried across window seams.  A clip longer than `maximum_number_of_frames` is cut
into windows, each fitted exactly as a stand-alone clip of its frames with seed + k; with window_overlap = K the float renders of the
shared frames are cross-faded before quantisation.

With masks (`run(frames, masks=...)`, `--masks_dir`: one uint8 mask per frame, 255 = foreground, any size) every window is fitted on the
fg/bg two-layer path instead, as stage1.main(two_layer=True) fits it (stage1_seg.py): four nets, both pre-train jobs, the masks resized
to the stage-1 size by the builder (stage1.put_mask_device) and uploaded with the video; a window gets the masks of its own frames, and
its alpha-blended render is the style.  RAFT and stage 2 never see the masks.  The masks are the user's: the reference's mask
preprocessors (external segmentation models) are not run by this package.  The layer products of the two-layer fit (mattes, atlas
textures: stage1_seg.py --atlas_outputs) are out of scope.

With key masks (`run(frames, mask_keys={index: mask})`, `--mask_keys_dir`: masks for a few frames only; masks.py) the
masks of the other frames are propagated along the stage-1-size flows on the device (af_mask_step / af_mask_blend), shot by shot, after
RAFT and before any fit; the fits then run on the two-layer path with the propagated planes as their mask_frames.  --masks_only stops
after the propagation and writes <out>/masks/%05d.png: the masks can be reviewed before a long run.

With style_size = "full" (`--style_size full`) the style of a frame is not the stage-1-size render stretched by stage 2 but the fitted
nets evaluated at the pixel centres of the clip's own size (AtlasFit.render_frame_at_device, include/atlasfit.h af_render_frame_at), so
stage 2's resize of the style is the same-size identity it already is for the content.  The default "stage1" does what it always did.

With cuts (`Deflicker(cuts="auto" | [I, J, K])`, `--cuts`; shots.py) the clip is split at its scene cuts and every shot
is treated as a clip of its own inside the one run: no RAFT pair across a cut, windows planned per shot (numbered in clip order, window
k fitted with seed + k), stage 2's recurrent state reset at a shot's first frame, E_warp without the cut pairs.  "auto" uploads and
scores every frame first (af_luma_grid) and runs RAFT afterwards.  The default None is one shot: the calls and bytes of before.

With a proxy (`Deflicker(proxy_long_edge=N)`, `--proxy_long_edge`; guided.py) a clip whose long edge exceeds N is shrunk
on the device, frame by frame, to the size --max_long_edge's rule gives for N (engines.shrink); everything above then runs on the shrunk
frames as on a clip of that size, and each proxy-size final frame is carried to its full-size frame by the residual guided transfer
(engines.guided_transfer: af_guided_coeffs / af_guided_apply).  `final` is full-size; every other kept sequence, the flows and E_warp
(recorded with its size) are the proxy's.  A clip no longer than N, or no flag: the calls, keys, laps and bytes of before.

With fidelity (`run(frames, fidelity=True | window, reference=...)`, `--fidelity [--reference_dir D] [--ssim_window N]`; fidelity.py,
DESIGN.md §2.17) the PSNR and SSIM of `final` against the input frames, and with a clean reference clip of the input and of `final`
against it, are taken on the device after the last stage (engines.fidelity: af_fidelity), at the clip's full size on the proxy route
too.  No flag: no call, no key, no lap.

With bits (`run(frames, bits=9..16)`, `--video_depth keep` on a stream of more than 8 bits per sample; guided.py) the
frames are uint16.  The deep route is the proxy route with a deep original: the deep frames are uploaded and kept (6 bytes per pixel),
their 8-bit reductions (engines.reduce_depth: af_depth_reduce) are the frames everything above sees, shrunk further when proxy_long_edge
says so, and after the filter is closed every final is carried to its deep frame as a smooth gain / offset field (engines.depth_transfer:
af_guided_coeffs of the 8-bit pair, af_guided_apply16).  `final` is uint16 and every bit below the eighth is the input's own; every other
kept sequence, the flows, E_warp and the fidelity report are those of the 8-bit frames.  proxy_radius and proxy_eps are its knobs (given
with proxy_long_edge, which shrinks nothing on a clip that is not longer).  No bits: the calls, keys, laps and bytes of before.

With proxy_guide="colour" (`--proxy_guide colour`) both routes carry the correction with the colour guide: every output
channel fitted on all three guide channels (af_guided_coeffs_colour / af_guided_apply_colour), so a correction that mixes channels survives
the transfer.  The engines then receive guide="colour" and the `proxy` / `depth` records gain "guide": "colour"; the default is "channel",
whose calls and records are those of before.

With --video the frames come from a YUV4MPEG2 stream (a file, or - for standard input: ffmpeg -f yuv4mpegpipe): each payload is uploaded
as it is (1.5 bytes per pixel for 4:2:0) and turned into the RGB tensor the stages read on the device (af_yuv_to_rgb); `run` sees the
same tensors a folder of PNGs with those pixels gives.  With --video_out the final frames are converted on the device (af_rgb_to_yuv,
`run(sink_device=True)`) and written as a stream in frame order instead of final/output/%05d.png; --video_out - puts the stream, and
nothing else, on standard output, and every message on standard error.  With --video, --keep_intermediates names the frames %05d.png and
writes the flows to <out>/flow.  Neither flag given: the engine calls and the frames of before.  --video_depth keep opens the stream
with Y4MReader(deep=True): an 8-bit stream runs as without the flag; a deeper one takes the deep route (af_yuv_to_rgb16 in, af_rgb_to_yuv16
out), needs --video_out (there is no deep PNG route) and its output repeats the input's layout and bits."""
import argparse
import json
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KEEP = ("final", "stage1", "filtered", "concat", "flows", "renders", "masks")
STYLE_SIZES = ("stage1", "full")
FLOW_PRECISIONS = ("fp32", "fp16")      # raft.PRECISIONS
FILTER_PRECISIONS = ("fp32", "fp16")    # stage2.PRECISIONS


def plan_windows(n_frames, max_frames, overlap=0):
    """[(start, stop)] of the windows a clip of n_frames is fitted in: k = ceil((n - overlap) / (max_frames - overlap)) windows,
    consecutive ones sharing exactly `overlap` frames, lengths differing by at most one and all <= max_frames; one window when
    n_frames <= max_frames."""
    n, m, o = int(n_frames), int(max_frames), int(overlap)
    if n < 1 or m < 1:
        raise ValueError("plan_windows: n_frames and max_frames must be positive, got %d and %d" % (n, m))
    if o < 0 or o >= m:
        raise ValueError("plan_windows: window overlap %d must be >= 0 and smaller than the window (maximum_number_of_frames %d)" % (o, m))
    if n <= m:
        return [(0, n)]
    k = -(-(n - o) // (m - o))
    total = n + (k - 1) * o                      # the windows' lengths add up to this
    base, extra = divmod(total, k)
    out, start = [], 0
    for i in range(k):
        length = base + (1 if i < extra else 0)
        out.append((start, start + length))
        start += length - o
    return out


def cross_fade_weights(overlap):
    """a_j = (j + 1) / (K + 1) for the j-th of K shared frames: the weight of the later window's render in the blend."""
    return [(j + 1) / (overlap + 1) for j in range(int(overlap))]


def seam_pairs(windows, n_frames):
    """The pairs (t, t + 1), named by t, whose two frames were not styled by the same set of windows: with hard cuts the pair across
    each cut, with overlap every pair that touches a cross-faded frame from outside or inside the blend's edge."""
    member = [frozenset(k for k, (a, b) in enumerate(windows) if a <= t < b) for t in range(n_frames)]
    return [t for t in range(n_frames - 1) if member[t] != member[t + 1]]


class DeviceEngines:
    """What Deflicker.run calls on the device: this package's three handles and the device forms of the hand-offs.  The tests replace it
    with host stubs to check the orchestration without a GPU."""

    def __init__(self, raft_sd, filter_sd, local_sd, device=0):
        self.raft_sd, self.filter_sd, self.local_sd, self.device = raft_sd, filter_sd, local_sd, int(device)

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def frame(self, x):
        """A decoded frame on the device: (H, W, 3) uint8 CUDA tensor."""
        import torch
        t = x if hasattr(x, "is_cuda") else torch.from_numpy(np.ascontiguousarray(x))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("frames must be (H, W, 3) uint8, got %s %s" % (tuple(t.shape), t.dtype))
        return t.to(self._dev()).contiguous()

    def open_flow(self, h, w, precision="fp32"):
        from .raft import RAFT
        r = RAFT(h, w, capacity=2, device=self.device, precision=precision)
        try:
            r.load_state_dict(self.raft_sd)
        except BaseException:
            r.close()
            raise
        return r

    def shrink(self, frame, h, w):
        """af_resize_area of a device frame to (h, w): the INTER_AREA shrink RAFT's input gets when the clip exceeds max_long_edge."""
        from .atlasfit import resize_area_device
        return resize_area_device(frame, h, w, device=self.device)

    def resize_flow(self, f, h, w):
        from .stage1 import resize_flow_device
        return resize_flow_device(f, h, w, device=self.device)

    def mask(self, x):
        """A decoded mask on the device: (Hm, Wm, 1) uint8 CUDA tensor, channel 0 of a mask that has channels (stage1.decode_u8(path, 1))."""
        import torch
        t = x if hasattr(x, "is_cuda") else torch.from_numpy(np.ascontiguousarray(x))
        t = t[:, :, None] if t.dim() == 2 else t[:, :, :1]
        return t.to(self._dev()).contiguous()

    def open_atlas(self, resx, resy, n_frames, config, two_layer=False):
        from . import atlasfit as A
        af = A.AtlasFit(A.default_config(resx, resy, n_frames, config, two_layer=two_layer), device=self.device)
        af.range_fallback = True      # as the stage-1 CLI: AF_ERANGE continues on the bf16x6 chains, recorded in af.arithmetic
        return af

    def resize_mask(self, mask, h, w):
        """A key mask at the stage-1 size: stage1.put_mask_device's arithmetic (u8 / 255, bilinear) into a plane of its own, (h, w) float32."""
        import torch
        from .atlasfit import resize_bilinear_device
        out = torch.empty((h, w), device=mask.device)
        resize_bilinear_device(mask, out, h, w, 1, 0, 0, device=self.device)
        return out

    def propagate_masks(self, keys, flows12, flows21, shots, thresh=1.0):
        """masks.propagate_masks_device of the resized key masks along the stage-1-size flows: (n, resy, resx) float32 on the device."""
        from .masks import propagate_masks_device
        return propagate_masks_device(keys, flows12, flows21, thresh=thresh, shots=shots)

    def inputs(self, frames, flows12, flows21, resy, resx, masks=None, mask_frames=None):
        """The builder's tensors of one window from device frames and the device flows of its internal pairs (already at resy x resx);
        with the window's device masks (two-layer path) also mask_frames, as load_input_data_device(with_masks=True) builds it, or with
        `mask_frames` (the window's propagated float planes, key-mask route) those planes copied into it."""
        from . import stage1 as S
        t = S.alloc_input_tensors(resy, resx, len(frames), self._dev(), masks is not None or mask_frames is not None)
        for i, im in enumerate(frames):
            S.put_frame_device(im, t[1], i, device=self.device)
            if masks is not None:
                S.put_mask_device(masks[i], t[5], i, device=self.device)
            elif mask_frames is not None:
                t[5][:, :, i] = mask_frames[i]
        for i, (f12, f21) in enumerate(zip(flows12, flows21)):
            S.put_flow_pair_device(f12, f21, t, i, True, device=self.device)
        return t

    def open_filter(self, h, w, precision="fp32"):
        from .stage2 import NeuralFilter
        nf = NeuralFilter(h, w, device=self.device, precision=precision)
        try:
            nf.load_state_dicts(self.filter_sd, self.local_sd)
        except BaseException:
            nf.close()
            raise
        return nf

    def resize(self, img, h, w):
        """af_resize_bilinear of an HWC image (uint8: / 255 first) to (h, w): (h, w, 3) float32."""
        import torch
        from .atlasfit import resize_bilinear_device
        out = torch.empty((h, w, 3), device=img.device)
        resize_bilinear_device(img.contiguous(), out, h, w, 3, 1, 0, device=self.device)
        return out

    def upload(self, arr):
        import torch
        a = np.ascontiguousarray(arr)
        if a.dtype == np.uint16:                              # a deep payload: storage only, the bytes travel as int16
            return torch.from_numpy(a.view(np.int16)).to(self._dev()).view(torch.uint16)
        return torch.from_numpy(a).to(self._dev())

    def quantise(self, img):
        """neural_filter.quantise on the device: clip to [0, 1], times 255 in fp32, truncated to uint8."""
        import torch
        return (img.clamp(0, 1) * 255.0).to(torch.uint8)

    def quantise_render(self, img):
        """stage1.quantise_render on the device: times 255 in fp64, truncated to uint8 (what af_render_frame_u8 applies)."""
        import torch
        return (img.double() * 255.0).to(torch.uint8)

    def lerp(self, a, b, weight):
        import torch
        return torch.lerp(a, b, float(weight))

    def concat(self, imgs):
        import torch
        return torch.cat(imgs, dim=1)

    def stack(self, imgs):
        import torch
        if imgs and imgs[0].dtype == torch.uint16:
            return torch.stack([t.view(torch.int16) for t in imgs]).view(torch.uint16)
        return torch.stack(imgs)

    def to_host(self, t):
        import torch
        if t.dtype == torch.uint16:
            return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        return t.cpu().numpy()

    def warp_error(self, img1, img2, f12, f21, align_corners):
        """E_warp of a pair of uint8 frames, read as warp_error.read_frame reads them: float32(v) / 255 of the host, through a table (a
        division on the device need not round as the host's does)."""
        import torch
        from .atlasfit import warp_error_pair
        if getattr(self, "_unit", None) is None:
            self._unit = torch.from_numpy(np.arange(256, dtype=np.float32) / 255.0).to(self._dev())
        return warp_error_pair(self._unit[img1.long()], self._unit[img2.long()], f12, f21, align_corners=align_corners, device=self.device)

    def luma_grids(self, dev_frames, gh, gw):
        """af_luma_grid of the clip's device frames: (sums int64 (n, GH, GW), counts int64 (GH, GW)) on the host, what shots.cut_scores reads."""
        from .shots import luma_grids
        return luma_grids(dev_frames, (gh, gw), device=self.device)

    def yuv_to_rgb(self, payload, h, w, layout, matrix, full_range):
        """af_yuv_to_rgb of an uploaded YUV4MPEG2 frame payload: the (h, w, 3) uint8 CUDA tensor `frame` would return for that picture."""
        from .y4m import yuv_to_rgb_device
        return yuv_to_rgb_device(payload, h, w, layout, matrix, full_range, device=self.device)

    def rgb_to_yuv(self, img, layout, matrix, full_range):
        """af_rgb_to_yuv of a device frame: its YUV4MPEG2 payload, a 1-D uint8 CUDA tensor."""
        from .y4m import rgb_to_yuv_device
        return rgb_to_yuv_device(img, layout, matrix, full_range, device=self.device)

    def guided_transfer(self, full, proxy_in, proxy_out, radius, eps, guide="channel"):
        """guided.guided_transfer_device: the correction proxy_in -> proxy_out carried to the full-size device frame, (H, W, 3) uint8."""
        from .guided import check_guide, guided_transfer_colour_device, guided_transfer_device
        fn = guided_transfer_colour_device if check_guide(guide, "guided_transfer") == "colour" else guided_transfer_device
        return fn(full, proxy_in, proxy_out, radius=radius, eps=eps)

    def frame16(self, x):
        """A deep frame on the device: (H, W, 3) torch.uint16 CUDA tensor.  The type is storage only (torch has few operators for it):
        the bytes travel as int16."""
        import torch
        if hasattr(x, "is_cuda"):
            t = x
        else:
            a = np.ascontiguousarray(x)
            if a.dtype != np.uint16:
                raise ValueError("frames must be (H, W, 3) uint16, got %s %s" % (a.shape, a.dtype))
            t = torch.from_numpy(a.view(np.int16)).to(self._dev()).view(torch.uint16)
        if t.dtype != torch.uint16 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("frames must be (H, W, 3) uint16, got %s %s" % (tuple(t.shape), t.dtype))
        return t.to(self._dev()).contiguous()

    def reduce_depth(self, frame16, bits):
        """guided.reduce_depth_device: the 8-bit reduction of a deep device frame, (H, W, 3) uint8."""
        from .guided import reduce_depth_device
        return reduce_depth_device(frame16, bits)

    def depth_transfer(self, full16, bits, proxy_in, proxy_out, radius, eps, guide="channel"):
        """guided.depth_transfer_device: the correction of the 8-bit pair carried to the deep device frame, (H, W, 3) uint16."""
        from .guided import check_guide, depth_transfer_colour_device, depth_transfer_device
        fn = depth_transfer_colour_device if check_guide(guide, "depth_transfer") == "colour" else depth_transfer_device
        return fn(full16, bits, proxy_in, proxy_out, radius=radius, eps=eps)

    def yuv_to_rgb16(self, payload, h, w, layout, matrix, full_range, bits):
        """af_yuv_to_rgb16 of an uploaded deep frame payload: the (h, w, 3) uint16 CUDA tensor `frame16` would return for that picture."""
        from .y4m import yuv_to_rgb16_device
        return yuv_to_rgb16_device(payload, h, w, layout, matrix, full_range, bits, device=self.device)

    def rgb16_to_yuv(self, img, layout, matrix, full_range, bits):
        """af_rgb_to_yuv16 of a deep device frame: its payload, a 1-D uint16 CUDA tensor."""
        from .y4m import rgb16_to_yuv_device
        return rgb16_to_yuv_device(img, layout, matrix, full_range, bits, device=self.device)

    def fidelity(self, a, b, win):
        """fidelity.frame_fidelity_device of two lists of device frames, frame by frame (the frames are tensors of their own: nothing is
        stacked): (sse uint64 (n, 3), ssim float64 (n, 3)) on the host."""
        from .fidelity import frame_fidelity_device
        rs = [frame_fidelity_device(x, y, win) for x, y in zip(a, b)]
        return np.concatenate([r["sse"] for r in rs]), np.concatenate([r["ssim"] for r in rs])

    def sync(self):
        import torch
        torch.cuda.synchronize(self._dev())


def _extra(default, **kw):
    """The keyword arguments of a route that is on: those whose value is not `default`.  An engine from before a route existed has no
    such parameter, so a run without the route must not pass it.  None is told by identity alone: a route's value may be an array."""
    return {k: v for k, v in kw.items() if not (v is default or (default is not None and v == default))}


def _sized(seq, first=True):
    """(n, first item) of a sequence with a known length: n is None for an iterator, the item None where seq is empty or cannot be
    indexed (or `first` is False: the caller wants the length alone and seq[0] is not touched)."""
    n = len(seq) if hasattr(seq, "__len__") else None
    return n, (seq[0] if first and n and hasattr(seq, "__getitem__") else None)


def _one_of(name, value, allowed):
    if value not in allowed:
        raise ValueError("Deflicker: %s must be one of %s, got %r" % (name, ", ".join(allowed), value))
    return value


class _Run:
    """What one Deflicker.run accumulates, phase by phase; nothing of a run is kept on the Deflicker."""
    __slots__ = ("E", "keep", "sink", "sink_device", "tensor_in", "fid_win", "seconds", "t0",      # the call's own
                 "h", "w", "resx", "resy", "flow_size",                                          # the clip's sizes (_flows, at frame 0)
                 "dev_frames", "full_frames", "dev_masks", "dev_keys",                           # full_frames: None off the proxy route
                 "small12", "small21", "full",                                                   # flows: at the stage-1 size, and as RAFT gave them
                 "shots", "scores", "cuts_at", "prop",
                 "windows", "seams", "styles", "psnr", "psnr_full", "arithmetic", "renders",
                 "out", "proxy_finals", "measured",
                 "bits", "deep_frames")                                                          # the deep route: None off it

    def __init__(self, engines, keep, sink, sink_device, tensor_in, fid_win):
        for name in self.__slots__:
            setattr(self, name, None)
        self.E, self.keep, self.sink, self.sink_device, self.tensor_in, self.fid_win = engines, keep, sink, sink_device, tensor_in, fid_win
        self.out, self.proxy_finals, self.measured = {}, [], {}
        self.seconds, self.t0 = {}, time.perf_counter()

    @property
    def proxied(self):
        return self.full_frames is not None

    @property
    def deep(self):
        return self.deep_frames is not None

    @property
    def carried(self):
        """The finals the filter makes are not the run's `final`: they are carried to a larger or deeper original afterwards."""
        return self.proxied or self.deep

    def lap(self, name):
        self.E.sync()
        t1 = time.perf_counter()
        self.seconds[name] = round(t1 - self.t0, 4)
        self.t0 = t1

    def emit(self, name, i, t):
        """Frame i of a kept sequence: held for the result, and handed to the sink as soon as it exists."""
        if name in self.out:
            self.out[name].append(t)
            if self.sink is not None:
                self.sink(name, i, t if self.sink_device else self.E.to_host(t))


class Deflicker:
    """frames -> deflickered frames on one MI355X: RAFT, the stage-1 atlas fit per window, the neural filter, all in this process."""

    def __init__(self, raft_sd, filter_sd, local_sd, config=None, down=4, seed=None, window_overlap=0, device=0, max_long_edge=2000,
                 engines=None, style_size="stage1", flow_precision="fp32", filter_precision="fp32", cuts=None,
                 cut_threshold=None, cut_margin=None, cut_radius=None, min_shot_frames=None, mask_thresh=None,
                 proxy_long_edge=None, proxy_radius=None, proxy_eps=None, proxy_guide=None):
        from .atlasfit import REFERENCE_CONFIG
        self._init_mask_thresh(mask_thresh)
        self._init_proxy(proxy_long_edge, proxy_radius, proxy_eps, proxy_guide)
        self.config = dict(REFERENCE_CONFIG)
        if config:
            self.config.update(config)
        if self.config["load_checkpoint"]:
            raise ValueError("Deflicker: load_checkpoint is not supported (every window starts from the seeded init)")
        self.style_size = _one_of("style_size", style_size, STYLE_SIZES)
        self.flow_precision = _one_of("flow_precision", flow_precision, FLOW_PRECISIONS)
        self.filter_precision = _one_of("filter_precision", filter_precision, FILTER_PRECISIONS)
        self.down, self.seed, self.overlap, self.device, self.max_long_edge = down, seed, int(window_overlap), int(device), int(max_long_edge)
        plan_windows(2, int(self.config["maximum_number_of_frames"]), self.overlap)      # rejects a bad overlap before any work
        self.schedule = _schedule(self.config)
        self.engines = engines if engines is not None else DeviceEngines(raft_sd, filter_sd, local_sd, device)
        self._init_cuts(cuts, cut_threshold, cut_margin, cut_radius, min_shot_frames)
        if self.proxy_long_edge is not None and not (hasattr(self.engines, "shrink") and hasattr(self.engines, "guided_transfer")):
            raise ValueError("Deflicker: proxy_long_edge needs an engine with shrink and guided_transfer; %s lacks one" % type(self.engines).__name__)

    def _init_mask_thresh(self, mask_thresh):
        """The round-trip bound of the key-mask propagation (masks.py); None: its default."""
        from .masks import DEFAULT_THRESH, _check_thresh
        try:
            self.mask_thresh = _check_thresh(DEFAULT_THRESH if mask_thresh is None else mask_thresh)
        except ValueError as e:
            raise ValueError("Deflicker: mask_thresh: %s" % e)

    def _init_proxy(self, long_edge, radius, eps, guide=None):
        """The proxy route (guided.py): None = the clip's own size; radius and eps None: guided.py's defaults; guide None:
        "channel"."""
        from .guided import DEFAULT_EPS, DEFAULT_RADIUS, check_guide, check_guided
        if long_edge is not None and (isinstance(long_edge, bool) or not isinstance(long_edge, (int, np.integer)) or long_edge < 1):
            raise ValueError("Deflicker: proxy_long_edge must be None or a positive integer, got %r" % (long_edge,))
        if long_edge is None and (radius is not None or eps is not None):
            raise ValueError("Deflicker: proxy_radius and proxy_eps belong to the proxy route: they need proxy_long_edge")
        if long_edge is None and guide is not None:
            raise ValueError("Deflicker: proxy_guide belongs to the proxy route: it needs proxy_long_edge")
        self.proxy_long_edge = None if long_edge is None else int(long_edge)
        self.proxy_guide = check_guide("channel" if guide is None else guide, "Deflicker: proxy")
        self.proxy_radius, self.proxy_eps = check_guided(DEFAULT_RADIUS if radius is None else radius, DEFAULT_EPS if eps is None else eps, "Deflicker: proxy",
                                                         self.proxy_guide)

    def _init_cuts(self, cuts, threshold, margin, radius, min_shot_frames):
        """Scene cuts (shots.py): None = one shot, "auto" = detected on the device, or the first frames of the new
        shots; a knob left None takes shots.CUT_DEFAULTS."""
        from .shots import CUT_DEFAULTS, detect_cuts, plan_shots
        knobs = {"threshold": threshold, "margin": margin, "radius": radius, "min_shot_frames": min_shot_frames}
        knobs = {k: CUT_DEFAULTS[k] if v is None else v for k, v in knobs.items()}
        self.cut_threshold, self.cut_margin, self.cut_radius, self.min_shot_frames = float(knobs["threshold"]), float(knobs["margin"]), int(knobs["radius"]), int(knobs["min_shot_frames"])
        if cuts is None or (isinstance(cuts, str) and cuts == "auto"):
            self.cuts = cuts
        elif isinstance(cuts, (list, tuple, np.ndarray)):
            self.cuts = [c for c in cuts]
            if self.cuts:
                try:
                    plan_shots(2 ** 62, self.cuts)            # what can be refused without the clip's length
                    self.cuts = [int(c) for c in self.cuts]
                except ValueError as e:
                    raise ValueError("Deflicker: cuts: %s" % e)
        else:
            raise ValueError("Deflicker: cuts must be None, \"auto\" or a sequence of first-frame indices of new shots, got %r" % (cuts,))
        if self.cuts == "auto":
            if not hasattr(self.engines, "luma_grids"):
                raise ValueError("Deflicker: cuts=\"auto\" needs an engine with luma_grids (the luminance grids of the device frames); %s has none"
                                 % type(self.engines).__name__)
            detect_cuts([], self.cut_threshold, self.cut_margin, self.cut_radius, self.min_shot_frames)      # rejects bad knobs before any work

    # ---- stage 0: RAFT over the clip (preprocess_optical_flow.preprocess) -------------------------------------------------
    def _upload(self, frames):
        """The clip on the device before anything else runs (cuts="auto": the scores need every frame, so RAFT cannot overlap the decode)."""
        dev_frames = []
        for i, x in enumerate(frames):
            t = self.engines.frame(x)
            if dev_frames and tuple(t.shape[:2]) != tuple(dev_frames[0].shape[:2]):
                raise ValueError("frame %d is %dx%d, the first frame %dx%d" % (i, t.shape[1], t.shape[0], dev_frames[0].shape[1], dev_frames[0].shape[0]))
            dev_frames.append(t)
        return dev_frames

    def _proxy(self, frames):
        """The proxy route's first step.  The first frame's size decides (read from the frame as given: no engine call): a clip no longer
        than proxy_long_edge -> (frames, None), and the run is the default's; a longer one -> (proxy frames, full-size device frames):
        the clip uploaded and every frame shrunk to preprocess_optical_flow.shrink_size(h, w, proxy_long_edge) (engines.shrink)."""
        import itertools
        from .preprocess_optical_flow import shrink_size
        first = _sized(frames)[1]
        if first is None:                                     # an iterator: its first frame is looked at and put back
            frames = iter(frames)
            first = next(frames, None)
            frames = itertools.chain([first], frames) if first is not None else iter(())
        if first is None or not hasattr(first, "shape") or len(first.shape) != 3:
            return frames, None                               # the default route names what is wrong with it
        try:
            small = shrink_size(int(first.shape[0]), int(first.shape[1]), self.proxy_long_edge, name="frame 0")
        except ValueError as e:
            raise ValueError(str(e).replace("--max_long_edge", "proxy_long_edge"))
        if small is None:
            return frames, None
        full = self._upload(frames)
        return [self.engines.shrink(t, small[0], small[1]) for t in full], full

    def _flows(self, r, frames, keep_full, starts=(), uploaded=False):
        """RAFT over `frames`, into r: its sizes (set when frame 0 is seen), dev_frames, small12, small21 and, with keep_full, full.
        `starts`: the first frames of the shots after the first.  No pair across a cut is computed (its entries are None), and a
        shot's frames take the slots its stand-alone run would give them: parity restarts at its first frame.  `uploaded`: `frames`
        are device frames already (_upload)."""
        from .preprocess_optical_flow import shrink_size
        E = self.engines
        r.dev_frames, r.small12, r.small21, r.full = dev_frames, small12, small21, full = [], [], [], []
        raft, prev, small = None, None, None
        starts, first = set(starts), 0
        try:
            for i, x in enumerate(frames):
                t = x if uploaded else E.frame(x)
                h, w = int(t.shape[0]), int(t.shape[1])
                if raft is None:
                    small = shrink_size(h, w, self.max_long_edge, name="frame 0")      # None: RAFT sees the frames as they are
                    r.h, r.w = h, w
                    r.flow_size = small if small is not None else (h, w)
                    r.resx, r.resy = (int(w / self.down), int(h / self.down)) if self.down is not None else (w, h)
                    # fp32 leaves the call as it was; fp16: RAFT in the reference's GPU arithmetic (raft.py)
                    raft = E.open_flow(*r.flow_size, **_extra("fp32", precision=self.flow_precision))
                elif (h, w) != (r.h, r.w):
                    raise ValueError("frame %d is %dx%d, the first frame %dx%d" % (i, w, h, r.w, r.h))
                dev_frames.append(t)
                if i in starts:                               # a new shot: no flow reaches back across the cut
                    prev, first = None, i
                    small12.append(None)
                    small21.append(None)
                    if keep_full:
                        full.append(None)
                cur = (i - first) & 1                         # two live frames: the slot not holding frame i - 1
                raft.encode(cur, t if small is None else E.shrink(t, small[0], small[1]))      # the shrunk frame feeds RAFT only
                if prev is not None:
                    f12, f21 = raft.flow_slots([(prev, cur), (cur, prev)], on_device=True)      # both directions in one launch (capacity 2)
                    small12.append(E.resize_flow(f12, r.resy, r.resx))
                    small21.append(E.resize_flow(f21, r.resy, r.resx))
                    if keep_full:
                        full.append((f12, f21))
                prev = cur
        finally:
            if raft is not None:
                raft.close()                                  # before stage 1 trains: its buffers are free for the fit

    # ---- stage 1: one window, the schedule of stage1.main ---------------------------------------------------------------
    def _fit_window(self, r, k, a, b, want_float):
        """-> (u8 renders, float renders or None, mean PSNR, arithmetic) of window k, frames a .. b - 1 of r, fitted as a stand-alone
        clip with seed + k; with the window's own masks (r.dev_masks) or its propagated planes (r.prop, key-mask route) as a stand-alone
        two-layer clip.  A single-atlas window calls the engines without the two-layer arguments.  style_size "full": the renders are
        the nets at the frames' own size (render_frame_at_device, the device frame as its reference), the stage-1-size render runs for
        its error sum only, and the window's mean full-size PSNR is appended to r.psnr_full."""
        import torch
        from . import stage1 as S
        E, cfg = self.engines, self.config
        frames, n = r.dev_frames[a:b], b - a
        mask_args = _extra(None, masks=None if r.dev_masks is None else r.dev_masks[a:b], mask_frames=None if r.prop is None else r.prop[a:b])
        two_layer = bool(mask_args)
        af = E.open_atlas(r.resx, r.resy, n, cfg, **_extra(False, two_layer=two_layer))
        try:
            gen = torch.Generator().manual_seed(int(self.seed) + k) if self.seed is not None else None
            jobs = S.init_networks(af, cfg, two_layer, gen)   # draws in the reference's order: init, pre-train seed(s), sampler seed
            pre, err = S.start_pretrain(af, cfg, jobs)        # overlapped with the builder, as in stage1.main
            try:                                              # no flow crosses a window's last frame: pairs a .. b - 2 only
                t = E.inputs(frames, r.small12[a:b - 1], r.small21[a:b - 1], r.resy, r.resx, **mask_args)
            finally:
                pre.join()                                    # the thread owns the handle until it ends
            if err:
                raise err[0]
            flows_mask, video_frames, flows_rev_mask, flows_rev, flows = t[:5]
            af.upload_video(video_frames, flows, flows_rev, flows_mask, flows_rev_mask, *t[5:6])      # mask_frames: two-layer only
            sampler_seed = int(torch.randint(2 ** 31, (1,), generator=gen))
            last_eval = max(i for i, s in enumerate(self.schedule) if s[3])
            for i, (first, count, _stop, _evaluate) in enumerate(self.schedule):
                af.train_steps(first, count, None, seed=sampler_seed, return_losses=False)
                if i == last_eval:                            # what the CLI leaves in stage_1/output: the last evaluation's render
                    u8s, floats, psnrs, full = [], [], [], []
                    for f in range(n):
                        if self.style_size == "full":
                            _, _, sse = af.render_frame_device(f, want_float=False, want_u8=False)
                            rgb, u8, sse_full = af.render_frame_at_device(f, r.h, r.w, want_float=want_float, want_u8=True, ref=frames[f])
                            full.append(S.frame_psnr(sse_full, r.h * r.w * 3))
                        else:
                            rgb, u8, sse = af.render_frame_device(f, want_float=want_float, want_u8=True)
                        u8s.append(u8)
                        floats.append(rgb)
                        psnrs.append(S.frame_psnr(sse, r.resx * r.resy * 3))
                    if full:
                        r.psnr_full.append(float(np.mean(full)))
            return u8s, (floats if want_float else None), float(np.mean(psnrs)), dict(af.arithmetic)
        finally:
            af.close()

    # ---- the check phase: what can be refused before any work ----------------------------------------------------------------
    @staticmethod
    def _check_mask(i, m):
        if not hasattr(m, "dtype") or str(m.dtype) not in ("uint8", "torch.uint8"):
            raise ValueError("mask %d must be uint8, got %s" % (i, getattr(m, "dtype", type(m).__name__)))
        if m.ndim not in (2, 3) or (m.ndim == 3 and m.shape[2] < 1):
            raise ValueError("mask %d must be (Hm, Wm) or (Hm, Wm, C), got %s" % (i, tuple(m.shape)))
        return m

    def _masks(self, masks, n):
        """The masks on the device as uint8, one (Hm, Wm, 1) tensor per frame, checked before any other work starts.  n: the clip's
        length, None when it is not known yet."""
        if hasattr(masks, "ndim") and hasattr(masks, "shape"):      # one array or tensor for the clip
            if str(masks.dtype) not in ("uint8", "torch.uint8"):
                raise ValueError("masks must be uint8, got %s" % (masks.dtype,))
            if masks.ndim not in (3, 4):
                raise ValueError("masks must be (N, Hm, Wm) or (N, Hm, Wm, C) uint8, got %s" % (tuple(masks.shape),))
        if hasattr(masks, "__len__") and n is not None and len(masks) != n:
            raise ValueError("%d masks for %d frames: the two-layer path needs one mask per frame" % (len(masks), n))
        return [self.engines.mask(self._check_mask(i, m)) for i, m in enumerate(masks)]

    def _mask_keys(self, mask_keys, n):
        """The key masks on the device as uint8, {frame index: (Hm, Wm, 1) tensor}; what can be refused is refused before the first upload."""
        from .masks import plan_mask_propagation
        from .shots import plan_shots
        if not hasattr(mask_keys, "items"):
            raise ValueError("mask_keys must be a {frame index: uint8 mask} mapping, got %s" % type(mask_keys).__name__)
        keys = {}
        for i, m in mask_keys.items():
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
                raise ValueError("mask_keys: frame index %r is not an integer" % (i,))
            keys[int(i)] = self._check_mask(int(i), m)
        if n is not None:                                     # the clip has a length: the planner's refusals come before any work
            explicit = self.cuts and self.cuts != "auto"
            plan_mask_propagation(n, keys, plan_shots(n, self.cuts) if explicit else None)
        else:                                                 # an iterator: no keys and a negative index now, the rest after the decode
            plan_mask_propagation(max(keys, default=0) + 1, keys)
        return {i: self.engines.mask(keys[i]) for i in sorted(keys)}

    def _check_fidelity(self, fidelity, reference, frames, masks_only):
        """The SSIM window of `run(fidelity=...)`, None when it is off; everything that can be refused before any work is refused here."""
        from .fidelity import DEFAULT_WINDOW, check_window
        if fidelity is None or fidelity is False:
            if reference is not None:
                raise ValueError("reference belongs to the fidelity report: it needs fidelity")
            return None
        win = DEFAULT_WINDOW if fidelity is True else check_window(fidelity, "fidelity")
        if masks_only:
            raise ValueError("fidelity compares the final frames: masks_only leaves none")
        if not hasattr(self.engines, "fidelity"):
            raise ValueError("fidelity needs an engine with fidelity; %s has none" % type(self.engines).__name__)
        if reference is not None:
            if not hasattr(reference, "__len__"):
                raise ValueError("reference must be a sequence of (H, W, 3) uint8 frames or one (N, H, W, 3) uint8 CUDA tensor, got %s" % type(reference).__name__)
            n, first = _sized(frames)
            self._check_reference(reference, n, tuple(first.shape[:2]) if first is not None and hasattr(first, "shape") and len(first.shape) == 3 else None)
        return win

    @staticmethod
    def _check_reference(reference, n, hw):
        """ValueError unless `reference` is n uint8 frames of (h, w, 3); n or hw None: not known yet."""
        if n is not None and len(reference) != n:
            raise ValueError("%d reference frames for %d frames: the reference is a clip of the same length" % (len(reference), n))
        for i, r in enumerate(reference):
            if not hasattr(r, "shape") or len(r.shape) != 3 or r.shape[2] != 3 or str(r.dtype) not in ("uint8", "torch.uint8"):
                raise ValueError("reference frame %d must be (H, W, 3) uint8, got %s %s" % (i, tuple(getattr(r, "shape", ())), getattr(r, "dtype", type(r).__name__)))
            if hw is not None and (int(r.shape[0]), int(r.shape[1])) != (int(hw[0]), int(hw[1])):
                raise ValueError("reference frame %d is %dx%d, the clip %dx%d: the reference has the clip's full size" % (i, r.shape[1], r.shape[0], hw[1], hw[0]))

    # ---- the pipeline -------------------------------------------------------------------------------------------------------
    def run(self, frames, masks=None, keep=("final",), sink=None, warp_error=None, sink_device=False, mask_keys=None, masks_only=False,
            fidelity=None, reference=None, bits=None):
        """The routes are the module's text; this is the call.  frames: a sequence (or iterator) of HWC uint8 numpy arrays, or one
        (N, H, W, 3) uint8 CUDA tensor.  masks: None (one atlas per window), or one uint8 mask per frame (channel 0 of a mask with
        channels) as a sequence or iterator of arrays or one uint8 CUDA tensor (N, Hm, Wm[, C]).  Returns a dict: `final`
        (N, H, W, 3) uint8 (a CUDA tensor when the input was one, else numpy), on request (`keep`) `stage1` (the styles: stage-1 size, or
        with style_size "full" the frames' own size),
        `filtered`, `concat`, `flows` ([(flow12, flow21)] at RAFT's padded size: of the shrunk frames when the clip is longer than
        max_long_edge; None at a pair across a scene cut) and `renders` (per window, its float renders); `psnr` (stage 1's per window), `windows`, `seam_pairs`,
        `shots` ([(start, stop)]), `cut_pairs`, `cuts` (as given), `cut_scores` (with cuts="auto": the score of every pair, else None), `arithmetic`,
        `two_layer`, `style_size`, `psnr_full` (with style_size "full": per window, the mean PSNR of the full-size renders against the
        full-size frames; else None), `flow_size` ((h, w) RAFT ran at, before padding: the frames' size unless they were shrunk), `max_long_edge`, `flow_precision`, `filter_precision`,
        `seconds` (wall clock per stage between device synchronisations).  sink(name, index, uint8 array): called with every frame of `final` and of the kept u8 sequences as soon as
        it is on the host (the CLI's PNG encoders); with sink_device the sink receives the engine's device tensor instead of a host copy (the
        CLI's video sink converts `final` to YCbCr on the device); warp_error: None, or align_corners of E_warp of the input and of `final`.
        mask_keys: instead of `masks`, {frame index: uint8 mask} for a few frames (at least one per shot); `keep` "masks" returns the
        propagated (N, resy, resx) float32 planes, `mask_keys` in the result is the sorted key indices (None on every other route).
        masks_only: stop after the propagation; the result then holds `masks` and the records of the stages that ran.
        With proxy_long_edge and a longer clip the result gains `proxy` ({"size": [h, w], "radius", "eps"}), `seconds` the laps "proxy"
        (upload and shrink) and "transfer", and `warp_error`, of the proxy-size input and finals, its "size".
        fidelity: None, True (window 7) or an odd SSIM window in 3..15: the result gains `fidelity` = {"window", "size": [H, W],
        "final_vs_input": fidelity.summarise(...)} and `seconds` the lap "fidelity"; reference: with fidelity, a sequence of uint8 frames or
        one (N, H, W, 3) uint8 CUDA tensor of the clip's full size and length (a clean clip): also "input_vs_reference" and
        "final_vs_reference".
        bits: None, or 9..16: the frames are HWC uint16 numpy arrays (a sequence or an iterator) or one (N, H, W, 3) torch.uint16 CUDA
        tensor holding that many bits per sample; `final` is uint16, the result gains `depth` ({"bits", "radius", "eps"}), `seconds`
        the laps "depth" (upload and reduction) and "transfer"; the fidelity report is that of the 8-bit reduction of `final` against the
        8-bit input and says "bits": 8.  A deep `reference` is not handled: it is 8-bit frames as on every other route.
        The work is the phases below, in this order, over one _Run that holds everything the call accumulates."""
        bits = self._check_bits(bits, frames)
        r = self._check(frames, masks, keep, sink, sink_device, mask_keys, masks_only, fidelity, reference)
        r.bits = bits
        self._ingest(r, frames, "flows" in r.keep or warp_error is not None, reference)
        self._propagate(r)
        if masks_only:
            return self._result(r, masks_only=True)
        self._fit(r)
        self._filter(r)
        self._transfer(r)
        self._measure(r, warp_error, reference)
        return self._result(r)

    def _check(self, frames, masks, keep, sink, sink_device, mask_keys, masks_only, fidelity, reference):
        """Everything that can be refused before any work; then the run's state, its clock started, with the masks or the key masks
        uploaded."""
        from .shots import plan_shots
        E = self.engines
        keep = set(keep)
        if keep - set(KEEP):
            raise ValueError("keep: unknown %s (known: %s)" % (sorted(keep - set(KEEP)), ", ".join(KEEP)))
        tensor_in = hasattr(frames, "is_cuda")
        if tensor_in and (frames.dim() != 4 or frames.shape[3] != 3):
            raise ValueError("frames must be (N, H, W, 3) uint8, got %s" % (tuple(frames.shape),))
        n = _sized(frames, first=False)[0]
        if n is not None and n < 2:
            raise ValueError("a clip needs at least 2 frames, got %d" % n)
        if masks is not None and mask_keys is not None:
            raise ValueError("masks and mask_keys are mutually exclusive: one mask per frame, or key masks to propagate")
        if mask_keys is None and ("masks" in keep or masks_only):
            raise ValueError("keep \"masks\" and masks_only belong to the key-mask route: they need mask_keys")
        if mask_keys is not None and not hasattr(E, "propagate_masks"):
            raise ValueError("mask_keys needs an engine with propagate_masks; %s has none" % type(E).__name__)
        fid_win = self._check_fidelity(fidelity, reference, frames, masks_only)
        r = _Run(E, keep, sink, sink_device, tensor_in, fid_win)
        if self.cuts and self.cuts != "auto" and n is not None:
            plan_shots(n, self.cuts)                          # explicit cuts that do not fit the clip: refused before any work
        r.dev_masks = self._masks(masks, n) if masks is not None else None
        r.dev_keys = self._mask_keys(mask_keys, n) if mask_keys is not None else None
        return r

    def _check_bits(self, bits, frames):
        """run's `bits`: None, or an integer in 9..16 with uint16 frames and an engine that has the deep route's hand-offs."""
        if bits is None:
            return None
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 9 <= int(bits) <= 16:
            raise ValueError("bits must be None or an integer in 9..16 (bits per sample of uint16 frames), got %r" % (bits,))
        missing = [m for m in ("frame16", "reduce_depth", "depth_transfer") if not hasattr(self.engines, m)]
        if missing:
            raise ValueError("bits needs an engine with frame16, reduce_depth and depth_transfer; %s lacks %s" % (type(self.engines).__name__, ", ".join(missing)))
        first = frames if hasattr(frames, "is_cuda") else _sized(frames)[1]
        if first is not None:
            self._check_deep_frame(0, first, int(bits))
        return int(bits)

    @staticmethod
    def _check_deep_frame(i, x, bits):
        if str(getattr(x, "dtype", None)) not in ("uint16", "torch.uint16"):
            raise ValueError("bits=%d: frame %d must be uint16, got %s (8-bit frames run without bits)" % (bits, i, getattr(x, "dtype", type(x).__name__)))

    def _deepen(self, r, frames):
        """The deep route's first step: the deep frames on the device (kept for the run) -> their 8-bit reductions, the frames every
        stage sees."""
        E = r.E
        r.deep_frames = []
        for i, x in enumerate(frames):
            self._check_deep_frame(i, x, r.bits)
            t = E.frame16(x)
            if r.deep_frames and tuple(t.shape[:2]) != tuple(r.deep_frames[0].shape[:2]):
                raise ValueError("frame %d is %dx%d, the first frame %dx%d" % (i, t.shape[1], t.shape[0], r.deep_frames[0].shape[1], r.deep_frames[0].shape[0]))
            r.deep_frames.append(t)
        return [E.reduce_depth(t, r.bits) for t in r.deep_frames]

    # ---- the phases of a run, in the order `run` calls them -----------------------------------------------------------------
    def _ingest(self, r, frames, keep_full, reference):
        """The clip on the device, its flows and its shots; what could not be counted before the decode is counted here."""
        from .shots import GRID, cut_pairs, cut_scores, detect_cuts, plan_shots
        if r.bits is not None:                                # the deep route: from here on `frames` are the 8-bit device frames
            frames = self._deepen(r, frames)
            r.lap("depth")
        if self.proxy_long_edge is not None:                  # the proxy route: from here on `frames` are the shrunk device frames
            frames, r.full_frames = self._proxy(frames)
            if r.proxied:
                r.lap("proxy")

        def check_counts(dev_frames):
            n = len(dev_frames)
            if n < 2:
                raise ValueError("a clip needs at least 2 frames, got %d" % n)
            if r.dev_masks is not None and len(r.dev_masks) != n:
                raise ValueError("%d masks for %d frames: the two-layer path needs one mask per frame" % (len(r.dev_masks), n))
            if reference is not None:                         # of the clip's own size: the proxy's is not
                self._check_reference(reference, n, tuple((r.full_frames if r.proxied else dev_frames)[0].shape[:2]))
            return n

        if self.cuts == "auto":                               # every frame first, scored on the device; RAFT afterwards, within the shots
            dev_frames = frames if r.carried else self._upload(frames)
            n = check_counts(dev_frames)
            r.scores = cut_scores(*r.E.luma_grids(dev_frames, GRID[0], GRID[1]))
            r.shots = plan_shots(n, detect_cuts(r.scores, self.cut_threshold, self.cut_margin, self.cut_radius, self.min_shot_frames))
            r.lap("decode + cuts")
            self._flows(r, dev_frames, keep_full, starts=[a for a, _ in r.shots[1:]], uploaded=True)
            r.lap("flow")
        else:
            self._flows(r, frames, keep_full, starts=self.cuts or (), uploaded=r.carried)
            n = check_counts(r.dev_frames)
            r.shots = plan_shots(n, self.cuts) if self.cuts else [(0, n)]
            r.lap("decode + flow")
        r.cuts_at = cut_pairs(r.shots)

    def _propagate(self, r):
        """Key masks -> the masks of the whole clip, shot by shot, before any fit."""
        if r.dev_keys is None:
            return
        from .masks import DEFAULT_THRESH, plan_mask_propagation
        plan_mask_propagation(len(r.dev_frames), r.dev_keys, r.shots)      # a stream's length and the detected shots are known only now
        small_keys = {i: r.E.resize_mask(m, r.resy, r.resx) for i, m in r.dev_keys.items()}
        r.prop = r.E.propagate_masks(small_keys, r.small12, r.small21, r.shots, **_extra(DEFAULT_THRESH, thresh=self.mask_thresh))
        r.lap("masks")

    def _fit(self, r):
        """Stage 1: every shot is windowed as a clip of its own; the windows are numbered in clip order, window k is fitted with
        seed + k, and the frames two windows share are cross-faded."""
        E, n = r.E, len(r.dev_frames)
        r.windows = windows = [(a + lo, a + hi) for a, b in r.shots for lo, hi in plan_windows(b - a, int(self.config["maximum_number_of_frames"]), self.overlap)]
        r.seams = [t for t in seam_pairs(windows, n) if t not in r.cuts_at]
        want_float = self.overlap > 0 or "renders" in r.keep
        styles, members = [None] * n, [0] * n
        r.psnr, r.psnr_full, r.arithmetic, r.renders = [], [], [], []
        for k, (a, b) in enumerate(windows):
            u8s, floats, p, arith = self._fit_window(r, k, a, b, want_float)
            r.psnr.append(p)
            r.arithmetic.append(arith)
            if "renders" in r.keep:
                r.renders.append(E.stack(floats))
            shared = cross_fade_weights(windows[k - 1][1] - a) if k else []
            for i in range(a, b):
                if members[i] == 0:
                    styles[i] = u8s[i - a] if not want_float else (u8s[i - a], floats[i - a])
                else:                                         # a frame the earlier window(s) rendered too: lerp of the float renders
                    blend = E.lerp(styles[i][1], floats[i - a], shared[i - a])
                    styles[i] = (E.quantise_render(blend), blend)
                members[i] += 1
        r.styles = [s[0] for s in styles] if want_float else styles
        r.lap("stage 1")

    def _filter(self, r):
        """Stage 2 over the whole clip in frame order; the kept sequences are emitted frame by frame."""
        E, h, w = r.E, r.h, r.w
        r.out = out = {name: [] for name in ("final", "stage1", "filtered", "concat") if name in r.keep or name == "final"}
        # fp32 leaves the call as it was; fp16: both stage-2 nets as the reference's modules compute them under fp16 autocast (stage2.py)
        nf = E.open_filter(h, w, **_extra("fp32", precision=self.filter_precision))
        try:
            nf.reset()
            for i in range(len(r.dev_frames)):
                if i and i - 1 in r.cuts_at:                  # a new shot starts as a clip starts: no recurrent state across the cut
                    nf.reset()
                r.emit("stage1", i, r.styles[i])
                content = E.resize(r.dev_frames[i], h, w)     # same size: u8 / 255, as load_image(resize=False)
                style = E.resize(r.styles[i], h, w)           # load_image(size=org_size): to the content's size
                pred, final = nf.frame(content, style)
                if "filtered" in out or "concat" in out:
                    pred_q = E.quantise(E.resize(pred, h, w))
                    r.emit("filtered", i, pred_q)
                if "concat" in out:                           # the padded content and style the nets saw, resized back
                    padded = E.upload(nf.activation("input"))
                    r.emit("concat", i, E.concat([E.quantise(E.resize(padded[..., :3], h, w)), E.quantise(E.resize(padded[..., 3:], h, w)), pred_q]))
                final = E.quantise(E.resize(final, h, w))
                if r.carried:                                 # carried to the full size / the deep frame after the filter is closed
                    r.proxy_finals.append(final)
                else:
                    r.emit("final", i, final)
        finally:
            nf.close()
        r.lap("stage 2")

    def _transfer(self, r):
        """Proxy route: each proxy-size final to its full-size frame (guided.py).  Deep route: each 8-bit final, shrunk or not, to its
        deep frame, with the coefficients of the 8-bit pair the run holds."""
        guide = _extra("channel", guide=self.proxy_guide)      # an engine from before the colour guide has no such parameter
        if r.deep:
            for i, deep in enumerate(r.deep_frames):
                r.emit("final", i, r.E.depth_transfer(deep, r.bits, r.dev_frames[i], r.proxy_finals[i], self.proxy_radius, self.proxy_eps, **guide))
            r.lap("transfer")
            return
        if not r.proxied:
            return
        for i, full in enumerate(r.full_frames):
            r.emit("final", i, r.E.guided_transfer(full, r.dev_frames[i], r.proxy_finals[i], self.proxy_radius, self.proxy_eps, **guide))
        r.lap("transfer")

    def _measure(self, r, warp_error, reference):
        """E_warp and the fidelity report, each only when asked for, into r.measured."""
        E = r.E
        if warp_error is not None:                            # proxy route: of the proxy-size input and finals, whose flows the run holds
            rec = r.measured["warp_error"] = self._warp_error(r, r.proxy_finals if r.carried else r.out["final"], bool(warp_error))
            if r.proxied:
                rec["size"] = [int(r.h), int(r.w)]
            r.lap("warp error")
        if r.fid_win is not None:                             # of the clip's own size: the full-size input and final on the proxy route too
            from .fidelity import summarise
            src, final, win = r.full_frames if r.proxied else r.dev_frames, r.out["final"], r.fid_win
            if r.deep:                                        # the 8-bit reduction of the deep finals against the 8-bit full-size input
                final = [E.reduce_depth(t, r.bits) for t in final]
            fh, fw = int(src[0].shape[0]), int(src[0].shape[1])
            rec = r.measured["fidelity"] = {"window": win, "size": [fh, fw], **({"bits": 8} if r.deep else {}),
                                            "final_vs_input": summarise(*E.fidelity(final, src, win), fh, fw)}
            if reference is not None:
                ref = [E.frame(x) for x in reference]
                rec["input_vs_reference"] = summarise(*E.fidelity(src, ref, win), fh, fw)
                rec["final_vs_reference"] = summarise(*E.fidelity(final, ref, win), fh, fw)
            r.lap("fidelity")

    def _result(self, r, masks_only=False):
        """The dict `run` returns, from the run's state; masks_only: the shorter record of a run that stopped after the propagation."""
        E, keep = r.E, r.keep

        def host(t):
            return t if r.tensor_in else E.to_host(t)

        cuts = {"shots": r.shots, "cut_pairs": r.cuts_at, "cuts": self.cuts if self.cuts is None or self.cuts == "auto" else list(self.cuts),
                "cut_scores": [float(v) for v in r.scores] if r.scores is not None else None}
        flow = {"flow_size": [int(v) for v in r.flow_size], "max_long_edge": self.max_long_edge, "flow_precision": self.flow_precision}
        masks = {"mask_keys": sorted(r.dev_keys) if r.dev_keys is not None else None, "mask_thresh": self.mask_thresh}
        two_layer = {"two_layer": r.dev_masks is not None or r.prop is not None}
        guide = _extra("channel", guide=self.proxy_guide)      # recorded only when it is not the default
        proxy = {"proxy": {"size": [int(r.h), int(r.w)], "radius": self.proxy_radius, "eps": self.proxy_eps, **guide}} if r.proxied else {}
        if r.deep:                                            # beside `proxy`, which is there when the 8-bit frames were shrunk too
            proxy = {**proxy, "depth": {"bits": r.bits, "radius": self.proxy_radius, "eps": self.proxy_eps, **guide}}
        flows = {"flows": r.full} if "flows" in keep else {}
        if masks_only:
            res = {"masks": host(r.prop), **masks, **cuts, **two_layer, **flow, **flows, **proxy}
        else:
            res = {"windows": r.windows, "seam_pairs": r.seams, "psnr": r.psnr, "arithmetic": r.arithmetic, "seed": self.seed, **two_layer,
                   "style_size": self.style_size, **masks, "psnr_full": r.psnr_full if self.style_size == "full" else None, **flow,
                   "filter_precision": self.filter_precision, **cuts, **proxy, **r.measured}
            for name, seq in r.out.items():
                if name in keep:
                    res[name] = E.stack(seq) if r.tensor_in else np.stack([E.to_host(t) for t in seq])
            res.update(flows)
            if "masks" in keep:
                res["masks"] = host(r.prop)
            if "renders" in keep:
                res["renders"] = [host(x) for x in r.renders]
        r.seconds["total"] = round(sum(r.seconds.values()), 4)
        res["seconds"] = r.seconds
        return res

    def _warp_error(self, r, finals, align_corners):
        """E_warp (warp_error.py) of the input and of the final frames with the flows this run computed, per pair and as means: over
        all pairs, over the pairs that straddle a window seam and over the others.  A pair across a scene cut has no flow and no
        E_warp: its per_pair entry is None and no mean counts it."""
        E, seams = self.engines, r.seams
        rec = {"geometry": "exact" if align_corners else "reference", "seam_pairs": list(seams), "cut_pairs": list(r.cuts_at)}
        for name, seq in (("input", r.dev_frames), ("final", finals)):
            per = []
            for t, pair in enumerate(r.full):                 # RAFT's padded size -> the frames' size, as warp_error.py resizes the .npy flows
                if pair is None:
                    per.append(None)
                    continue
                f12, f21 = pair
                per.append(E.warp_error(seq[t], seq[t + 1], E.resize_flow(f12, r.h, r.w), E.resize_flow(f21, r.h, r.w), align_corners))
            inside = [v for t, v in enumerate(per) if t not in seams and v is not None]
            across = [v for t, v in enumerate(per) if t in seams and v is not None]
            rec[name] = {"mean": float(np.mean([v for v in per if v is not None])), "per_pair": [None if v is None else float(v) for v in per],
                         "mean_seam_pairs": float(np.mean(across)) if across else None,
                         "mean_other_pairs": float(np.mean(inside)) if inside else None}
        return rec


def _schedule(config):
    from .stage1 import training_schedule
    sched = training_schedule(0, int(config["iters_num"]), int(config["evaluate_every"]))
    if not any(s[3] for s in sched):
        raise ValueError("config: iters_num %d reaches no evaluation iteration (evaluate_every %d): stage 1 would leave no frames for stage 2"
                         % (int(config["iters_num"]), int(config["evaluate_every"])))
    return sched


# ---------------------------------------------------------------------------------------------
def parse_cuts(text):
    """--cuts: none -> None, auto -> "auto", I,J,K -> [I, J, K]."""
    t = str(text).strip().lower()
    if t in ("none", "auto"):
        return None if t == "none" else "auto"
    try:
        return [int(v) for v in t.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("expected none, auto or comma-separated first-frame indices of new shots, got %r" % text)


def parse_args(argv=None):
    from .shots import add_cut_arguments
    from .y4m import LAYOUTS, add_yuv_arguments, parse_fps
    p = argparse.ArgumentParser(description="deflicker a frame folder on the MI355X: RAFT, atlas fit and neural filter in one process")
    p.add_argument("--frames_dir", type=str, default=None, help="folder of *.png / *.jpg frames (or --video)")
    p.add_argument("--video", type=str, default=None, metavar="FILE|-",
                   help="a YUV4MPEG2 stream instead of --frames_dir: a .y4m file, or - for standard input (ffmpeg -i in.mp4 -f yuv4mpegpipe -); 8-bit "
                        "progressive 444, 422, 420jpeg, 420mpeg2 or mono, converted to RGB on the device")
    p.add_argument("--video_out", type=str, default=None, metavar="FILE|-",
                   help="write the final frames as a YUV4MPEG2 stream (converted on the device) instead of final/output/%%05d.png; - is standard "
                        "output, which then carries the stream and nothing else.  Repeats the input stream's size, rate, aspect, layout and range; "
                        "with --frames_dir it needs --fps and takes --yuv_layout")
    p.add_argument("--fps", type=parse_fps, default=None, metavar="N[:D]", help="frame rate of --video_out when the input is --frames_dir")
    p.add_argument("--yuv_layout", type=str, default=None, choices=LAYOUTS, help="chroma layout of --video_out when the input is --frames_dir (default 420jpeg)")
    add_yuv_arguments(p)
    p.add_argument("--video_depth", type=str, default="8", choices=("8", "keep"),
                   help="with --video: 8 refuses a stream of more than 8 bits per sample; keep carries a 9 to 16-bit stream (C420pN, C422pN, C444pN, "
                        "CmonoN) through the run at its depth: the stages see its 8-bit reduction and the correction is carried to the deep frames as a "
                        "smooth gain / offset field.  Needs --video_out on such a stream (there is no deep PNG route); on an 8-bit stream it changes nothing")
    p.add_argument("--masks_dir", type=str, default=None,
                   help="folder of *.png / *.jpg foreground masks, one per frame in name order (255 = foreground, any size): fit a fg/bg pair of "
                        "atlases per window instead of one atlas.  The reference's convention is <frames_dir>_seg, written by its mask "
                        "preprocessors; those are external segmentation models that this package does not run")
    p.add_argument("--mask_keys_dir", type=str, default=None,
                   help="folder of *.png / *.jpg foreground masks for a few key frames only (instead of --masks_dir): with --frames_dir a mask belongs to the "
                        "frame with the same file stem, with --video the stem is the decimal frame index.  The masks of the other frames are propagated "
                        "along the optical flows on the device, inside each shot; every shot needs at least one key")
    p.add_argument("--mask_thresh", type=float, default=None,
                   help="with --mask_keys_dir: a propagated value is trusted where the forward-backward round trip of the flows closes within this many "
                        "stage-1 pixels (default 1.0, the reference's flow filter)")
    p.add_argument("--masks_only", action="store_true",
                   help="with --mask_keys_dir: stop after the propagation and write <out>/masks/%%05d.png (needs the RAFT checkpoint only): review the masks before a long run")
    p.add_argument("--out", type=str, default=None, help="results folder (default: results/<name of frames_dir>)")
    p.add_argument("--config", type=str, default=None, help="stage-1 config JSON (default: the shipped config_flow_100 values)")
    p.add_argument("--down", type=int, default=4)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--model", type=str, default="pretrained_weights/raft-things.pth", help="the RAFT checkpoint")
    p.add_argument("--ckpt_filter", type=str, default="./pretrained_weights/neural_filter.pth")
    p.add_argument("--ckpt_local", type=str, default="./pretrained_weights/local_refinement_net.pth")
    p.add_argument("--window_overlap", type=int, default=0, help="frames shared by consecutive windows of a clip longer than maximum_number_of_frames, cross-faded")
    p.add_argument("--max_long_edge", type=int, default=2000,
                   help="maximum image dimension RAFT processes without resizing: longer frames are shrunk to it (INTER_AREA, on the device) for the flow "
                        "only, as the reference's flow precompute does; every other stage keeps the full-size frames")
    p.add_argument("--proxy_long_edge", type=int, default=None,
                   help="run the whole pipeline on frames shrunk to this long edge (INTER_AREA, on the device; no effect on a clip that is not longer) and "
                        "carry each final frame to its full-size frame as a smooth gain / offset field (residual guided transfer); E_warp is then the proxy's")
    p.add_argument("--proxy_radius", type=int, default=None, help="with --proxy_long_edge: window radius of the guided transfer in proxy pixels, 1..32 (default 8)")
    p.add_argument("--proxy_eps", type=float, default=None, help="with --proxy_long_edge: regulariser of the guided transfer in squared 8-bit levels (default 64)")
    p.add_argument("--proxy_guide", type=str, default=None, choices=("channel", "colour"),
                   help="with --proxy_long_edge: the guide of the transfer: channel (every channel on its own, the default) or colour (every channel "
                        "fitted on all three, so a correction that mixes channels is carried)")
    p.add_argument("--style_size", type=str, default="stage1", choices=STYLE_SIZES,
                   help="size of the style frames stage 2 receives: stage1 (the stage-1 render, stretched to the clip's size by stage 2) or full (the "
                        "fitted nets evaluated at the clip's own pixels)")
    p.add_argument("--flow_precision", type=str, default="fp32", choices=FLOW_PRECISIONS,
                   help="arithmetic of the RAFT stage: fp32 (what the reference computes on a CPU) or fp16 (what it runs on a GPU: the encoders and the "
                        "update block under fp16 autocast)")
    p.add_argument("--filter_precision", type=str, default="fp32", choices=FILTER_PRECISIONS,
                   help="arithmetic of stage 2: fp32, or fp16 (both nets as the reference's modules compute them under fp16 autocast, on the 16-bit matrix pipe)")
    p.add_argument("--cuts", type=parse_cuts, default=None, metavar="none|auto|I,J,K",
                   help="scene cuts: none (the clip is one shot), auto (detected on the device from luminance grids; shots.py prints them without "
                        "running anything else) or the first-frame indices of the new shots.  Every shot is fitted and filtered as a clip of its own")
    add_cut_arguments(p)
    p.add_argument("--keep_intermediates", action="store_true", help="also write <frames_dir>_flow/*.npy, stage_1/output, neural_filter/output and neural_filter/concat")
    p.add_argument("--warp_error", action="store_true", help="add E_warp of the input and of the final frames to deflicker.json")
    p.add_argument("--warp_error_geometry", type=str, default="exact", choices=("exact", "reference"))
    p.add_argument("--fidelity", action="store_true", help="add the PSNR and SSIM of the final frames against the input frames to deflicker.json (taken on the device, at the clip's full size)")
    p.add_argument("--reference_dir", type=str, default=None,
                   help="with --fidelity: a folder of clean frames of the clip's size and length (a processed video's source, or the clip flicker.py flickered): "
                        "also the input and the final frames against it")
    p.add_argument("--ssim_window", type=int, default=None, help="with --fidelity: side of the uniform SSIM window, odd, 3..15 (default 7)")
    opts = p.parse_args(argv)
    if opts.video is not None and opts.frames_dir is not None:
        p.error("--video and --frames_dir are mutually exclusive: the frames come from one of them")
    if opts.video is None and opts.frames_dir is None:
        p.error("the following arguments are required: --frames_dir")
    if opts.video is not None and (opts.fps is not None or opts.yuv_layout is not None):
        p.error("--fps and --yuv_layout describe --video_out for frames from --frames_dir: with --video the output repeats the input stream's")
    if opts.video is None and opts.video_out is None and (opts.fps is not None or opts.yuv_layout is not None or opts.yuv_matrix != "auto" or opts.yuv_range != "auto"):
        p.error("--fps, --yuv_layout, --yuv_matrix and --yuv_range are options of --video / --video_out")
    if opts.video is None and opts.video_depth != "8":
        p.error("--video_depth is an option of --video")
    if opts.video is None and opts.video_out is not None and opts.fps is None:
        p.error("--video_out with --frames_dir needs --fps (a folder of frames has no frame rate)")
    if opts.mask_keys_dir is not None and opts.masks_dir is not None:
        p.error("--masks_dir and --mask_keys_dir are mutually exclusive: one mask per frame, or key masks to propagate")
    if opts.mask_keys_dir is None and (opts.mask_thresh is not None or opts.masks_only):
        p.error("--mask_thresh and --masks_only are options of --mask_keys_dir")
    if opts.proxy_long_edge is None and (opts.proxy_radius is not None or opts.proxy_eps is not None):
        p.error("--proxy_radius and --proxy_eps are options of --proxy_long_edge")
    if opts.proxy_long_edge is None and opts.proxy_guide is not None:
        p.error("--proxy_guide is an option of --proxy_long_edge")
    if not opts.fidelity and (opts.reference_dir is not None or opts.ssim_window is not None):
        p.error("--reference_dir and --ssim_window are options of --fidelity")
    if opts.fidelity and opts.masks_only:
        p.error("--fidelity compares the final frames: --masks_only leaves none")
    if opts.ssim_window is not None and not (3 <= opts.ssim_window <= 15 and opts.ssim_window % 2 == 1):
        p.error("--ssim_window must be odd and in 3..15")
    if opts.proxy_long_edge is not None and opts.proxy_long_edge < 1:
        p.error("--proxy_long_edge must be positive")
    if opts.out is None:
        if opts.video is not None:
            name = "stdin" if opts.video == "-" else os.path.splitext(os.path.basename(opts.video))[0]
        else:
            name = os.path.basename(os.path.normpath(opts.frames_dir))
        opts.out = os.path.join("results", name)
    return opts


def list_masks(masks_dir, n_frames):
    """The first n_frames of *.jpg and *.png under masks_dir, sorted together by name: what load_input_data_device reads from <vid>_seg."""
    from pathlib import Path
    d = Path(masks_dir)
    files = sorted(list(d.glob("*.jpg")) + list(d.glob("*.png")))
    if len(files) < n_frames:
        raise SystemExit("%d masks (*.jpg / *.png) under %s for %d frames: the two-layer path needs one mask per frame (--masks_dir)"
                         % (len(files), masks_dir, n_frames))
    return files[:n_frames]


def list_mask_keys(keys_dir, frame_files=None):
    """{frame index: path} of the *.jpg / *.png key masks under keys_dir (--mask_keys_dir).  With the frames' files a mask belongs to the
    frame with the same file stem; without (a video stream) its stem is the decimal frame index.  A stem that matches no frame, two masks
    for one frame and an empty folder are a SystemExit naming the file."""
    from .warp_error import list_frames
    files = list_frames(keys_dir)
    if not files:
        raise SystemExit("no key masks (*.jpg / *.png) under %s (--mask_keys_dir)" % keys_dir)
    stems = {f.stem: i for i, f in enumerate(frame_files)} if frame_files is not None else None
    out = {}
    for f in files:
        if stems is not None:
            if f.stem not in stems:
                raise SystemExit("%s: no frame is named %s.png or %s.jpg (--mask_keys_dir matches a key mask to the frame with its file stem)" % (f, f.stem, f.stem))
            i = stems[f.stem]
        else:
            if not f.stem.isdigit():
                raise SystemExit("%s: with --video the stem of a key mask is the decimal frame index, got %r" % (f, f.stem))
            i = int(f.stem)
        if i in out:
            raise SystemExit("%s and %s are both key masks of frame %d" % (out[i], f, i))
        out[i] = f
    return out


def decode_mask(path):
    """A mask file as the stage-1 CLI decodes it (stage1.decode_u8(path, 1)): (Hm, Wm, 1) uint8, channel 0."""
    from .stage1 import decode_u8
    try:
        return decode_u8(path, 1)
    except ValueError:
        raise SystemExit("%s: only 8-bit masks are handled" % path)


def load_checkpoints(opts):
    """(raft, filter, local) state dicts; a missing file is a SystemExit naming it and its flag.  --masks_only runs RAFT alone: the
    other two are None and their files are not looked for."""
    import torch
    sds = []
    for path, flag in ((opts.model, "--model"), (opts.ckpt_filter, "--ckpt_filter"), (opts.ckpt_local, "--ckpt_local")):
        if getattr(opts, "masks_only", False) and flag != "--model":
            sds.append(None)
            continue
        if not os.path.exists(path):
            raise SystemExit("checkpoint %s not found (%s)" % (path, flag))
        sds.append(torch.load(path, map_location="cpu"))
    return sds


def video_frames(engines, reader, matrix, full_range, count=None):
    """The frame iterator `run` gets for --video: every payload of the stream uploaded as it is and converted on the device
    (engines.upload, engines.yuv_to_rgb; engines.yuv_to_rgb16 for a reader of more than 8 bits per sample).  `count`: a one-element list
    that ends up holding the number of frames read."""
    bits = getattr(reader, "bits", 8)
    for payload in reader:
        if count is not None:
            count[0] += 1
        if bits > 8:
            yield engines.yuv_to_rgb16(engines.upload(payload), reader.height, reader.width, reader.layout, matrix, full_range, bits)
            continue
        yield engines.yuv_to_rgb(engines.upload(payload), reader.height, reader.width, reader.layout, matrix, full_range)


class VideoSink:
    """The CLI's sink for --video_out: `final` frames arrive as device tensors in frame order, are converted on the device
    (engines.rgb_to_yuv), copied to the host and written; the stream's header is written with the first frame, whose size it takes.
    Everything else goes to `other` (the PNG encoders) as a host array.  bits above 8: `final` frames are uint16 tensors, converted by
    engines.rgb16_to_yuv and written at that depth."""

    def __init__(self, engines, target, fps, layout, matrix, full_range, aspect=None, other=None, interlace="p", bits=8):
        self.bits = int(bits)
        self.E, self.target, self.fps, self.layout, self.matrix, self.full_range, self.aspect, self.other = engines, target, fps, layout, matrix, full_range, aspect, other
        self.interlace = interlace
        self.writer, self.resolved = None, None

    def __call__(self, name, i, t):
        from .y4m import Y4MWriter, resolve_matrix
        if name != "final":
            if self.other is not None:
                self.other(name, i, self.E.to_host(t))
            return
        h, w = int(t.shape[0]), int(t.shape[1])
        if self.writer is None:
            self.resolved = resolve_matrix(self.matrix, h, w)
            self.writer = Y4MWriter(self.target, w, h, self.fps, self.layout, self.full_range, aspect=self.aspect, interlace=self.interlace,
                                    **({"bits": self.bits} if self.bits > 8 else {}))
        if self.bits > 8:
            self.writer.write(self.E.to_host(self.E.rgb16_to_yuv(t, self.layout, self.resolved, self.full_range, self.bits)))
            return
        self.writer.write(self.E.to_host(self.E.rgb_to_yuv(t, self.layout, self.resolved, self.full_range)))

    def close(self):
        if self.writer is not None:
            self.writer.close()


def main(argv=None, engines=None):
    """engines: a replacement for DeviceEngines (the host tests' stubs); then neither a GPU nor the checkpoints are looked for."""
    opts = parse_args(argv)
    to_stdout = opts.video_out == "-"
    stream_out = sys.stdout.buffer if to_stdout else opts.video_out      # taken before standard output is handed to the messages' stream
    stdout = sys.stdout
    if to_stdout:
        sys.stdout = sys.stderr                               # standard output carries the stream and nothing else
    try:
        return _main(opts, engines, stream_out)
    finally:
        sys.stdout = stdout


def _open_input(opts):
    """-> (reader, files, source): the YUV4MPEG2 reader of --video or the frame files of --frames_dir (the other is None), and the
    input's name for messages."""
    from .warp_error import list_frames
    from .y4m import Y4MError, Y4MReader
    if opts.video is None:
        files = list_frames(opts.frames_dir)
        if len(files) < 2:
            raise SystemExit("%d frames (*.jpg / *.png) under %s: a clip needs at least 2" % (len(files), opts.frames_dir))
        return None, files, opts.frames_dir
    source = "standard input" if opts.video == "-" else opts.video
    if opts.video != "-" and not os.path.exists(opts.video):
        raise SystemExit("video %s not found (--video)" % opts.video)
    keep = getattr(opts, "video_depth", "8") == "keep"
    try:
        reader = Y4MReader(opts.video, **({"deep": True} if keep else {}))
    except Y4MError as e:
        raise SystemExit("%s: %s" % (source, e))
    if reader.bits > 8 and opts.video_out is None:           # before any work: the final frames would have nowhere to go
        reader.close()
        raise SystemExit("%s: --video_depth keep on a stream of %d bits per sample needs --video_out: the final frames are written as a stream of "
                         "that depth, there is no deep PNG route" % (source, reader.bits))
    return reader, None, source


def _side_inputs(opts, files):
    """-> (mask_files, key_files, ref_files, config): what the flags name beside the frames, each None without its flag."""
    from .warp_error import list_frames
    mask_files = None
    if opts.masks_dir is not None:                            # a stream's length is not known yet: every mask there is, counted against the frames by run
        mask_files = list_masks(opts.masks_dir, len(files)) if files is not None else list_frames(opts.masks_dir)
    key_files = list_mask_keys(opts.mask_keys_dir, files) if opts.mask_keys_dir is not None else None
    ref_files = None
    if getattr(opts, "reference_dir", None) is not None:      # with --video too the reference is a folder of frames
        ref_files = list_frames(opts.reference_dir) if os.path.isdir(opts.reference_dir) else []
        if not ref_files:
            raise SystemExit("no reference frames (*.jpg / *.png) under %s (--reference_dir)" % opts.reference_dir)
        if files is not None and len(ref_files) != len(files):
            raise SystemExit("%d reference frames under %s for %d frames (--reference_dir)" % (len(ref_files), opts.reference_dir, len(files)))
    config = None
    if opts.config is not None:
        if not os.path.exists(opts.config):
            raise SystemExit("config %s not found (--config)" % opts.config)
        with open(opts.config) as f:
            config = json.load(f)
    return mask_files, key_files, ref_files, config


def _configure(opts, engines, config, files):
    """The Deflicker the flags describe; what it refuses is a SystemExit."""
    raft_sd, filter_sd, local_sd = load_checkpoints(opts) if engines is None else (None, None, None)
    knobs = {k: getattr(opts, k, None) for k in ("mask_thresh", "proxy_long_edge", "proxy_radius", "proxy_eps", "proxy_guide")}
    try:
        d = Deflicker(raft_sd, filter_sd, local_sd, config=config, down=opts.down, seed=opts.seed, window_overlap=opts.window_overlap, device=opts.gpu,
                      max_long_edge=opts.max_long_edge, style_size=opts.style_size, flow_precision=opts.flow_precision,
                      filter_precision=opts.filter_precision, cuts=opts.cuts, cut_threshold=opts.cut_threshold, cut_margin=opts.cut_margin,
                      cut_radius=opts.cut_radius, min_shot_frames=opts.min_shot_frames, engines=engines, **knobs)
        if isinstance(d.cuts, list) and d.cuts and files is not None:
            from .shots import plan_shots
            plan_shots(len(files), d.cuts)                    # before a frame is decoded
    except ValueError as e:
        raise SystemExit(str(e))
    return d


def _yuv_side(opts, reader):
    """The YCbCr side (y4m.py) -> (video, fps, layout, full_range): the fields of the record, and what the sink and the reader's
    conversion take (None without --video / --video_out).  The matrix is policy or the flag, the range the flag or the input's
    header; the output repeats the input's."""
    from .y4m import resolve_matrix, resolve_range
    video = {"video": opts.video, "video_out": opts.video_out, "fps": None, "yuv_layout": None, "yuv_matrix": None, "yuv_range": None}
    if reader is None and opts.video_out is None:
        return video, None, None, None
    full_range = resolve_range(opts.yuv_range, reader.full_range if reader is not None else False)
    fps = reader.fps if reader is not None else opts.fps
    layout = reader.layout if reader is not None else (opts.yuv_layout or "420jpeg")
    video.update(fps=[fps.numerator, fps.denominator], yuv_layout=layout, yuv_range="full" if full_range else "limited")
    if reader is not None:
        video["yuv_matrix"] = resolve_matrix(opts.yuv_matrix, reader.height, reader.width)
    return video, fps, layout, full_range


def _plan_outputs(opts, out, with_keys):
    """-> (dirs, keep): the folder of every sequence that is written as PNGs, made here, and what `run` is asked to keep."""
    dirs = {} if opts.video_out is not None or opts.masks_only else {"final": out / "final" / "output"}
    keep = ["final"]
    if opts.keep_intermediates:
        if not opts.masks_only:
            dirs.update(stage1=out / "stage_1" / "output", filtered=out / "neural_filter" / "output", concat=out / "neural_filter" / "concat")
        keep += ["stage1", "filtered", "concat", "flows"]
    if with_keys and (opts.keep_intermediates or opts.masks_only):      # the propagated planes, written after the run
        dirs["masks"] = out / "masks"
        keep += ["masks"]
    out.mkdir(parents=True, exist_ok=True)
    for p in dirs.values():
        p.mkdir(parents=True, exist_ok=True)
    return dirs, keep


def _decode(path):
    from .neural_filter import read_png
    img = read_png(str(path))
    if img.dtype != np.uint8:
        raise SystemExit("%s: only 8-bit images are handled" % path)
    return img


def _run_with_sinks(d, opts, reader, files, source, side, yuv, keep, sink, stream_out):
    """`d.run` on the input, with the sinks -> (res, number of frames); the video sink and the reader are closed whatever happens."""
    from .stage1 import _prefetch
    from .warp_error import parse_geometry
    mask_files, key_files, ref_files = side
    video, fps, layout, full_range = yuv
    count, vsink = [0], None
    if opts.video_out is not None:
        vsink = VideoSink(d.engines, stream_out, fps, layout, video["yuv_matrix"] or opts.yuv_matrix, full_range,
                          aspect=reader.aspect if reader is not None else None, other=sink,
                          interlace=reader.interlace if reader is not None else "p",
                          **({"bits": reader.bits} if reader is not None and reader.bits > 8 else {}))
    try:
        frames = video_frames(d.engines, reader, video["yuv_matrix"], full_range, count) if reader is not None else _prefetch(_decode, files)
        routes = dict(sink_device=vsink is not None, masks_only=bool(opts.masks_only),      # a route that is off passes run's own default
                      mask_keys=None if key_files is None else {i: decode_mask(p) for i, p in key_files.items()},
                      fidelity=(True if opts.ssim_window is None else opts.ssim_window) if getattr(opts, "fidelity", False) else None,
                      reference=None if ref_files is None else [_decode(f) for f in ref_files],
                      **({"bits": reader.bits} if reader is not None and reader.bits > 8 else {}))
        res = d.run(frames, masks=_prefetch(decode_mask, mask_files) if mask_files is not None else None, keep=keep,
                    sink=vsink if vsink is not None else sink, warp_error=parse_geometry(opts.warp_error_geometry) if opts.warp_error else None, **routes)
    except ValueError as e:                                   # Y4MError is one: a truncated stream ends the run with its named error
        raise SystemExit("%s: %s" % (source, e))
    finally:
        if vsink is not None:
            vsink.close()
        if reader is not None:
            reader.close()
    if vsink is not None:
        video["yuv_matrix"] = vsink.resolved
    return res, (len(files) if files is not None else count[0])


def _dump_flows(opts, out, files, n_frames, flows, submit):
    """--keep_intermediates: the flows as the flow CLI names them, <a>_<b>.npy and <b>_<a>.npy per pair."""
    from pathlib import Path
    flow_dir = Path(os.path.normpath(opts.frames_dir) + "_flow") if files is not None else out / "flow"
    flow_dir.mkdir(exist_ok=True)
    names = [f.name for f in files] if files is not None else ["%05d.png" % i for i in range(n_frames)]
    for i, pair in enumerate(flows):
        if pair is None:                                      # a pair across a scene cut has no flow
            continue
        (f12, f21), a, b = pair, names[i], names[i + 1]
        submit(np.save, flow_dir / ("%s_%s.npy" % (a, b)), f12.cpu().numpy())
        submit(np.save, flow_dir / ("%s_%s.npy" % (b, a)), f21.cpu().numpy())


# deflicker.json: what `run` returned and what _main adds, in the file's order; a key a route did not produce is left out
_RECORD = ("windows", "seam_pairs", "psnr", "seconds", "arithmetic", "seed", "two_layer", "flow_size", "max_long_edge", "style_size", "psnr_full",
          "flow_precision", "filter_precision", "shots", "cut_pairs", "cuts", "cut_scores", "mask_keys", "mask_thresh", "proxy", "depth",
          "cut_threshold", "cut_margin", "cut_radius", "min_shot_frames", "masks_dir", "mask_keys_dir", "masks_only", "frames", "window_overlap",
          "video", "video_out", "fps", "yuv_layout", "yuv_matrix", "yuv_range", "warp_error", "fidelity", "reference_dir")


def _write_record(path, d, opts, res, video, n_frames):
    own = dict(video, cut_threshold=d.cut_threshold, cut_margin=d.cut_margin, cut_radius=d.cut_radius, min_shot_frames=d.min_shot_frames,
               masks_dir=opts.masks_dir, mask_keys_dir=opts.mask_keys_dir, masks_only=bool(opts.masks_only), frames=n_frames,
               window_overlap=opts.window_overlap, **({"reference_dir": opts.reference_dir} if "fidelity" in res else {}))
    fields = {**res, **own}
    with open(path, "w") as f:
        json.dump({k: fields[k] for k in _RECORD if k in fields}, f, indent=2)


def _main(opts, engines, stream_out):
    from concurrent.futures import ThreadPoolExecutor
    from pathlib import Path
    from PIL import Image
    if engines is None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("No GPU found: the pipeline has no CPU path")
    reader, files, source = _open_input(opts)
    mask_files, key_files, ref_files, config = _side_inputs(opts, files)
    d = _configure(opts, engines, config, files)
    yuv = _yuv_side(opts, reader)
    out = Path(opts.out)
    dirs, keep = _plan_outputs(opts, out, key_files is not None)
    with ThreadPoolExecutor(max_workers=8) as pool:           # PNG encodes (zlib drops the GIL) run behind the device work
        jobs = []

        def submit(*job):
            jobs.append(pool.submit(*job))

        def sink(name, i, arr):
            submit(lambda: Image.fromarray(arr).save(str(dirs[name] / ("%05d.png" % i))))
        res, n_frames = _run_with_sinks(d, opts, reader, files, source, (mask_files, key_files, ref_files), yuv, keep, sink, stream_out)
        if opts.keep_intermediates:
            _dump_flows(opts, out, files, n_frames, res["flows"], submit)
        if "masks" in dirs:                                   # the propagated planes as 8-bit PNGs: trunc(m * 255 + 0.5), in fp64
            for i, m in enumerate(res["masks"]):
                sink("masks", i, (np.asarray(m, np.float64) * 255.0 + 0.5).astype(np.uint8))
        for j in jobs:
            j.result()
    _write_record(out / "deflicker.json", d, opts, res, yuv[0], n_frames)
    if opts.masks_only:
        print("wrote the masks of %d frames (keys %s) to %s; seconds %s" % (n_frames, res["mask_keys"], dirs["masks"], res["seconds"]))
        return 0
    where = dirs["final"] if "final" in dirs else ("standard output" if opts.video_out == "-" else opts.video_out)
    print("wrote %d frames to %s; PSNR per window %s; seconds %s" % (n_frames, where, ["%.2f" % p for p in res["psnr"]], res["seconds"]))
    return 0


if __name__ == "__main__":
    if __package__ in (None, ""):
        sys.path.insert(0, os.path.dirname(_HERE))
        import aiod_amd  # noqa: F401
        from aiod_amd import deflicker as _d
        sys.exit(_d.main())
    sys.exit(main())
