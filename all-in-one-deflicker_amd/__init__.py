"""MI355X-native (gfx950) implementation of the stage-1 neural-atlas optimisation loop of
All-In-One-Deflicker (reference: src/stage1_neural_atlas.py).  The compute path is libatlasfit.so
(hand-written HIP, C ABI in include/atlasfit.h); this package is the thin host-side mirror of the
reference's Python interface for that path.  There is NO CPU fallback: without the HIP library and a
GPU every compute entry point raises."""
from .atlasfit import AtlasFit, AtlasFitError, EditSession, warp_error_pair, resize_area, resize_area_device, AfConfig, default_config, load_library, NET_MAPPING1, NET_ATLAS, NET_MAPPING2, NET_ALPHA  # noqa: F401
from .stage2 import NeuralFilter, StateDictError  # noqa: F401,E402
from .raft import RAFT  # noqa: F401,E402
from .deflicker import Deflicker, plan_windows  # noqa: F401,E402
from .shots import luma_grids, cut_scores, detect_cuts, plan_shots  # noqa: F401,E402
from .masks import plan_mask_propagation, propagate_masks, propagate_masks_device  # noqa: F401,E402
from .guided import guided_transfer, guided_transfer_device, guided_coeffs, guided_coeffs_device, guided_apply, guided_apply_device, DEFAULT_EPS, DEFAULT_RADIUS, reduce_depth, reduce_depth_device, guided_apply16, guided_apply16_device, depth_transfer, depth_transfer_device, guided_coeffs_colour, guided_coeffs_colour_device, guided_transfer_colour, guided_transfer_colour_device, depth_transfer_colour, depth_transfer_colour_device, guided_apply_colour, guided_apply_colour_device, guided_apply_colour16, guided_apply_colour16_device  # noqa: F401,E402
from .y4m import Y4MReader, Y4MWriter, Y4MError, yuv_to_rgb, rgb_to_yuv, yuv_to_rgb_device, rgb_to_yuv_device, resolve_matrix, yuv_to_rgb16, rgb16_to_yuv, yuv_to_rgb16_device, rgb16_to_yuv_device  # noqa: F401,E402
from .fidelity import frame_fidelity, frame_fidelity_device, psnr_from_sse, summarise, DEFAULT_WINDOW  # noqa: F401,E402
from .flicker import synth_flicker  # noqa: F401,E402
