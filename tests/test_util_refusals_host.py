"""The handle-free utilities of libatlasfit.so without a GPU (include/atlasfit.h: af_resize_bilinear, af_resize_area, af_luma_grid,
af_yuv_to_rgb, af_rgb_to_yuv, af_yuv_frame_bytes, af_mask_step, af_mask_blend, af_flow_consistency, af_warp_error_pair).

One table of refusals: every row is a valid call of an entry with exactly one condition broken; the status is AF_EINVAL and the text
of af_last_error(NULL) is compared with ==.  All of these refusals come before the device is selected, so they need none.  Without a
device a valid call of every entry fails in hipSetDevice (AF_EHIP): nothing is computed on the host."""
import ctypes as C

import numpy as np
import pytest

AF_EINVAL, AF_EHIP = -1, -2
H, W = 5, 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import aiod_amd
    return aiod_amd.load_library()


def _plane(*tail, dtype=np.float32):
    return np.zeros((H, W) + tail, dtype)


def _valid():
    """{entry: ordered {argument: value}} of a valid call on host buffers, without the device ordinal and on_device."""
    yuv = np.zeros(H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2), np.uint8)      # 420jpeg payload of a 5 x 7 picture: 59 bytes
    return {
        "af_resize_bilinear": dict(src=_plane(3, dtype=np.uint8), src_u8=1, sh=H, sw=W, ch=3, dst=np.zeros((3, 4, 3), np.float32), dh=3, dw=4,
                                   pix_stride=3, ch_stride=1, offset=0, scale0=1.0, scale1=1.0),
        "af_resize_area": dict(src=_plane(3, dtype=np.uint8), sh=H, sw=W, ch=3, dst=np.zeros((3, 4, 3), np.uint8), dh=3, dw=4),
        "af_luma_grid": dict(src=np.zeros((2, H, W, 3), np.uint8), n=2, h=H, w=W, gh=2, gw=3, sums_out=np.zeros((2, 2, 3), np.uint64)),
        "af_yuv_to_rgb": dict(src=yuv, h=H, w=W, layout=2, matrix=1, full_range=0, dst=_plane(3, dtype=np.uint8)),
        "af_rgb_to_yuv": dict(src=_plane(3, dtype=np.uint8), h=H, w=W, layout=2, matrix=1, full_range=0, dst=yuv.copy()),
        "af_mask_step": dict(m_s=_plane(), c_s=_plane(), f_ts=_plane(2), f_st=_plane(2), h=H, w=W, thresh=1.0, m_t=_plane(), c_t=_plane()),
        "af_mask_blend": dict(m_f=_plane(), c_f=_plane(), m_b=_plane(), c_b=_plane(), h=H, w=W, a=0, t=1, b=2, out=_plane()),
        "af_flow_consistency": dict(f12=_plane(2), f21=_plane(2), h=H, w=W, out=_plane(), pix_stride=1, offset=0, thresh=1.0),
        "af_warp_error_pair": dict(img1=_plane(3), img2=_plane(3), flow12=_plane(2), flow21=_plane(2), h=H, w=W, align_corners=1,
                                   err=C.c_double(-1.0), noc=None, warped=None),
    }


class Same:
    """The value of another argument of the same call (an aliased buffer)."""

    def __init__(self, name):
        self.name = name


# (entry, {argument: broken value}, message after "<entry>: ")
REFUSALS = [
    ("af_resize_bilinear", dict(src=None), "arguments"),
    ("af_resize_bilinear", dict(dh=0), "arguments"),
    ("af_resize_area", dict(ch=5), "ch must be 1..4"),
    ("af_luma_grid", dict(src=None), "null pointer"),
    ("af_luma_grid", dict(n=0), "n < 1"),
    ("af_luma_grid", dict(gh=65), "gh must be 1..64"),
    ("af_luma_grid", dict(gw=0), "gw must be 1..64"),
    ("af_yuv_to_rgb", dict(src=None), "null pointer"),
    ("af_yuv_to_rgb", dict(h=0), "h must be 1..16384"),
    ("af_yuv_to_rgb", dict(w=16385), "w must be 1..16384"),
    ("af_yuv_to_rgb", dict(layout=99), "unknown layout"),
    ("af_rgb_to_yuv", dict(matrix=99), "unknown matrix"),
    ("af_mask_step", dict(m_s=None), "null pointer"),
    ("af_mask_step", dict(h=0), "h must be 1..16384"),
    ("af_mask_step", dict(thresh=0.0), "thresh must be finite and > 0"),
    ("af_mask_step", dict(thresh=float("nan")), "thresh must be finite and > 0"),
    ("af_mask_step", dict(m_t=Same("m_s")), "an output aliases an input"),
    ("af_mask_step", dict(m_t=Same("c_t")), "m_t aliases c_t"),
    ("af_mask_blend", dict(c_b=None), "null pointer"),
    ("af_mask_blend", dict(w=0), "w must be 1..16384"),
    ("af_mask_blend", dict(a=0, t=2, b=2), "frames must satisfy a < t < b"),
    ("af_mask_blend", dict(out=Same("m_b")), "the output aliases an input"),
    ("af_flow_consistency", dict(h=0), "arguments"),
    ("af_warp_error_pair", dict(h=1), "arguments"),
    ("af_warp_error_pair", dict(align_corners=2), "arguments"),
    ("af_warp_error_pair", dict(h=32768, w=32768), "image too large"),
]


def _call(lib, entry, args):
    def conv(v):
        if isinstance(v, Same):
            v = args[v.name]
        if isinstance(v, np.ndarray):
            return v.ctypes.data_as(C.c_void_p)
        return C.byref(v) if isinstance(v, C.c_double) else v
    rc = getattr(lib, entry)(0, *[conv(v) for v in args.values()], 0)
    return rc, lib.af_last_error(None).decode()


def _row_id(row):
    return "%s-%s" % (row[0], ",".join("%s=%s" % (k, v.name if isinstance(v, Same) else v) for k, v in row[1].items()))


@pytest.mark.parametrize("row", REFUSALS, ids=_row_id)
def test_refusal(lib, row):
    entry, broken, msg = row
    args = _valid()[entry]
    assert set(broken) <= set(args)
    args.update(broken)
    assert _call(lib, entry, args) == (AF_EINVAL, "%s: %s" % (entry, msg))


def test_yuv_frame_bytes(lib):
    assert [lib.af_yuv_frame_bytes(5, 7, layout) for layout in range(-1, 7)] == [0, 105, 75, 59, 59, 35, 0, 0]
    assert lib.af_yuv_frame_bytes(0, 7, 0) == 0


@pytest.mark.parametrize("entry", sorted(_valid()))
def test_a_valid_call_needs_the_device(lib, entry):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc, text = _call(lib, entry, _valid()[entry])
    assert rc == AF_EHIP and text.startswith("hipSetDevice: "), (rc, text)
