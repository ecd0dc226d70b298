#!/usr/bin/env python
"""The pin `af_resize_area` still lacks: vectors written by the REAL OpenCV for the one call of RAFTWrapper.load_image
(src/models/stage_1/raft_wrapper.py:44), `cv2.resize(img, (new_w, new_h), interpolation=cv2.INTER_AREA)` on uint8 frames.  No image of
this project carries cv2, so the kernel is held against a restatement of OpenCV 4.x's resize.cpp (tests/resize_area_ref.py) and an
exact area average only ("parity with OpenCV unpinned").  Run this script ONCE on any machine with opencv-python 4.x:

    python tools/make_golden_resize_area.py            # writes tests/golden/resize_area_cv2.npz (inputs AND cv2's outputs, ~0.3 MB)

From then on tests/test_resize_area_cv2.py holds, without cv2, the restatement (CPU) and the kernel (GPU) against what OpenCV itself
computed, bit for bit.  The cases are the shapes of tests/test_gpu_resize_area.py: a clipped last cell, a scale barely above 1, the
reference's own quirk sizes, an integer scale on one axis only, and the three integer-scale paths (2x2 with 1, 2, 3 and 4 channels: the
SIMD average against the float product), each on a random image, an all-0 and an all-255 image.  The distance between cv2 and the
restatement at generation time is RECORDED per case, not assumed to be zero."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "resize_area_cv2.npz")


def cases():
    """name -> (image, dh, dw)."""
    import resize_area_ref as R
    c = {}
    todo = [(s, 3) for s in R.SHAPES] + [((20, 30, 10, 15), 1), ((20, 30, 10, 15), 2), ((20, 30, 10, 15), 4), ((17, 23, 8, 11), 1)]
    for (sh, sw, dh, dw), ch in todo:
        for kind, img in zip(("random", "zeros", "full"), R.inputs(sh, sw, ch)):
            c["%dx%d_to_%dx%d_c%d_%s" % (sh, sw, dh, dw, ch, kind)] = (img, dh, dw)
    return c


def main():
    import cv2
    import resize_area_ref as R
    out, names = {}, []
    for name, (img, dh, dw) in cases().items():
        src = img if img.shape[2] > 1 else img[:, :, 0]
        got = cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA).reshape(dh, dw, img.shape[2])
        assert got.dtype == np.uint8
        dist = int(np.abs(got.astype(np.int64) - R.resize_area(img, dh, dw).astype(np.int64)).max())
        names.append(name)
        out[name + ".in"], out[name + ".size"], out[name + ".out"], out[name + ".dist_at_generation"] = img, np.array([dh, dw]), got, np.array(dist)
        print("%-36s cv2 vs restatement: max |diff| = %d" % (name, dist))
    out["names"] = np.array(names)
    out["cv2_version"] = np.array(cv2.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d cases, cv2 %s, %d bytes)" % (OUT, len(names), cv2.__version__, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
