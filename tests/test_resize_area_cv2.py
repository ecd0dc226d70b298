"""Consumes tests/golden/resize_area_cv2.npz — outputs of the REAL OpenCV for `cv2.resize(img, (dw, dh), interpolation=cv2.INTER_AREA)`
on uint8 images, written by tools/make_golden_resize_area.py on a machine that has cv2 (no image of this project does: until someone
runs it these tests skip and parity of af_resize_area with OpenCV's own bytes stays unpinned).  With the fixture, the restatement
(tests/resize_area_ref.py) and - on the GPU - k_resize_area are held against what OpenCV itself computed, bit for bit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FIX = os.path.join(HERE, "golden", "resize_area_cv2.npz")
pytestmark = pytest.mark.skipif(not os.path.exists(FIX), reason="tests/golden/resize_area_cv2.npz not generated yet (needs a machine with cv2: python tools/make_golden_resize_area.py)")


def _cases():
    g = np.load(FIX)
    for name in [str(n) for n in g["names"]]:
        dh, dw = (int(v) for v in g[name + ".size"])
        yield name, g[name + ".in"], dh, dw, g[name + ".out"]


def test_restatement_equals_opencv():
    import resize_area_ref as R
    for name, img, dh, dw, out in _cases():
        assert np.array_equal(R.resize_area(img, dh, dw), out), name


@pytest.mark.gpu
def test_kernel_equals_opencv():
    import aiod_amd
    for name, img, dh, dw, out in _cases():
        assert np.array_equal(aiod_amd.resize_area(img, dh, dw), out), name
