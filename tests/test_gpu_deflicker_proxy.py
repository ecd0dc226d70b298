"""The proxy route of the one-process pipeline on the GPU (Deflicker(proxy_long_edge=...)), on the synthetic assets and
the short schedule of tests/test_gpu_deflicker.py.

The comparisons are exact and the tolerance is derived: the proxy route shrinks the frames with the kernel aiod_amd.resize_area runs,
runs the code a plain run of the shrunk frames runs (same kernels, same values, same seed, fixed-order reductions) and carries the result
up with the kernels aiod_amd.guided_transfer runs."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as PB  # noqa: E402

H, W, DOWN, SEED, N = 130, 197, 4, 11, 3
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


def test_proxy_route_is_the_plain_run_of_the_shrunk_frames_carried_up():
    import aiod_amd
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    from aiod_amd.preprocess_optical_flow import shrink_size
    weights = PB.synthetic_weights()
    cfg = dict(REFERENCE_CONFIG, **SHORT)
    frames = PB.synthetic_clip(N, H, W, seed=5)
    edge, radius = 195, 5                                     # just below the long edge: RAFT needs a padded frame of at least 128 x 128
    h, w = shrink_size(H, W, edge)
    assert (h, w) != (H, W) and max(h, w) <= edge and min(h, w) >= 128

    def run(clip, **kw):
        return aiod_amd.Deflicker(*weights, config=cfg, down=DOWN, seed=SEED, **kw).run(clip)

    res = run(frames, proxy_long_edge=edge, proxy_radius=radius)
    assert res["final"].shape == (N, H, W, 3) and res["final"].dtype == np.uint8
    assert res["proxy"] == {"size": [h, w], "radius": radius, "eps": aiod_amd.DEFAULT_EPS} and res["flow_size"] == [h, w]
    assert {"proxy", "transfer"} <= set(res["seconds"])
    small = [aiod_amd.resize_area(f, h, w) for f in frames]
    plain = run(small)
    assert plain["final"].shape == (N, h, w, 3) and "proxy" not in plain
    for i in range(N):
        expect = aiod_amd.guided_transfer(frames[i], small[i], plain["final"][i], radius=radius, eps=aiod_amd.DEFAULT_EPS)
        assert np.array_equal(res["final"][i], expect), (i, int((res["final"][i] != expect).sum()))
    assert any(not np.array_equal(res["final"][i], frames[i]) for i in range(N))      # the run did change the frames
    # at or above the long edge the flag does nothing: the default run's bytes, keys and laps
    default, same = run(frames), run(frames, proxy_long_edge=max(H, W))
    assert np.array_equal(default["final"], same["final"]) and "proxy" not in same
    assert set(default) == set(same) and set(default["seconds"]) == set(same["seconds"])
