"""The fidelity metrics on the GPU (include/atlasfit.h af_fidelity, csrc/fidelity.hip) against the numpy restatement
tests/fidelity_ref.py, the flicker synthesiser against its restatement, and `Deflicker.run(fidelity=...)` on the synthetic assets and the
short schedule of tests/test_gpu_deflicker_proxy.py.

Exactness: the SSIM map equals the restatement bit for bit and the SSE equals numpy's int64 sum.  The per-frame SSIM is the device's
fixed-order fp64 sum of the map divided by the window count; against math.fsum(map) / count it may differ by the error of a summation of
`count` terms of magnitude at most 1, at most count * 2^-53 after the division (any order of summation stays inside the sequential
bound (count - 1) u sum|x| with u = 2^-53), so the tolerance is derived, not chosen.

The shapes are the smallest at which the kernel can go wrong; the tile constants come from the kernel's own header."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fidelity_ref as R  # noqa: E402

TX, TY, SSE_BYTES = R.tile()
WINS = (3, 7, 15)


def _shapes(win):
    """(h, w) around every edge of the kernel's tile for this window."""
    out = [(win, win), (win, win + 1), (win + 1, win)]
    out += [(TY + win - 1 + dy, TX + win - 1 + dx) for dy, dx in ((-1, -1), (0, 0), (1, 1), (-1, 1), (1, -1))]      # one below, at, one above the tile edge
    out += [(37, 53), (130, 197)]                             # odd widths; 130 x 197 x 3 bytes span several workgroups of the SSE kernel too
    out += [(TY + win - 1, 4 * ((TX + win + 2) // 4)), (40, 64)]      # widths that are multiples of 4: the dword path
    return out


CASES = [(win, h, w) for win in WINS for h, w in _shapes(win)]


@lru_cache(maxsize=None)
def _pair(h, w, n=1):
    frames = [R.make_pair(h, w, 1000 * h + w + 7 * k, "structured" if k % 2 == 0 else "random") for k in range(n)]
    a, b = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@lru_cache(maxsize=None)
def _expected(h, w, win, n=1):
    """(sse uint64 (n, 3), map float64 (n, oh, ow, 3), fsum means (n, 3)) of _pair(h, w, n): computed once, shared, read-only."""
    a, b = _pair(h, w, n)
    maps = np.stack([R.ssim_map(a[k], b[k], win) for k in range(n)])
    means = np.stack([R.ssim_mean(m) for m in maps])
    sse = R.sse(a, b)
    for arr in (maps, means, sse):
        arr.setflags(write=False)
    return sse, maps, means


def _call(a, b, win, route, misalign=False, **kw):
    """frame_fidelity through host pointers, or through device pointers (optionally one byte off a 4-byte boundary); numpy results."""
    import torch
    import aiod_amd
    if route == "host":
        return aiod_amd.frame_fidelity(a, b, win, **kw)
    def dev(x):
        if not misalign:
            return torch.from_numpy(np.array(x)).cuda()      # a writable copy: the shared inputs are read-only
        buf = torch.empty(x.size + 1, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        view = buf[1:].view(x.shape)
        view.copy_(torch.from_numpy(np.array(x)))
        assert view.data_ptr() % 4 == 1 and view.is_contiguous()
        return view
    r = aiod_amd.frame_fidelity_device(dev(a), dev(b), win, **kw)
    if "map" in r:
        r["map"] = r["map"].cpu().numpy()
    return r


def _check(r, h, w, win, n=1, want_map=True):
    sse, maps, means = _expected(h, w, win, n)
    count = (h - win + 1) * (w - win + 1)
    assert r["sse"].dtype == np.uint64 and r["sse"].shape == (n, 3) and np.array_equal(r["sse"], sse)
    if want_map:
        assert r["map"].shape == maps.shape and r["map"].dtype == np.float64
        assert np.array_equal(r["map"].view(np.uint64), maps.view(np.uint64)), "%d of %d windows differ, max %.3e" % (
            int((r["map"] != maps).sum()), maps.size, float(np.abs(r["map"] - maps).max()))
    err = np.abs(r["ssim"] - means).max()
    print("%dx%d win %d: max |ssim - fsum / count| = %.3e (bound %.3e)" % (w, h, win, err, count * 2.0 ** -53))
    assert r["ssim"].shape == (n, 3) and err <= count * 2.0 ** -53


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("win,h,w", CASES)
def test_map_and_sums_equal_the_restatement(win, h, w, route):
    a, b = _pair(h, w)
    r = _call(a, b, win, route, want_map=True)
    _check(r, h, w, win)
    again = _call(a, b, win, route, want_map=True)           # two calls agree bitwise
    assert np.array_equal(r["ssim"].view(np.uint64), again["ssim"].view(np.uint64)) and np.array_equal(r["sse"], again["sse"])
    assert np.array_equal(r["map"].view(np.uint64), again["map"].view(np.uint64))


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("h,w", [(37, 53), (24, 40)])
def test_three_different_frames_in_one_call(h, w, route):
    a, b = _pair(h, w, 3)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    _check(_call(a, b, 7, route, want_map=True), h, w, 7, n=3)
    sse, maps, _ = _expected(h, w, 7, 3)
    assert len({tuple(row) for row in sse.tolist()}) == 3    # a frame-stride slip would show


@pytest.mark.parametrize("win,h,w", [(7, 40, 64), (7, 37, 53), (15, 130, 197), (3, TY + 2, 4 * ((TX + 5) // 4))])
def test_pointers_one_byte_off_take_the_byte_path(win, h, w):
    a, b = _pair(h, w)
    _check(_call(a, b, win, "device", misalign=True, want_map=True), h, w, win)
    r = _call(a, b, win, "device", misalign=True, want_ssim=False)
    assert r["ssim"] is None and np.array_equal(r["sse"], _expected(h, w, win)[0])


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("h,w,n", [(7, 7, 1), (37, 53, 1), (40, 64, 1), (130, 197, 1), (24, 40, 3), (37, 53, 3), (3, 5, 2)])
def test_sse_alone_and_ssim_without_the_map(h, w, n, route):
    """The SSE-only call runs the streaming kernel (12-byte groups when 3 h w is a multiple of 12 and the pointers are aligned, else
    bytes; 130 x 197 spans several workgroups; 3 x 5: less than one group per frame)."""
    a, b = _pair(h, w, n)
    win = 3 if h < 7 else 7
    assert 3 * h * w > SSE_BYTES or (h, w) != (130, 197)
    r = _call(a, b, win, route, want_ssim=False)
    assert r["ssim"] is None and "map" not in r and np.array_equal(r["sse"], R.sse(a, b))
    r = _call(a, b, win, route)
    assert "map" not in r
    _check(r, h, w, win, n=n, want_map=False)


@pytest.mark.parametrize("win", WINS)
def test_identical_constant_and_extreme_frames(win):
    import aiod_amd
    a, _ = _pair(37, 53)
    r = aiod_amd.frame_fidelity(a[0], a[0].copy(), win, want_map=True)
    assert not r["sse"].any() and np.array_equal(r["map"], np.ones_like(r["map"])) and np.array_equal(r["ssim"], np.ones((1, 3)))
    assert aiod_amd.psnr_from_sse(r["sse"][0], 37 * 53) == float("inf")
    x, y = np.full((17, 19, 3), 100, np.uint8), np.full((17, 19, 3), 50, np.uint8)
    r = aiod_amd.frame_fidelity(x, y, win, want_map=True)
    assert np.array_equal(r["map"][0].view(np.uint64), R.ssim_map(x, y, win).view(np.uint64)) and np.array_equal(r["sse"], np.full((1, 3), 17 * 19 * 2500, np.uint64))
    white, black = np.full((16, 16, 3), 255, np.uint8), np.zeros((16, 16, 3), np.uint8)
    r = aiod_amd.frame_fidelity(white, black, win, want_map=True)
    assert np.array_equal(r["map"][0].view(np.uint64), R.ssim_map(white, black, win).view(np.uint64))
    assert abs(float(r["ssim"][0, 0]) - 9.999e-05) < 1e-8 and aiod_amd.psnr_from_sse(r["sse"][0], 256) == 0.0


# ---- the flicker synthesiser and the plane wrapper ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["global", "local"])
def test_synth_flicker_equals_its_restatement(kind):
    import aiod_amd
    frames = [R.make_pair(37, 53, 40 + k)[0] for k in range(3)]
    out, planes = aiod_amd.synth_flicker(frames, kind=kind, strength=0.2, grid=(3, 4), seed=5)
    want, ref_planes = R.flicker(frames, kind, 0.2, (3, 4), 5)
    assert out.shape == (3, 37, 53, 3) and out.dtype == np.uint8 and np.array_equal(out, want)
    assert all(np.array_equal(a, ra) and np.array_equal(b, rb) for (a, b), (ra, rb) in zip(planes, ref_planes))
    assert any(not np.array_equal(o, f) for o, f in zip(out, frames))


def test_guided_apply_with_zero_planes_returns_the_frame():
    import torch
    import aiod_amd
    f = R.make_pair(37, 53, 3)[0]
    for shape in ((1, 1, 3), (4, 4, 3), (37, 53, 3)):
        zero = np.zeros(shape, np.float32)
        assert np.array_equal(aiod_amd.guided_apply(f, zero, zero), f)
    z = torch.zeros((2, 3, 3), device="cuda")
    assert np.array_equal(aiod_amd.guided_apply_device(torch.from_numpy(f).cuda(), z, z).cpu().numpy(), f)
    plus = aiod_amd.guided_apply(np.full((5, 6, 3), 100, np.uint8), np.zeros((1, 1, 3), np.float32), np.full((1, 1, 3), 7, np.float32))
    assert np.array_equal(plus, np.full((5, 6, 3), 107, np.uint8))


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
H, W, DOWN, SEED, N = 130, 197, 4, 11, 3
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


def _deflicker(**kw):
    import aiod_amd
    import pipeline_bench as PB
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    return aiod_amd.Deflicker(*PB.synthetic_weights(), config=dict(REFERENCE_CONFIG, **SHORT), down=DOWN, seed=SEED, **kw)


def _frames():
    import pipeline_bench as PB
    return PB.synthetic_clip(N, H, W, seed=5)


def _summary(a, b, win=7):
    import aiod_amd
    r = aiod_amd.frame_fidelity(np.stack(list(a)), np.stack(list(b)), win)
    return aiod_amd.summarise(r["sse"], r["ssim"], H, W)


def test_run_with_fidelity_changes_no_byte_and_reports_the_direct_call():
    frames = _frames()
    plain = _deflicker().run(frames)
    res = _deflicker().run(frames, fidelity=True)
    assert np.array_equal(res["final"], plain["final"]) and "fidelity" not in plain and "fidelity" not in plain["seconds"]
    assert set(res) - set(plain) == {"fidelity"} and set(res["seconds"]) - set(plain["seconds"]) == {"fidelity"}
    assert res["fidelity"] == {"window": 7, "size": [H, W], "final_vs_input": _summary(frames, res["final"])}
    assert any(not np.array_equal(res["final"][i], frames[i]) for i in range(N))


def test_proxy_route_reports_the_full_size():
    frames = _frames()
    res = _deflicker(proxy_long_edge=195, proxy_radius=5).run(frames, fidelity=9)
    assert res["proxy"]["size"] != [H, W] and res["final"].shape == (N, H, W, 3)
    assert res["fidelity"]["size"] == [H, W] and res["fidelity"]["window"] == 9
    assert res["fidelity"]["final_vs_input"] == _summary(frames, res["final"], 9)


def test_run_on_a_flickered_clip_with_its_clean_reference():
    import aiod_amd
    frames = _frames()
    flickered, _ = aiod_amd.synth_flicker(frames)
    res = _deflicker().run(list(flickered), fidelity=True, reference=frames)
    assert set(res["fidelity"]) == {"window", "size", "final_vs_input", "input_vs_reference", "final_vs_reference"}
    assert res["fidelity"]["input_vs_reference"] == _summary(flickered, frames)
    assert res["fidelity"]["final_vs_reference"] == _summary(res["final"], frames)
    assert res["fidelity"]["final_vs_input"] == _summary(res["final"], flickered)
