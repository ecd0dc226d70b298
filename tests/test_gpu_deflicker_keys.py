"""The key-mask route of the one-process pipeline on the GPU (aiod_amd.Deflicker.run(frames, mask_keys=...), deflicker.py --mask_keys_dir;
masks.py).

Every comparison is exact, for the reasons tests/test_gpu_deflicker_seg.py and tests/test_gpu_shots.py give: the route calls the entry
points the `masks=` route calls, on the same values in the same order; a key is resized by the arithmetic a mask is resized by; the
propagation kernels are single rounded fp32 operations (tests/test_gpu_maskprop.py); a shot is treated as a clip of its own.

Inputs are those of tests/test_gpu_deflicker_seg.py, restated: tools/pipeline_bench's synthetic clip of 130 x 197, its synthetic
weights and masks, --down 4, seed 11, the SHORT config with stop_bootstrapping_iteration 20."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as PB  # noqa: E402

H, W, DOWN, SEED = 130, 197, 4, 11
RESY, RESX = H // DOWN, W // DOWN
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15,
         "stop_bootstrapping_iteration": 20}
KEEP = ("final", "stage1", "masks", "flows")


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("deflicker_keys_assets")
    weights = PB.synthetic_weights()
    cfg = dict(REFERENCE_CONFIG, **SHORT)
    with open(d / "short.json", "w") as f:
        json.dump(cfg, f)
    shot_b = [np.ascontiguousarray(f.transpose(1, 0, 2)) for f in PB.synthetic_clip(3, W, H, seed=9, motion=(-2.0, 1.0))]
    masks_b = [np.ascontiguousarray(m.T) for m in PB.synthetic_masks(3, W, H, motion=(-2.0, 1.0))]
    return {"dir": d, "weights": weights, "paths": PB.write_weights(str(d / "weights"), weights), "cfg": cfg, "cfg_path": str(d / "short.json"),
            "frames": PB.synthetic_clip(4, H, W, seed=5), "masks": PB.synthetic_masks(4, H, W), "shot_b": shot_b, "masks_b": masks_b}


def _mk(assets, seed=SEED, **kw):
    import aiod_amd
    return aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"], down=DOWN, seed=seed, **kw)


@pytest.fixture(scope="module")
def default_first(assets):
    """The default single-atlas run of this process, made before any key-mask run."""
    return _mk(assets).run(assets["frames"][:3], keep=("final", "stage1"))


def test_a_key_on_every_frame_is_the_masks_route(assets, default_first):
    n = 4
    want = _mk(assets).run(assets["frames"], masks=assets["masks"], keep=("final", "stage1"))
    got = _mk(assets).run(assets["frames"], mask_keys={i: assets["masks"][i] for i in range(n)}, keep=KEEP)
    assert got["two_layer"] is True and got["mask_keys"] == [0, 1, 2, 3] and want["mask_keys"] is None and got["mask_thresh"] == 1.0
    for name in ("final", "stage1"):
        assert np.array_equal(got[name], want[name]), "%s differs in %d values" % (name, int((got[name] != want[name]).sum()))
    assert got["psnr"] == want["psnr"] and got["windows"] == want["windows"] == [(0, 4)]
    assert got["masks"].shape == (n, RESY, RESX) and got["masks"].dtype == np.float32
    assert not np.array_equal(got["stage1"][:3], default_first["stage1"])      # two layers, not one


def test_keys_at_both_ends_propagate_along_the_runs_own_flows(assets, tmp_path):
    from aiod_amd import deflicker, propagate_masks_device
    n = 4
    keys = {0: assets["masks"][0], n - 1: assets["masks"][n - 1][:, :, None]}      # (Hm, Wm) and (Hm, Wm, 1) are both taken
    d = _mk(assets)
    r = d.run(assets["frames"], mask_keys=keys, keep=KEEP)
    assert r["two_layer"] is True and r["mask_keys"] == [0, n - 1] and len(r["psnr"]) == 1 and np.isfinite(r["psnr"][0])
    assert r["final"].shape == (n, H, W, 3) and "masks" in r["seconds"]
    E = d.engines
    small = {i: E.resize_mask(E.mask(assets["masks"][i]), RESY, RESX) for i in keys}
    for i in keys:                                                          # the key planes are the resized keys, untouched
        assert np.array_equal(r["masks"][i].view(np.uint32), small[i].cpu().numpy().view(np.uint32))
    # ... and those are the planes the masks= route builds: put_mask_device's arithmetic
    t = E.inputs([E.frame(f) for f in assets["frames"]], [], [], RESY, RESX, masks=[E.mask(m) for m in assets["masks"]])
    assert torch.equal(t[5][:, :, 0], small[0]) and torch.equal(t[5][:, :, n - 1], small[n - 1])
    f12 = [E.resize_flow(a, RESY, RESX) for a, _ in r["flows"]]
    f21 = [E.resize_flow(b, RESY, RESX) for _, b in r["flows"]]
    want = propagate_masks_device(small, f12, f21).cpu().numpy()
    assert np.array_equal(r["masks"].view(np.uint32), want.view(np.uint32))
    inner = r["masks"][1:n - 1]
    assert ((inner > 0) & (inner < 1)).any() and (inner == 0).any() and (inner > 0.99).any()
    assert not np.array_equal(r["masks"][1], r["masks"][0])                 # propagated, not copied
    # the CLI on the same clip and keys: the same final frames, and the planes as PNGs
    PB.write_clip(str(tmp_path / "clip"), assets["frames"])
    PB.write_masks(str(tmp_path / "all"), assets["masks"])
    (tmp_path / "keys").mkdir()
    for i in keys:
        os.replace(tmp_path / "all" / ("%05d.png" % i), tmp_path / "keys" / ("%05d.png" % i))
    argv = ["--frames_dir", str(tmp_path / "clip"), "--out", str(tmp_path / "out"), "--config", assets["cfg_path"], "--down", str(DOWN), "--seed", str(SEED),
            "--model", assets["paths"][0], "--ckpt_filter", assets["paths"][1], "--ckpt_local", assets["paths"][2], "--mask_keys_dir", str(tmp_path / "keys")]
    assert deflicker.main(argv + ["--keep_intermediates"]) == 0
    rec = json.load(open(tmp_path / "out" / "deflicker.json"))
    assert rec["two_layer"] is True and rec["mask_keys"] == [0, n - 1] and rec["mask_thresh"] == 1.0 and rec["psnr"] == r["psnr"]
    for i in range(n):
        assert np.array_equal(_png(tmp_path / "out" / "final" / "output" / ("%05d.png" % i)), r["final"][i])
        assert np.array_equal(_png(tmp_path / "out" / "masks" / ("%05d.png" % i)), (r["masks"][i].astype(np.float64) * 255.0 + 0.5).astype(np.uint8))
    assert deflicker.main(argv + ["--masks_only", "--out", str(tmp_path / "only"), "--ckpt_filter", "absent.pth", "--ckpt_local", "absent.pth"]) == 0
    assert sorted(os.listdir(tmp_path / "only")) == ["deflicker.json", "masks"]
    for i in range(n):
        assert np.array_equal(_png(tmp_path / "only" / "masks" / ("%05d.png" % i)), _png(tmp_path / "out" / "masks" / ("%05d.png" % i)))


def test_two_shots_with_a_key_each_equal_the_two_stand_alone_runs(assets):
    """DESIGN.md §2.13's contract on this route: a shot equals the stand-alone run of its frames with its own keys, indices shifted;
    window k is fitted with seed + k."""
    a, b = assets["frames"][:3], assets["shot_b"]
    ka, kb = assets["masks"][1], assets["masks_b"][2]
    whole = _mk(assets, cuts=[3]).run(a + b, mask_keys={1: ka, 5: kb}, keep=KEEP)
    first = _mk(assets).run(a, mask_keys={1: ka}, keep=KEEP)
    second = _mk(assets, seed=SEED + 1).run(b, mask_keys={2: kb}, keep=KEEP)
    assert whole["shots"] == [(0, 3), (3, 6)] and whole["windows"] == [(0, 3), (3, 6)] and whole["mask_keys"] == [1, 5] and whole["flows"][2] is None
    for (lo, hi), alone, k in (((0, 3), first, 0), ((3, 6), second, 1)):
        for name in ("final", "stage1"):
            assert np.array_equal(whole[name][lo:hi], alone[name]), "%s of shot %d differs in %d values" % (name, k, int((whole[name][lo:hi] != alone[name]).sum()))
        assert np.array_equal(whole["masks"][lo:hi].view(np.uint32), alone["masks"].view(np.uint32))
        assert whole["psnr"][k] == alone["psnr"][0]
    with pytest.raises(ValueError, match=r"shot 1 \(frames 3\.\.5\) holds no key mask"):
        _mk(assets, cuts=[3]).run(a + b, mask_keys={1: ka})


def test_the_default_route_afterwards_is_a_fresh_default_run(assets, default_first):
    again = _mk(assets).run(assets["frames"][:3], keep=("final", "stage1"))
    assert again["two_layer"] is False and again["mask_keys"] is None
    assert np.array_equal(again["final"], default_first["final"]) and np.array_equal(again["stage1"], default_first["stage1"])
    assert again["psnr"] == default_first["psnr"]
