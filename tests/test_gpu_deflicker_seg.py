"""The fg/bg two-layer route of the one-process pipeline on the GPU (aiod_amd.Deflicker.run(frames, masks=...), deflicker.py --masks_dir).

Every comparison here is exact, for the reason tests/test_gpu_deflicker.py gives: the in-process route and the three chained CLIs
(preprocess_optical_flow.py, stage1_seg.py --down D --seed S --skip_preprocess, neural_filter.py) call the same entry points on the same
values, the reductions are fixed-order, float32 .npy and PNG are lossless, and a window is fitted by the code that fits a
stand-alone two-layer clip.  A difference is a bug to locate by stage and by file, not a tolerance to widen.

Inputs as in tests/test_gpu_deflicker.py: tools/pipeline_bench.synthetic_clip frames of 130x197, its synthetic weights (flow head scaled),
--down 4, seed 11, the SHORT config plus stop_bootstrapping_iteration 20: global rigidity stops at iteration 15 and the alpha
bootstrapping at 20, so both two-layer switches are crossed inside the 31 iterations.  The masks are
tools/pipeline_bench.synthetic_masks: a soft-edged blob that moves with the clip's pattern."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as PB  # noqa: E402

H, W, DOWN, SEED = 130, 197, 4, 11
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15,
         "stop_bootstrapping_iteration": 20}


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(str(c) for c in cmd) + "\n" + r.stdout[-2000:] + r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("deflicker_seg_assets")
    weights = PB.synthetic_weights()
    paths = PB.write_weights(str(d / "weights"), weights)
    cfgs = {}
    for name, extra in (("short", {}), ("win5", {"maximum_number_of_frames": 5})):
        cfgs[name] = dict(REFERENCE_CONFIG, **SHORT, **extra)
        with open(d / (name + ".json"), "w") as f:
            json.dump(cfgs[name], f)
    return {"dir": d, "weights": weights, "paths": paths, "cfg": cfgs, "cfg_path": {k: str(d / (k + ".json")) for k in cfgs},
            "frames": PB.synthetic_clip(9, H, W, seed=5), "masks": PB.synthetic_masks(9, H, W)}


@pytest.fixture(scope="module")
def api(assets):
    """run(lo, hi, cfg name, seed, overlap, keep, masks) through the Python API, cached: several tests compare against the same
    stand-alone runs.  masks: "own" (the frames' masks), "reversed" (the same masks in reverse order) or None (single atlas)."""
    import aiod_amd
    cache = {}

    def run(lo, hi, cfg="short", seed=SEED, overlap=0, keep=("final", "stage1", "renders"), masks="own", fresh=False):
        key = (lo, hi, cfg, seed, overlap, tuple(keep), masks)
        if fresh or key not in cache:
            d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"][cfg], down=DOWN, seed=seed, window_overlap=overlap)
            m = {"own": assets["masks"][lo:hi], "reversed": assets["masks"][lo:hi][::-1], None: None}[masks]
            r = d.run(assets["frames"][lo:hi], masks=m, keep=keep)
            if fresh:
                return r
            cache[key] = r
        return cache[key]
    return run


# ---- test 1: identity with the three CLIs chained, stage1_seg.py in the middle ------------------------------------------------
def test_identity_with_the_three_chained_clis(assets, api, tmp_path):
    import aiod_amd
    n = 6
    frames, masks = assets["frames"][:n], assets["masks"][:n]
    roots = {arm: tmp_path / arm for arm in ("in_process", "chained")}
    for r in roots.values():
        PB.write_clip(str(r / "data" / "test" / "clip"), frames)
        PB.write_masks(str(r / "data" / "test" / "clip_seg"), masks)
    out = roots["in_process"] / "anywhere" / "clip"
    _run(PB.in_process_command(str(roots["in_process"] / "data" / "test" / "clip"), str(out), assets["cfg_path"]["short"], DOWN, SEED, assets["paths"],
                               extra=["--keep_intermediates"], masks_dir=str(roots["in_process"] / "data" / "test" / "clip_seg")), tmp_path)
    cmds = PB.chained_commands("clip", assets["cfg_path"]["short"], DOWN, SEED, assets["paths"], two_layer=True)
    assert os.path.basename(cmds[1][1][1]) == "stage1_seg.py" and cmds[1][1][cmds[1][1].index("--down") + 1] == str(DOWN)
    for _, cmd in cmds:
        _run(cmd, roots["chained"])
    ref = roots["chained"] / "results" / "clip"
    names = ["%05d.png" % i for i in range(n)]
    fa, fb = roots["in_process"] / "data" / "test" / "clip_flow", roots["chained"] / "data" / "test" / "clip_flow"
    flow_names = sorted(os.listdir(fb))
    assert len(flow_names) == 2 * (n - 1) and sorted(os.listdir(fa)) == flow_names
    for fn in flow_names:
        assert (fa / fn).read_bytes() == (fb / fn).read_bytes(), "flow %s differs" % fn
    for sub in (("stage_1", "output"), ("neural_filter", "output"), ("neural_filter", "concat"), ("final", "output")):
        a, b = out.joinpath(*sub), ref.joinpath(*sub)
        assert sorted(os.listdir(a)) == names == sorted(os.listdir(b)), sub
        for fn in names:
            x, y = _png(a / fn), _png(b / fn)
            assert x.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y), "%s/%s differs in %d values" % ("/".join(sub), fn, int((x != y).sum()))
    assert _png(out / "stage_1" / "output" / names[0]).shape == (H // DOWN, W // DOWN, 3)
    rec = json.load(open(out / "deflicker.json"))
    assert rec["two_layer"] is True and rec["masks_dir"] == str(roots["in_process"] / "data" / "test" / "clip_seg")
    assert rec["windows"] == [[0, n]] and rec["seed"] == SEED and len(rec["psnr"]) == 1 and np.isfinite(rec["psnr"][0])
    marker = [m for m in os.listdir(ref / "stage_1" / "000030") if m.startswith("PSNR_")]
    assert marker == ["PSNR_%f" % rec["psnr"][0]]
    # the chained route did fit two layers: its checkpoint holds the four nets
    ck = torch.load(str(ref / "stage_1" / "checkpoint"), map_location="cpu", weights_only=False)
    assert "model_F_alpha_state_dict" in ck and "model_F_mapping2_state_dict" in ck
    # the API: numpy masks and one CUDA mask tensor give the CLI's final frames
    final_files = np.stack([_png(out / "final" / "output" / fn) for fn in names])
    style_files = np.stack([_png(out / "stage_1" / "output" / fn) for fn in names])
    r_np = api(0, n)
    assert r_np["two_layer"] is True and isinstance(r_np["final"], np.ndarray)
    assert np.array_equal(r_np["final"], final_files) and np.array_equal(r_np["stage1"], style_files)
    d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["short"], down=DOWN, seed=SEED)
    r_t = d.run(frames, masks=torch.from_numpy(np.stack(masks)).cuda(), keep=("final", "stage1"))
    assert np.array_equal(r_t["final"], final_files) and np.array_equal(r_t["stage1"], style_files)
    assert r_np["psnr"] == rec["psnr"] == r_t["psnr"]


# ---- test 2: the mask hand-off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,channels", [(False, 1), (True, 1), (True, 3)])
def test_mask_hand_off(half, channels, tmp_path):
    """mask_frames from device masks against load_input_data_device(with_masks=True) on the same masks as PNG files, at 49x32."""
    from PIL import Image
    from aiod_amd import stage1 as S
    from aiod_amd.deflicker import DeviceEngines
    resy, resx, F = H // DOWN, W // DOWN, 3
    assert (resy, resx) == (32, 49)
    frames = PB.synthetic_clip(F, H, W, seed=2)
    hm, wm = (H // 2, W // 2) if half else (H, W)
    masks = PB.synthetic_masks(F, hm, wm, motion=(3.0, -2.0))
    if channels == 3:                                                       # channel 0 is the mask; the others must not be read
        masks = [np.dstack([m, 255 - m, np.full_like(m, 77)]) for m in masks]
    PB.write_clip(str(tmp_path / "clip"), frames)
    (tmp_path / "clip_seg").mkdir()
    (tmp_path / "clip_flow").mkdir()
    for i, m in enumerate(masks):
        Image.fromarray(m).save(str(tmp_path / "clip_seg" / ("%05d.png" % i)))
    rng = np.random.default_rng(4)
    flows = [(0.3 * rng.standard_normal((resy, resx, 2))).astype(np.float32) for _ in range(2 * (F - 1))]
    for i in range(F - 1):
        a, b = "%05d.png" % i, "%05d.png" % (i + 1)
        np.save(tmp_path / "clip_flow" / ("%s_%s.npy" % (a, b)), flows[2 * i])
        np.save(tmp_path / "clip_flow" / ("%s_%s.npy" % (b, a)), flows[2 * i + 1])
    want = S.load_input_data_device(resy, resx, 200, tmp_path / "clip", True, tmp_path, "clip", with_masks=True)
    E = DeviceEngines(None, None, None)
    dev = [torch.from_numpy(f).cuda() for f in flows]
    got = E.inputs([E.frame(f) for f in frames], dev[0::2], dev[1::2], resy, resx, masks=[E.mask(m) for m in masks])
    assert len(got) == len(want) == 6 and got[5].shape == (resy, resx, F) and got[5].dtype == torch.float32
    for g, w_ in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), w_.cpu().numpy().view(np.uint32))
    mf = got[5].cpu().numpy()
    assert ((mf > 0) & (mf < 1)).any() and (mf == 0).any() and (mf > 0.99).any()      # fractional: a nearest-neighbour resize of these masks would not pass
    assert len(S.alloc_input_tensors(resy, resx, F, torch.device("cuda", 0))) == 5      # the single-atlas builder has no mask tensor


# ---- test 3: windows, hard cut ---------------------------------------------------------------------------------------------------
def test_windows_hard_cut_and_repeatability(api):
    r = api(0, 9, cfg="win5", keep=("final", "stage1"))
    assert r["windows"] == [(0, 5), (5, 9)] and r["seam_pairs"] == [4] and r["two_layer"] is True and len(r["psnr"]) == 2
    first, second = api(0, 5), api(5, 9, seed=SEED + 1)
    assert np.array_equal(r["stage1"][5:9], second["stage1"])              # window 1: the stand-alone two-layer clip 5..8, masks 5..8, seed + 1
    assert np.array_equal(r["stage1"][0:5], first["stage1"])
    assert np.array_equal(r["final"][0:5], first["final"])                 # stage 2 is causal
    assert r["psnr"] == [first["psnr"][0], second["psnr"][0]]
    again = api(0, 9, cfg="win5", keep=("final", "stage1"), fresh=True)
    assert np.array_equal(again["final"], r["final"]) and np.array_equal(again["stage1"], r["stage1"]) and again["psnr"] == r["psnr"]


# ---- test 4: windows with overlap 1 ----------------------------------------------------------------------------------------------
def test_windows_cross_fade(api):
    r = api(0, 9, cfg="win5", overlap=1)
    assert r["windows"] == [(0, 5), (4, 9)] and r["seam_pairs"] == [3, 4] and r["two_layer"] is True
    first, second = api(0, 5), api(4, 9, seed=SEED + 1)
    ra, rb = r["renders"]
    assert ra.shape == rb.shape == (5, H // DOWN, W // DOWN, 3) and ra.dtype == np.float32
    assert np.array_equal(ra, first["renders"][0]) and np.array_equal(rb, second["renders"][0])
    a, b = ra[4], rb[0]                                                     # frame 4 in both windows: the composited float renders
    blend = torch.lerp(torch.from_numpy(a), torch.from_numpy(b), 0.5).numpy()
    assert np.array_equal(r["stage1"][4], (blend.astype(np.float64) * 255).astype(np.uint8))      # quantise_render's truncation
    assert not np.array_equal(r["stage1"][4], first["stage1"][4]) and not np.array_equal(r["stage1"][4], second["stage1"][0])
    assert np.array_equal(r["stage1"][0:4], first["stage1"][0:4]) and np.array_equal(r["stage1"][5:9], second["stage1"][1:5])
    assert np.array_equal(r["final"][0:4], first["final"][0:4])


# ---- test 5: the masks reach the fit ---------------------------------------------------------------------------------------------
def test_the_masks_reach_the_fit(api):
    keep = ("final", "stage1")
    single_before = api(0, 5, keep=keep, masks=None, fresh=True)
    two = api(0, 5)
    flipped = api(0, 5, keep=keep, masks="reversed")
    single_after = api(0, 5, keep=keep, masks=None, fresh=True)
    assert single_before["two_layer"] is False and two["two_layer"] is True and flipped["two_layer"] is True
    assert not np.array_equal(two["stage1"], single_before["stage1"])      # two layers, not one
    assert not np.array_equal(two["stage1"], flipped["stage1"])            # and these masks, in this order
    assert np.array_equal(single_before["stage1"], single_after["stage1"]) and np.array_equal(single_before["final"], single_after["final"])
    assert single_before["psnr"] == single_after["psnr"]


# ---- test 6: errors --------------------------------------------------------------------------------------------------------------
def test_errors_name_the_cause_and_leave_the_process_usable(assets, api, tmp_path):
    import aiod_amd
    from PIL import Image
    from aiod_amd import deflicker
    frames, masks = assets["frames"][:3], assets["masks"][:3]
    d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["short"], down=DOWN, seed=SEED)
    with pytest.raises(ValueError, match="2 masks for 3 frames"):
        d.run(frames, masks=masks[:2])
    with pytest.raises(ValueError, match="2 masks for 3 frames"):
        d.run(iter(frames), masks=iter(masks[:2]))                          # counted after RAFT, still before the fit
    with pytest.raises(ValueError, match="mask 1 must be uint8, got float32"):
        d.run(frames, masks=[masks[0], masks[1].astype(np.float32), masks[2]])
    with pytest.raises(ValueError, match="masks must be uint8, got torch.float32"):
        d.run(frames, masks=torch.zeros((3, H, W), device="cuda"))
    with pytest.raises(ValueError, match=r"masks must be \(N, Hm, Wm\) or \(N, Hm, Wm, C\) uint8, got \(3, 130\)"):
        d.run(frames, masks=torch.zeros((3, H), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match=r"got \(3, 130, 197, 1, 1\)"):
        d.run(frames, masks=torch.zeros((3, H, W, 1, 1), dtype=torch.uint8, device="cuda"))
    # the CLI: too few masks, a 16-bit mask
    PB.write_clip(str(tmp_path / "clip"), frames)
    PB.write_masks(str(tmp_path / "clip_seg"), masks)
    PB.write_masks(str(tmp_path / "few"), masks[:2])
    PB.write_masks(str(tmp_path / "deep"), masks)
    Image.fromarray(masks[1].astype(np.uint16) * 257).save(str(tmp_path / "deep" / "00001.png"))
    argv = ["--frames_dir", str(tmp_path / "clip"), "--out", str(tmp_path / "out"), "--config", assets["cfg_path"]["short"], "--seed", str(SEED),
            "--model", assets["paths"][0], "--ckpt_filter", assets["paths"][1], "--ckpt_local", assets["paths"][2]]
    with pytest.raises(SystemExit) as e:
        deflicker.main(argv + ["--masks_dir", str(tmp_path / "few")])
    assert "2 masks" in str(e.value) and "3 frames" in str(e.value) and str(tmp_path / "few") in str(e.value)
    with pytest.raises(SystemExit, match="00001.png: only 8-bit masks are handled"):
        deflicker.main(argv + ["--masks_dir", str(tmp_path / "deep")])
    # a failure while the pre-train thread of a two-layer window runs (the builder raises), and one after the fit (stage 2's weights)
    class _Broken(deflicker.DeviceEngines):
        def inputs(self, *a, **k):
            raise RuntimeError("builder failed")
    broken = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["short"], down=DOWN, seed=SEED, engines=_Broken(*assets["weights"]))
    with pytest.raises(RuntimeError, match="builder failed"):
        broken.run(frames, masks=masks)
    assert not [t for t in threading.enumerate() if t.name == "af-pretrain"]      # joined before the handle was closed
    wrong = dict(assets["weights"][1]); wrong.pop("conv.bias")
    with pytest.raises(aiod_amd.StateDictError, match="missing key 'conv.bias'"):
        aiod_amd.Deflicker(assets["weights"][0], wrong, assets["weights"][2], config=assets["cfg"]["short"], down=DOWN, seed=SEED).run(frames, masks=masks)
    # after every failure above the same process still runs the two-layer route, and computes what a fresh object computes
    assert deflicker.main(argv + ["--masks_dir", str(tmp_path / "clip_seg")]) == 0
    got = np.stack([_png(tmp_path / "out" / "final" / "output" / ("%05d.png" % i)) for i in range(3)])
    assert json.load(open(tmp_path / "out" / "deflicker.json"))["two_layer"] is True
    assert np.array_equal(got, api(0, 3, keep=("final",))["final"])
    assert np.array_equal(got, d.run(frames, masks=masks)["final"])
