"""The one-process pipeline on the GPU (aiod_amd.Deflicker, all-in-one-deflicker_amd/deflicker.py, af_render_frame_u8).

Every comparison here is exact.  The tolerance is derived, not measured: the in-process route and the three chained CLIs run the same
kernels on the same values with fixed-order reductions, float32 .npy and PNG are lossless, and a window is fitted by the
code that fits a stand-alone clip.  A difference is a bug to locate by stage and by file.

Inputs: seeded synthetic frames of 130x197 (the RAFT fixture's size, padded to 136x200), the fixtures' synthetic weights, --down 4, a
short config (3 pre-train iterations, 31 iterations with the one evaluation at iteration 30), always a seed.  One departure from the
fixtures' fills, made for both routes alike (tools/pipeline_bench.synthetic_weights): RAFT's last flow-head convolution is scaled by
2^-4.  Unscaled, the synthetic RAFT returns ~14 px rms of noise, no pixel passes the input builder's forward/backward consistency test
(measured with the torch restatement of tools/make_golden_raft.py on the CPU: 0.0 - 0.1 % valid), so every stage-1 batch is without a
valid flow pixel and af_train_steps reports the NaN loss the reference has there too; scaled, the flows are ~0.9 px rms and every pixel
is valid."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as PB  # noqa: E402

H, W, DOWN, SEED = 130, 197, 4, 11
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


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
    d = tmp_path_factory.mktemp("deflicker_assets")
    weights = PB.synthetic_weights()
    paths = PB.write_weights(str(d / "weights"), weights)
    cfgs = {}
    for name, extra in (("short", {}), ("win5", {"maximum_number_of_frames": 5})):
        cfgs[name] = dict(REFERENCE_CONFIG, **SHORT, **extra)
        with open(d / (name + ".json"), "w") as f:
            json.dump(cfgs[name], f)
    return {"dir": d, "weights": weights, "paths": paths, "cfg": cfgs, "cfg_path": {k: str(d / (k + ".json")) for k in cfgs},
            "frames": PB.synthetic_clip(9, H, W, seed=5)}


@pytest.fixture(scope="module")
def api(assets):
    """run(frames, cfg name, seed, overlap, keep) through the Python API, cached: several tests compare against the same stand-alone runs."""
    import aiod_amd
    cache = {}

    def run(lo, hi, cfg="short", seed=SEED, overlap=0, keep=("final", "stage1", "renders")):
        key = (lo, hi, cfg, seed, overlap, tuple(keep))
        if key not in cache:
            d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"][cfg], down=DOWN, seed=seed, window_overlap=overlap)
            cache[key] = d.run(assets["frames"][lo:hi], keep=keep)
        return cache[key]
    return run


# ---- test 1: the render hand-off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_layer", [False, True])
def test_render_hand_off(two_layer):
    import aiod_amd
    from aiod_amd import stage1 as S
    resx, resy, F = 49, 32, 3
    g = torch.Generator().manual_seed(3)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(resx, resy, F, samples_batch=256, two_layer=two_layer))
    try:
        S.init_networks(af, {"pretrain_mapping1": False, "pretrain_mapping2": False}, two_layer, g)
        video = torch.rand((resy, resx, 3, F), generator=g).numpy()
        flows = torch.zeros((resy, resx, 2, F)).numpy()
        ones = torch.ones((resy, resx, F)).numpy()
        af.upload_video(video, flows, flows, ones, ones, torch.rand((resy, resx, F), generator=g).numpy() if two_layer else None)
        if not two_layer:
            af.train_steps(0, 5, None, seed=1, return_losses=False)
        for f in range(F):
            rgb, sse = af.render_frame(f)
            p_ref = af.psnr()
            d_rgb, d_u8, d_sse = af.render_frame_device(f)
            p_dev = af.psnr()
            h_rgb, h_u8, h_sse = af.render_frame_u8(f)
            p_host = af.psnr()
            expect = (rgb.astype(np.float64) * 255).astype(np.uint8)      # evaluate_model_single's truncation
            assert d_rgb.is_cuda and d_u8.is_cuda and d_u8.dtype == torch.uint8
            assert np.array_equal(d_rgb.cpu().numpy().view(np.uint32), rgb.view(np.uint32))
            assert np.array_equal(h_rgb.view(np.uint32), rgb.view(np.uint32))
            assert np.array_equal(d_u8.cpu().numpy(), expect) and np.array_equal(h_u8, expect)
            assert d_sse == sse == h_sse
            assert p_ref[0] == p_dev[0] == p_host[0] and np.array_equal(p_ref[1], p_dev[1]) and np.array_equal(p_ref[1], p_host[1])
            assert expect.min() < expect.max()
        only_u8 = af.render_frame_device(0, want_float=False)
        assert only_u8[0] is None and np.array_equal(only_u8[1].cpu().numpy(), (af.render_frame(0)[0].astype(np.float64) * 255).astype(np.uint8))
        with pytest.raises(aiod_amd.AtlasFitError, match="af_render_frame_u8: frame index"):
            af.render_frame_device(F)
    finally:
        af.close()


# ---- test 2: identity with the disk route --------------------------------------------------------------------------------------
def test_identity_with_the_three_chained_clis(assets, api, tmp_path):
    import aiod_amd
    n = 6
    frames = assets["frames"][:n]
    roots = {arm: tmp_path / arm for arm in ("in_process", "chained")}
    for r in roots.values():
        PB.write_clip(str(r / "data" / "test" / "clip"), frames)
    out = roots["in_process"] / "anywhere" / "clip"
    _run(PB.in_process_command(str(roots["in_process"] / "data" / "test" / "clip"), str(out), assets["cfg_path"]["short"], DOWN, SEED, assets["paths"],
                               extra=["--keep_intermediates", "--warp_error"]), tmp_path)
    for _, cmd in PB.chained_commands("clip", assets["cfg_path"]["short"], DOWN, SEED, assets["paths"]):
        _run(cmd, roots["chained"])
    ref = roots["chained"] / "results" / "clip"
    names = ["%05d.png" % i for i in range(n)]
    # flows: byte-identical files
    fa, fb = roots["in_process"] / "data" / "test" / "clip_flow", roots["chained"] / "data" / "test" / "clip_flow"
    flow_names = sorted(os.listdir(fb))
    assert len(flow_names) == 2 * (n - 1) and sorted(os.listdir(fa)) == flow_names
    for fn in flow_names:
        assert (fa / fn).read_bytes() == (fb / fn).read_bytes(), "flow %s differs" % fn
    # every PNG tree: identical decoded pixels
    for sub in (("stage_1", "output"), ("neural_filter", "output"), ("neural_filter", "concat"), ("final", "output")):
        a, b = out.joinpath(*sub), ref.joinpath(*sub)
        assert sorted(os.listdir(a)) == names == sorted(os.listdir(b)), sub
        for fn in names:
            x, y = _png(a / fn), _png(b / fn)
            assert x.dtype == np.uint8 and x.shape == y.shape and np.array_equal(x, y), "%s/%s differs in %d values" % ("/".join(sub), fn, int((x != y).sum()))
    assert _png(out / "stage_1" / "output" / names[0]).shape == (H // DOWN, W // DOWN, 3)
    assert _png(out / "neural_filter" / "concat" / names[0]).shape == (H, 3 * W, 3)
    rec = json.load(open(out / "deflicker.json"))
    assert rec["windows"] == [[0, n]] and rec["seam_pairs"] == [] and rec["seed"] == SEED and len(rec["psnr"]) == 1
    assert set(rec["seconds"]) >= {"decode + flow", "stage 1", "stage 2", "total"} and rec["arithmetic"][0]["mlp_mode"] in (0, 1, 2, 3)
    marker = [m for m in os.listdir(ref / "stage_1" / "000030") if m.startswith("PSNR_")]
    assert marker == ["PSNR_%f" % rec["psnr"][0]]
    we = rec["warp_error"]
    assert we["geometry"] == "exact" and len(we["input"]["per_pair"]) == n - 1 == len(we["final"]["per_pair"]) and we["seam_pairs"] == []
    # the same E_warp as warp_error.py measures on the chained route's files
    from aiod_amd import warp_error as WE
    files = WE.list_frames(roots["chained"] / "data" / "test" / "clip")
    pairs = WE.flow_pairs(files, fb)
    assert WE.measure_sequence(files, pairs, True)[1] == we["input"]["per_pair"]
    assert WE.measure_sequence(WE.list_frames(ref / "final" / "output"), pairs, True)[1] == we["final"]["per_pair"]
    # the API: a numpy list and a CUDA tensor give the CLI's final frames
    final_files = np.stack([_png(out / "final" / "output" / fn) for fn in names])
    r_np = api(0, n)
    assert isinstance(r_np["final"], np.ndarray) and np.array_equal(r_np["final"], final_files)
    d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["short"], down=DOWN, seed=SEED)
    r_t = d.run(torch.from_numpy(np.stack(frames)).cuda(), keep=("final", "stage1", "flows"))
    assert r_t["final"].is_cuda and r_t["final"].dtype == torch.uint8 and np.array_equal(r_t["final"].cpu().numpy(), final_files)
    assert np.array_equal(r_t["stage1"].cpu().numpy(), r_np["stage1"]) and len(r_t["flows"]) == n - 1
    assert r_np["psnr"] == rec["psnr"] == r_t["psnr"]


# ---- tests 3 and 5: windows without overlap, repeatability ---------------------------------------------------------------------
def test_windows_hard_cut_and_repeatability(assets, api, tmp_path):
    PB.write_clip(str(tmp_path / "clip9"), assets["frames"])
    out = tmp_path / "res"
    _run(PB.in_process_command(str(tmp_path / "clip9"), str(out), assets["cfg_path"]["win5"], DOWN, SEED, assets["paths"], extra=["--keep_intermediates"]), tmp_path)
    rec = json.load(open(out / "deflicker.json"))
    assert rec["windows"] == [[0, 5], [5, 9]] and rec["seam_pairs"] == [4] and len(rec["psnr"]) == 2 and rec["frames"] == 9
    names = ["%05d.png" % i for i in range(9)]
    assert sorted(os.listdir(out / "final" / "output")) == names
    final = np.stack([_png(out / "final" / "output" / fn) for fn in names])
    style = np.stack([_png(out / "stage_1" / "output" / fn) for fn in names])
    first, second = api(0, 5), api(5, 9, seed=SEED + 1)
    assert np.array_equal(final[0:5], first["final"])                      # stage 2 is causal: the later window cannot reach back
    assert np.array_equal(style[0:5], first["stage1"])
    assert np.array_equal(style[5:9], second["stage1"])                    # window 1 is the stand-alone clip 5..8 with seed + 1
    assert rec["psnr"] == [first["psnr"][0], second["psnr"][0]]
    # repeatability: the API in this process gives the child's bytes, twice
    for _ in range(2):
        import aiod_amd
        r = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["win5"], down=DOWN, seed=SEED).run(assets["frames"], keep=("final", "stage1"))
        assert r["windows"] == [(0, 5), (5, 9)] and r["seam_pairs"] == [4]
        assert np.array_equal(r["final"], final) and np.array_equal(r["stage1"], style)


# ---- test 4: windows with overlap 1 --------------------------------------------------------------------------------------------
def test_windows_cross_fade(assets, api):
    r = api(0, 9, cfg="win5", overlap=1)
    assert r["windows"] == [(0, 5), (4, 9)] and r["seam_pairs"] == [3, 4]
    first, second = api(0, 5), api(4, 9, seed=SEED + 1)
    ra, rb = r["renders"]
    assert ra.shape == rb.shape == (5, H // DOWN, W // DOWN, 3)
    assert ra.dtype == np.float32 and np.array_equal(ra, first["renders"][0]) and np.array_equal(rb, second["renders"][0])
    a, b = ra[4], rb[0]                                                     # frame 4 in both windows
    blend = b - (b - a) * np.float32(0.5)                                   # torch.lerp's form for a weight >= 1/2; the product by 1/2 is exact
    assert np.array_equal(blend, torch.lerp(torch.from_numpy(a), torch.from_numpy(b), 0.5).numpy())
    assert np.array_equal(r["stage1"][4], (blend.astype(np.float64) * 255).astype(np.uint8))
    assert not np.array_equal(r["stage1"][4], first["stage1"][4]) and not np.array_equal(r["stage1"][4], second["stage1"][0])
    assert np.array_equal(r["stage1"][0:4], first["stage1"][0:4]) and np.array_equal(r["stage1"][5:9], second["stage1"][1:5])
    assert np.array_equal(r["final"][0:4], first["final"][0:4])


# ---- test 6: errors ------------------------------------------------------------------------------------------------------------
def test_errors_name_the_cause_and_leave_the_process_usable(assets, api, tmp_path):
    import aiod_amd
    from aiod_amd import deflicker
    d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["short"], down=DOWN, seed=SEED)
    bad = list(assets["frames"][:4])
    bad[2] = np.zeros((H, W + 1, 3), np.uint8)
    with pytest.raises(ValueError, match="frame 2 is 198x130, the first frame 197x130"):
        d.run(bad)
    with pytest.raises(ValueError, match="at least 2 frames, got 1"):
        d.run(assets["frames"][:1])
    with pytest.raises(ValueError, match="window overlap 5 must be >= 0 and smaller than the window"):
        aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"]["win5"], window_overlap=5)
    PB.write_clip(str(tmp_path / "clip"), assets["frames"][:3])
    argv = ["--frames_dir", str(tmp_path / "clip"), "--out", str(tmp_path / "out"), "--config", assets["cfg_path"]["short"], "--seed", str(SEED),
            "--model", assets["paths"][0], "--ckpt_filter", assets["paths"][1], "--ckpt_local", assets["paths"][2]]
    with pytest.raises(SystemExit, match="nowhere.pth not found \\(--ckpt_local\\)"):
        deflicker.main(argv[:-1] + [str(tmp_path / "nowhere.pth")])
    PB.write_clip(str(tmp_path / "mixed"), bad)
    with pytest.raises(SystemExit, match="frame 2 is 198x130"):
        deflicker.main(["--frames_dir", str(tmp_path / "mixed")] + argv[2:])
    with pytest.raises(SystemExit, match="window overlap"):
        deflicker.main(argv + ["--window_overlap", "200"])
    wrong = dict(assets["weights"][1]); wrong.pop("conv.bias")
    with pytest.raises(aiod_amd.StateDictError, match="missing key 'conv.bias'"):      # fails in stage 2, after RAFT and the fit: every handle is closed on the way out
        aiod_amd.Deflicker(assets["weights"][0], wrong, assets["weights"][2], config=assets["cfg"]["short"], down=DOWN, seed=SEED).run(assets["frames"][:3])
    # after every failure above the same process still runs, and computes what a fresh one computes
    assert deflicker.main(argv) == 0
    got = np.stack([_png(tmp_path / "out" / "final" / "output" / ("%05d.png" % i)) for i in range(3)])
    assert np.array_equal(got, d.run(assets["frames"][:3])["final"])
