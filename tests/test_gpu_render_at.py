"""af_render_frame_at on the GPU: the fitted nets evaluated on a grid other than the stage-1 lattice (include/atlasfit.h).  The 40x24x6
clips of conftest.py; the oracle's models at the restated coordinates (tests/render_at_ref.py) are the reference, with the rule and the
floor of test_gpu_parity.py::test_render_matches_oracle_per_pixel; same-size and coinciding pixels are held bit for bit against
af_render_frame."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import render_at_ref as R  # noqa: E402

SIZES = [(41, 67), (72, 120), (12, 20)]      # non-integer factors and a ragged last tile; k = 3 in nine bands; a down-scale


def _nets(two_layer):
    import aiod_amd
    return (aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2, aiod_amd.NET_ATLAS, aiod_amd.NET_ALPHA) if two_layer else (aiod_amd.NET_MAPPING1, aiod_amd.NET_ATLAS)


def _models(g, two_layer):
    if two_layer:
        from conftest import seg_start_models
        return list(seg_start_models(g))
    from test_gpu_parity import _oracle_models
    return list(_oracle_models(g))


def _handle(g, v, two_layer, models, upload=True):
    import aiod_amd
    h = aiod_amd.AtlasFit(aiod_amd.default_config(int(g["resx"]), int(g["resy"]), int(g["nframes"]), dict(g["config"]), two_layer=two_layer))
    if upload:
        h.upload_video(v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, v.optical_flows_reverse_mask,
                       *((v.mask_frames,) if two_layer else ()))
    for net, m in zip(_nets(two_layer), models):
        h.load_state_dict(net, m.state_dict())
    return h


def _frame_u8(v, f):
    return np.ascontiguousarray((v.video_frames[:, :, :, f].numpy().astype(np.float64) * 255.0).round().clip(0, 255).astype(np.uint8))


CASES = [("single", "golden", "small_video"), ("single_field", "golden_field", "small_video_field"),
         ("seg", "golden_seg", "small_seg_video"), ("seg_field", "golden_seg_field", "small_seg_video_field")]


@pytest.fixture(scope="module")
def handles(request):
    """{name: (handle, fixture, video, two_layer, oracle models)}: one handle per path and video, the oracle's start state loaded."""
    out = {}
    for name, gname, vname in CASES:
        g, v = request.getfixturevalue(gname), request.getfixturevalue(vname)
        two = name.startswith("seg")
        models = _models(g, two)
        out[name] = (_handle(g, v, two, models), g, v, two, models)
    yield out
    for c in out.values():
        c[0].close()


@pytest.fixture(params=[c[0] for c in CASES])
def case(request, handles):
    return handles[request.param]


@pytest.fixture(params=["single", "seg"])
def case2(request, handles):
    return handles[request.param]


def _frames(v):
    return (0, v.F // 2, v.F - 1)


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------
def test_same_size_is_render_frame_bit_for_bit(case2):
    """One finish kernel through two host routes: af_render_frame / af_render_frame_u8 (error against the record table, cached for
    af_psnr) and af_render_frame_at at (resy, resx) (error against a uint8 image, no cache) return the same colours and bytes."""
    h, g, v, two, _ = case2
    for f in _frames(v):
        want, _ = h.render_frame(f)
        _, want_u8, _ = h.render_frame_u8(f)
        ref = _frame_u8(v, f)
        got, got_u8, sse = h.render_frame_at_u8(f, v.resy, v.resx, ref=ref)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (f, np.abs(got - want).max())
        assert np.array_equal(got_u8, want_u8)
        host = float(((ref.astype(np.float64) / 255.0 - got.astype(np.float64)) ** 2).sum())
        print("frame %d: sse %.17g, host fp64 sum %.17g" % (f, sse, host))
        assert abs(sse - host) <= 1e-12 * host, (f, sse, host)
        assert np.array_equal(h.render_frame_at(f, v.resy, v.resx).view(np.uint32), want.view(np.uint32))


# ---- 2. coinciding pixels ----------------------------------------------------------------------------------------------------------
def test_odd_factor_hits_the_lattice_pixels_bit_for_bit(case2):
    """k = 3: output pixel 3i + 1 has lattice pixel i's coordinate exactly, and a row's arithmetic depends on no other row of its tile
    or band (nine bands here, the lattice pixels spread over all of them)."""
    h, g, v, two, _ = case2
    for f in _frames(v):
        want, _ = h.render_frame(f)
        got = h.render_frame_at(f, 3 * v.resy, 3 * v.resx)
        sub = np.ascontiguousarray(got[1::3, 1::3])
        assert sub.shape == want.shape and np.array_equal(sub.view(np.uint32), want.view(np.uint32)), (f, np.abs(sub - want).max())


# ---- 3. oracle ---------------------------------------------------------------------------------------------------------------------
def test_matches_the_oracle_at_the_restated_coordinates(case):
    """Every pixel no further from the fp64 twin of the oracle's models (on the unrounded positions) than max(2e-6, 2 e_ref), e_ref the
    oracle's own fp32 render against that twin on the same grid: the rule of test_render_matches_oracle_per_pixel."""
    h, g, v, two, models = case
    twins = R.fp64_twin(models)
    for oh, ow in SIZES:
        for f in _frames(v):
            want, want64 = R.render_pair(models, twins, v.resx, v.resy, oh, ow, f, v.F)
            got = h.render_frame_at(f, oh, ow)
            assert got.shape == (oh, ow, 3)
            d, e_ref, e_hip = float(np.abs(got - want).max()), float(np.abs(want - want64).max()), float(np.abs(got - want64).max())
            print("%dx%d frame %d: vs fp32 oracle %.3g, oracle vs twin %.3g, hip vs twin %.3g" % (ow, oh, f, d, e_ref, e_hip))
            assert e_hip <= max(2e-6, 2.0 * e_ref), (oh, ow, f, d, e_hip, e_ref)


def test_border_pixels_are_clamped_to_the_lattice(case2):
    """Up-scaling by 3, the first output column sits at -1/3 of a lattice pixel and is clamped to 0, where the second one lies exactly:
    the two render bit-equal, and so do the last two columns and the first / last two lines; by 41x67 the first column is clamped and
    equals the render at the clamped coordinate, i.e. column 0 of a grid whose column 0 needs no clamp."""
    h, g, v, two, _ = case2
    f = v.F // 2
    got = h.render_frame_at(f, 3 * v.resy, 3 * v.resx).view(np.uint32)
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, -1], got[:, -2])
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[-1], got[-2])
    assert not np.array_equal(got[:, 1], got[:, 2])
    assert (R.source_positions(v.resx, 67)[[0, -1]] == [0.0, v.resx - 1.0]).all() and (R.source_positions(v.resy, 41)[[0, -1]] == [0.0, v.resy - 1.0]).all()
    ragged = h.render_frame_at(f, 41, 67).view(np.uint32)
    lattice = h.render_frame(f)[0].view(np.uint32)
    for yy, xx in ((0, 0), (0, -1), (-1, 0), (-1, -1)):     # the clamped corners are the lattice's corner pixels
        assert np.array_equal(ragged[yy, xx], lattice[yy, xx])


# ---- 4. plumbing -------------------------------------------------------------------------------------------------------------------
def test_device_pointers_u8_cast_and_repeat(case2):
    h, g, v, two, _ = case2
    f, oh, ow = v.F - 1, 41, 67
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 256, (oh, ow, 3), dtype=np.uint8)
    rgb, u8, sse = h.render_frame_at_u8(f, oh, ow, ref=ref)
    assert np.array_equal(u8, (rgb.astype(np.float64) * 255).astype(np.uint8))
    host = float(((ref.astype(np.float64) / 255.0 - rgb.astype(np.float64)) ** 2).sum())
    assert abs(sse - host) <= 1e-12 * host, (sse, host)
    d_rgb, d_u8, d_sse = h.render_frame_at_device(f, oh, ow, ref=torch.from_numpy(ref).cuda())
    assert np.array_equal(d_rgb.cpu().numpy().view(np.uint32), rgb.view(np.uint32)) and np.array_equal(d_u8.cpu().numpy(), u8) and d_sse == sse
    rgb2, u82, sse2 = h.render_frame_at_u8(f, oh, ow, ref=ref)
    assert np.array_equal(rgb2.view(np.uint32), rgb.view(np.uint32)) and np.array_equal(u82, u8) and sse2 == sse
    only_u8 = h.render_frame_at_device(f, oh, ow, want_float=False, want_u8=True)
    assert only_u8[0] is None and only_u8[2] is None and np.array_equal(only_u8[1].cpu().numpy(), u8)
    only_sse = h.render_frame_at_device(f, oh, ow, want_float=False, want_u8=False, ref=torch.from_numpy(ref).cuda())
    assert only_sse[0] is None and only_sse[1] is None and only_sse[2] == sse


def test_every_mlp_mode(case2):
    """The lattice call and the any-size call at (resy, resx) are one kernel on two host routes: the same bits in every mode."""
    h, g, v, two, _ = case2
    f, start = 1, h.arithmetic["mlp_mode"]
    try:
        for mode in (0, 1, 2, 3):
            h.set_mlp_mode(mode)
            want, _ = h.render_frame(f)
            assert np.array_equal(h.render_frame_at(f, v.resy, v.resx).view(np.uint32), want.view(np.uint32)), mode
            got = h.render_frame_at(f, 3 * v.resy, 3 * v.resx)
            assert np.array_equal(np.ascontiguousarray(got[1::3, 1::3]).view(np.uint32), want.view(np.uint32)), mode
    finally:
        h.set_mlp_mode(start)


@pytest.mark.parametrize("name", ["single", "seg"])
def test_forward_only(name, handles):
    """af_psnr and a following train_steps trajectory are bitwise what they are without the call in between."""
    _, g, v, two, models = handles[name]
    inds = g["inds"][:3].astype(np.int64)
    runs = []
    for with_calls in (False, True):
        h = _handle(g, v, two, models)
        try:
            if with_calls:
                h.render_frame_at(0, 41, 67, ref=np.zeros((41, 67, 3), np.uint8))      # before af_psnr has cached anything
            mean, per = h.psnr()
            if with_calls:
                h.render_frame_at(2, 72, 120)
            l1 = h.train_steps(0, 2, inds[:2])
            if with_calls:
                h.render_frame_at_device(1, 12, 20, ref=torch.zeros((12, 20, 3), dtype=torch.uint8, device="cuda"))
            l2 = h.train_steps(2, 1, inds[2:])
            params = [h.get_params_flat(n) for n in _nets(two)]
            adam = [h.adam_state(n) for n in _nets(two)]
            runs.append((mean, per, l1, l2, params, adam, h.psnr()[1]))
        finally:
            h.close()
    a, b = runs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[6], b[6])
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
    for p, q in zip(a[4], b[4]):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
    for (m0, v0, s0), (m1, v1, s1) in zip(a[5], b[5]):
        assert s0 == s1 and np.array_equal(m0.view(np.uint32), m1.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))


@pytest.mark.parametrize("name", ["single", "seg"])
def test_needs_no_video(name, handles):
    ref_h, g, v, two, models = handles[name]
    h = _handle(g, v, two, models, upload=False)
    try:
        got, sse = h.render_frame_at(2, 41, 67, ref=np.full((41, 67, 3), 7, np.uint8))
        assert np.array_equal(got.view(np.uint32), ref_h.render_frame_at(2, 41, 67).view(np.uint32)) and sse > 0
    finally:
        h.close()


def test_invalid_arguments(handles):
    import aiod_amd
    h = handles["single"][0]
    F, lib = h.cfg.number_of_frames, h.lib
    rgb = np.zeros((4, 4, 3), np.float32); u8 = np.zeros((4, 4, 3), np.uint8); sse = C.c_double(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    bad = [((F, 4, 4, p(rgb), None, None, None), "frame index"), ((-1, 4, 4, p(rgb), None, None, None), "frame index"),
           ((0, 0, 4, p(rgb), None, None, None), "oh and ow must be 1..16384"), ((0, 4, 16385, p(rgb), None, None, None), "oh and ow must be 1..16384"),
           ((0, 4, 4, None, None, None, None), "all NULL"),
           ((0, 4, 4, p(rgb), None, None, C.byref(sse)), "sse_out needs ref_u8"),
           ((0, 4, 4, p(rgb), None, p(u8), None), "ref_u8 needs sse_out")]
    for args, msg in bad:
        rc = lib.af_render_frame_at(h.h, *args, 0)
        assert rc == -1 and msg in lib.af_last_error(h.h).decode(), (args[:3], rc, lib.af_last_error(h.h))
    with pytest.raises(aiod_amd.AtlasFitError, match="frame index"):
        h.render_frame_at(F, 4, 4)
    with pytest.raises(ValueError, match="ref must be uint8"):
        h.render_frame_at(0, 4, 4, ref=np.zeros((4, 5, 3), np.uint8))
    assert h.render_frame_at(0, 1, 1).shape == (1, 1, 3)


# ---- 5. the pipeline ---------------------------------------------------------------------------------------------------------------
# Patterned on tests/test_gpu_deflicker.py: its clip size, its synthetic weights, its short config; every comparison exact, for the
# reasons given there (same kernels on the same values, fixed-order reductions, lossless files).
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import pipeline_bench as PB  # noqa: E402

H, W, DOWN, SEED = 130, 197, 4, 11
SHORT = {"samples_batch": 1024, "iters_num": 31, "evaluate_every": 30, "pretrain_iter_number": 3, "stop_global_rigidity": 15}


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(cmd, cwd):
    import subprocess
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(str(c) for c in cmd) + "\n" + r.stdout[-2000:] + r.stderr[-3000:]


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    import json
    from aiod_amd.atlasfit import REFERENCE_CONFIG
    d = tmp_path_factory.mktemp("render_at_assets")
    weights = PB.synthetic_weights()
    paths = PB.write_weights(str(d / "weights"), weights)
    cfgs = {}
    for name, extra in (("short", {}), ("win5", {"maximum_number_of_frames": 5})):
        cfgs[name] = dict(REFERENCE_CONFIG, **SHORT, **extra)
        with open(d / (name + ".json"), "w") as f:
            json.dump(cfgs[name], f)
    return {"weights": weights, "paths": paths, "cfg": cfgs, "cfg_path": {k: str(d / (k + ".json")) for k in cfgs},
            "frames": PB.synthetic_clip(9, H, W, seed=5)}


def test_full_size_styles_in_process_and_chained(assets, tmp_path):
    """deflicker.py --style_size full against preprocess_optical_flow.py -> stage1.py --style_size full -> neural_filter.py, and the
    kept styles against render_frame_at of the chained route's own fit (its checkpoint, written at the evaluation that rendered them)."""
    import json
    import aiod_amd
    from aiod_amd import stage1 as S
    n = 4
    frames = assets["frames"][:n]
    roots = {arm: tmp_path / arm for arm in ("in_process", "chained")}
    for r in roots.values():
        PB.write_clip(str(r / "data" / "test" / "clip"), frames)
    out = roots["in_process"] / "anywhere" / "clip"
    _run(PB.in_process_command(str(roots["in_process"] / "data" / "test" / "clip"), str(out), assets["cfg_path"]["short"], DOWN, SEED, assets["paths"],
                               extra=["--keep_intermediates", "--style_size", "full"]), tmp_path)
    for name, cmd in PB.chained_commands("clip", assets["cfg_path"]["short"], DOWN, SEED, assets["paths"]):
        _run(cmd + (["--style_size", "full"] if name == "stage 1" else []), roots["chained"])
    ref = roots["chained"] / "results" / "clip"
    names = ["%05d.png" % i for i in range(n)]
    for sub in (("stage_1", "output"), ("neural_filter", "output"), ("final", "output")):
        a, b = out.joinpath(*sub), ref.joinpath(*sub)
        assert sorted(os.listdir(a)) == names == sorted(os.listdir(b)), sub
        for fn in names:
            x, y = _png(a / fn), _png(b / fn)
            assert x.dtype == np.uint8 and x.shape == y.shape == (H, W, 3) and np.array_equal(x, y), "%s/%s differs in %d values" % ("/".join(sub), fn, int((x != y).sum()))
    rec = json.load(open(out / "deflicker.json"))
    assert rec["style_size"] == "full" and len(rec["psnr_full"]) == 1 and np.isfinite(rec["psnr_full"][0]) and len(rec["psnr"]) == 1
    assert [m for m in os.listdir(ref / "stage_1" / "000030") if m.startswith("PSNR_")] == ["PSNR_%f" % rec["psnr"][0]]      # the stage-1-size figure
    assert json.load(open(ref / "stage_1" / "config.json"))["style_size"] == "full"
    # the stand-alone fit with this seed, from its checkpoint: the styles are its render_frame_at, and psnr_full is its error against the frames
    af = aiod_amd.AtlasFit(aiod_amd.default_config(W // DOWN, H // DOWN, n, assets["cfg"]["short"]))
    try:
        assert S.load_checkpoint(af, ref / "stage_1" / "checkpoint") == 30
        full = []
        for f in range(n):
            _, u8, sse = af.render_frame_at_u8(f, H, W, want_float=False, ref=frames[f])
            assert np.array_equal(u8, _png(out / "stage_1" / "output" / names[f])), f
            full.append(S.frame_psnr(sse, H * W * 3))
        assert rec["psnr_full"] == [float(np.mean(full))]
    finally:
        af.close()


def test_full_size_cross_fade_and_default_bytes(assets, tmp_path):
    import aiod_amd
    from aiod_amd import deflicker

    def run(lo, hi, cfg="short", seed=SEED, overlap=0, **kw):
        d = aiod_amd.Deflicker(*assets["weights"], config=assets["cfg"][cfg], down=DOWN, seed=seed, window_overlap=overlap, **kw)
        return d.run(assets["frames"][lo:hi], keep=("final", "stage1", "renders"))
    r = run(0, 9, cfg="win5", overlap=1, style_size="full")
    assert r["windows"] == [(0, 5), (4, 9)] and r["style_size"] == "full" and len(r["psnr_full"]) == 2
    first, second = run(0, 5, style_size="full"), run(4, 9, seed=SEED + 1, style_size="full")
    ra, rb = r["renders"]
    assert ra.shape == rb.shape == (5, H, W, 3) and ra.dtype == np.float32
    assert np.array_equal(ra, first["renders"][0]) and np.array_equal(rb, second["renders"][0])
    a, b = ra[4], rb[0]                                                     # frame 4 in both windows
    blend = torch.lerp(torch.from_numpy(a), torch.from_numpy(b), 0.5).numpy()
    assert np.array_equal(r["stage1"][4], (blend.astype(np.float64) * 255).astype(np.uint8))
    assert not np.array_equal(r["stage1"][4], first["stage1"][4]) and not np.array_equal(r["stage1"][4], second["stage1"][0])
    assert np.array_equal(r["stage1"][0:4], first["stage1"][0:4]) and np.array_equal(r["stage1"][5:9], second["stage1"][1:5])
    assert r["psnr_full"] == [first["psnr_full"][0], second["psnr_full"][0]] and r["psnr"] == [first["psnr"][0], second["psnr"][0]]
    # --style_size stage1 is a run without the flag, byte for byte
    PB.write_clip(str(tmp_path / "clip"), assets["frames"][:3])
    argv = ["--frames_dir", str(tmp_path / "clip"), "--config", assets["cfg_path"]["short"], "--seed", str(SEED), "--down", str(DOWN), "--keep_intermediates",
            "--model", assets["paths"][0], "--ckpt_filter", assets["paths"][1], "--ckpt_local", assets["paths"][2]]
    assert deflicker.main(argv + ["--out", str(tmp_path / "plain")]) == 0
    assert deflicker.main(argv + ["--out", str(tmp_path / "flag"), "--style_size", "stage1"]) == 0
    for sub in (("stage_1", "output"), ("neural_filter", "output"), ("neural_filter", "concat"), ("final", "output")):
        for i in range(3):
            fn = "%05d.png" % i
            assert tmp_path.joinpath("plain", *sub, fn).read_bytes() == tmp_path.joinpath("flag", *sub, fn).read_bytes(), (sub, fn)
    assert _png(tmp_path / "flag" / "stage_1" / "output" / "00000.png").shape == (H // DOWN, W // DOWN, 3)
