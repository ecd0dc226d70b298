"""CPU tests: the oracle restatement against the golden fixtures that oracle/make_golden.py produced by
running the reference's own modules."""
import os

import numpy as np
import pytest
import torch

from oracle import atlas_oracle as O

FIXTURE_THREADS = 8      # intra-op threads oracle/make_golden*.py ran with: MKL's fp32 summation order, and so the last bits, follow the thread count


@pytest.fixture(autouse=True, scope="module")
def _fixture_thread_count():
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    yield
    torch.set_num_threads(n)


def _load_flat(model, flat):
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            n = p.numel(); p.copy_(torch.from_numpy(flat[off:off + n].reshape(p.shape))); off += n


def test_init_and_forward_match_reference_fixture(golden):
    m, a = O.build_single_atlas_models(golden["config"], seed=int(golden["weight_seed"]))
    assert abs(float(np.abs(O.flat_params(m)).sum()) - float(golden["init_checksum"][0])) < 1e-3
    assert abs(float(np.abs(O.flat_params(a)).sum()) - float(golden["init_checksum"][1])) < 1e-3
    with torch.no_grad():
        assert np.abs(m(torch.from_numpy(golden["rows_xyt"])).numpy() - golden["fwd_map"]).max() < 1e-6
        assert np.abs(a(torch.from_numpy(golden["rows_uv"])).numpy() - golden["fwd_atlas"]).max() < 1e-6


def test_pe_layout():
    x = torch.tensor([[0.25, -0.5]])
    b = torch.tensor([(2 ** j) * np.pi for j in range(3)])
    pe = O.positional_encoding(x, b)[0]
    exp = []
    for k in range(3):
        exp += [np.sin(0.25 * float(b[k])), np.sin(-0.5 * float(b[k])), np.cos(0.25 * float(b[k])), np.cos(-0.5 * float(b[k]))]
    assert np.allclose(pe.numpy(), np.array(exp, np.float32), atol=1e-6)


@pytest.mark.parametrize("flow", ["constant", "field"])
def test_trajectory_matches_reference_fixture(flow, request):
    golden, small_video = (request.getfixturevalue(n + ("" if flow == "constant" else "_field")) for n in ("golden", "small_video"))
    m, a = O.build_single_atlas_models(golden["config"], seed=int(golden["weight_seed"]))
    _load_flat(m, golden["start_map"]); _load_flat(a, golden["start_atlas"])
    tr = O.SingleAtlasTrainer(golden["config"], small_video, mapping=m, atlas=a)
    inds = torch.from_numpy(golden["inds"].astype(np.int64))
    for i in range(inds.shape[0]):
        t = tr.step(i, inds[i])
        got = np.array([t[k] for k in ("rgb", "gradient", "rigidity", "global_rigidity", "flow", "total")])
        assert np.allclose(got, golden["losses"][i], rtol=1e-4, atol=1e-7), (i, got, golden["losses"][i])
    assert np.abs(O.flat_params(m)[::97] - golden["end_map_sample"]).max() < 1e-5
    mean, _ = O.mean_psnr(m, a, small_video)
    assert abs(mean - float(golden["psnr"])) < 1e-3


def test_pretrain_matches_reference_fixture(golden):
    m, _ = O.build_single_atlas_models(golden["config"], seed=int(golden["weight_seed"]))
    ys = torch.from_numpy(golden["pre_ys"].astype(np.int64)); xs = torch.from_numpy(golden["pre_xs"].astype(np.int64))
    L = max(int(golden["resx"]), int(golden["resy"]))
    losses = O.pre_train_mapping(m, int(golden["nframes"]), golden["config"]["uv_mapping_scale"], int(golden["resx"]),
                                 int(golden["resy"]), np.int64(L), 2, ys, xs, batch=int(golden["pre_batch"]))
    assert np.allclose(losses, golden["pre_losses"], rtol=1e-5)


def test_empty_flow_set_is_nan_like_the_reference(golden, small_video):
    """loss_utils.py:317-320: a batch without valid flow pixels gives mean(empty) = NaN."""
    v = small_video
    m, a = O.build_single_atlas_models(golden["config"], seed=1)
    tr = O.SingleAtlasTrainer(golden["config"], v, mapping=m, atlas=a)
    # last frame has no forward flow, so pick samples only there AND zero the reverse mask
    v2 = O.Video(v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, torch.zeros_like(v.optical_flows_reverse_mask))
    tr.video = v2
    p2 = v.resx * v.resy
    inds = torch.arange(64) + (v.F - 1) * p2
    t = tr.loss_and_grads(0, inds)
    assert np.isnan(t["flow"])


def test_field_video_has_a_per_pixel_flow_that_moves_its_texture():
    """The `flow="field"` videos (round 4): no two flow vectors of a frame are equal, fields differ from frame
    to frame, the masks are the reference's consistency rule applied to the fields (unwrap_utils.py:10-23,151-159) and have holes away
    from the border, and the flow really is the motion of the texture (without flicker: frame f+1 sampled at p + flow(p) == frame f)."""
    v = O.synthetic_video(96, 54, 7, seed=5, flow="field", flicker=False)
    fl, fr = v.optical_flows.numpy()[..., 0], v.optical_flows_reverse.numpy()[..., 0]
    mk, mr = v.optical_flows_mask.numpy()[..., 0], v.optical_flows_reverse_mask.numpy()[..., 0]
    assert not fl[:, :, :, -1].any() and not fr[:, :, :, 0].any() and not mk[:, :, -1].any() and not mr[:, :, 0].any()      # unwrap_utils.py:135-159
    yy, xx = np.mgrid[0:54, 0:96].astype(np.float32)
    for f in range(6):
        for comp in (0, 1):
            assert np.unique(fl[:, :, comp, f]).size > 0.98 * 96 * 54
        assert np.abs(fl[:, :, :, f] - fl[:, :, :, (f + 1) % 6]).mean() > 0.05
        assert np.array_equal(mk[:, :, f] > 0, O.compute_consistency(fl[:, :, :, f], fr[:, :, :, f + 1]) < 1.0)
        assert np.array_equal(mr[:, :, f + 1] > 0, O.compute_consistency(fr[:, :, :, f + 1], fl[:, :, :, f]) < 1.0)
        inner = mk[8:-8, 12:-12, f]
        assert 0.5 < inner.mean() < 0.999                                        # holes inside the frame, not only border strips
        warped = O.remap_bilinear_zero(v.video_frames[:, :, :, f + 1].numpy(), xx + fl[:, :, 0, f], yy + fl[:, :, 1, f])
        err = np.abs(warped - v.video_frames[:, :, :, f].numpy())[mk[:, :, f] > 0]
        assert np.median(err) < 2e-3 and err.mean() < np.abs((v.video_frames[:, :, :, f + 1] - v.video_frames[:, :, :, f]).numpy()).mean()
    # the device generator of bench.py builds the same kind of video from torch's generator (its own draws)
    import bench
    frames, flows, flows_rev, mask, mask_rev = bench.synth_video_device(64, 36, 4, 9, torch.device("cpu"), flow="field", flicker=False)
    yy, xx = np.mgrid[0:36, 0:64].astype(np.float32)
    for f in range(3):
        assert np.array_equal(mask[:, :, f].numpy() > 0, O.compute_consistency(flows[:, :, :, f].numpy(), flows_rev[:, :, :, f + 1].numpy()) < 1.0)
        warped = O.remap_bilinear_zero(frames[:, :, :, f + 1].numpy(), xx + flows[:, :, 0, f].numpy(), yy + flows[:, :, 1, f].numpy())
        assert np.median(np.abs(warped - frames[:, :, :, f].numpy())[mask[:, :, f].numpy() > 0]) < 5e-3
        warped = O.remap_bilinear_zero(frames[:, :, :, f].numpy(), xx + flows_rev[:, :, 0, f + 1].numpy(), yy + flows_rev[:, :, 1, f + 1].numpy())
        assert np.median(np.abs(warped - frames[:, :, :, f + 1].numpy())[mask_rev[:, :, f + 1].numpy() > 0]) < 5e-3


@pytest.mark.parametrize("flow", ["constant", "field"])
def test_restatement_against_reference_vectors(flow, request):
    """What oracle/make_golden.py asserts while it runs the reference's own modules, replayed on the vectors it stored: the reference's
    pre-train (its own torch.randint order, 10 000 rows per step) ends within 1e-7 of single_small_start.npz, from which the ten loop iterations track the
    reference's losses to 2e-5 and its end parameters of both nets to 2e-6, and the portrait-aspect iterations (resy > resx: the gradient
    loss normalises by resx, everything else by larger_dim) give the reference's terms with and without the global-rigidity term."""
    golden = request.getfixturevalue("golden" if flow == "constant" else "golden_field")
    video = request.getfixturevalue("small_video" if flow == "constant" else "small_video_field")
    c, wseed, nf = golden["config"], int(golden["weight_seed"]), int(golden["nframes"])
    resx, resy = int(golden["resx"]), int(golden["resy"])
    terms = ("rgb", "gradient", "rigidity", "global_rigidity", "flow", "total")
    m, a = O.build_single_atlas_models(c, seed=wseed)
    torch.manual_seed(wseed + 1)
    O.pre_train_mapping(m, nf, c["uv_mapping_scale"], resx, resy, video.larger_dim, 1)
    assert np.abs(O.flat_params(m) - golden["start_map"]).max() <= 1e-7       # the stored state: the reference's pre-train
    assert np.array_equal(O.flat_params(a), golden["start_atlas"])
    _load_flat(m, golden["start_map"])                                         # the loop starts from it (oracle/make_golden.py)
    tr = O.SingleAtlasTrainer(c, video, mapping=m, atlas=a)
    inds = torch.from_numpy(golden["inds"].astype(np.int64))
    for i in range(inds.shape[0]):
        t = tr.step(i, inds[i])
        got = np.array([t[k] for k in terms])
        assert np.allclose(got, golden["losses"][i], rtol=2e-5, atol=1e-7), (i, got, golden["losses"][i])
    assert np.abs(O.flat_params(m)[::97] - golden["end_map_sample"]).max() < 2e-6
    assert np.abs(O.flat_params(a)[::97] - golden["end_atlas_sample"]).max() < 2e-6
    pv = O.synthetic_video(24, 40, 5, seed=int(golden["video_seed"]) + 1, flow=flow)
    pm, pa = O.build_single_atlas_models(c, seed=wseed + 7)
    ptr = O.SingleAtlasTrainer(c, pv, mapping=pm, atlas=pa)
    pg = torch.Generator().manual_seed(5)
    for k, it in enumerate((0, golden["inds"].shape[0] + 1)):
        pinds = torch.randint(5 * 40 * 24, (int(c["samples_batch"]),), generator=pg)
        t = ptr.loss_and_grads(it, pinds)
        got = np.array([t[j] for j in terms])
        assert np.allclose(got, golden["portrait_losses"][k], rtol=2e-5, atol=1e-7), (it, got, golden["portrait_losses"][k])


# ---- fg/bg dual-atlas path (src/stage1_neural_atlas_seg.py)
def test_seg_init_and_forward_match_reference_fixture(golden_seg):
    ms = O.build_seg_models(golden_seg["config"], seed=int(golden_seg["weight_seed"]))
    for m, ref in zip(ms, golden_seg["init_checksum"]):
        assert abs(float(np.abs(O.flat_params(m)).sum()) - float(ref)) < 1e-3
    rows = torch.from_numpy(golden_seg["rows_xyt"])
    with torch.no_grad():
        assert np.abs(ms[1](rows).numpy() - golden_seg["fwd_map2"]).max() < 1e-6
        assert np.abs(ms[3](rows).numpy() - golden_seg["fwd_alpha"]).max() < 1e-6


def test_alpha_pe_layout():
    """in_dim 3: feature index = 6k + [sin x0,x1,x2, cos x0,x1,x2] (implicit_neural_networks.py:9-13)."""
    x = torch.tensor([[0.25, -0.5, 0.125]])
    b = torch.tensor([(2 ** j) * np.pi for j in range(2)])
    pe = O.positional_encoding(x, b)[0].numpy()
    exp = []
    for k in range(2):
        exp += [np.sin(v * float(b[k])) for v in (0.25, -0.5, 0.125)] + [np.cos(v * float(b[k])) for v in (0.25, -0.5, 0.125)]
    assert np.allclose(pe, np.array(exp, np.float32), atol=1e-6)


@pytest.mark.parametrize("flow", ["constant", "field"])
def test_seg_trajectory_matches_reference_fixture(flow, request):
    golden_seg, small_seg_video = (request.getfixturevalue(n + ("" if flow == "constant" else "_field")) for n in ("golden_seg", "small_seg_video"))
    from conftest import seg_start_models
    tr = O.SegAtlasTrainer(golden_seg["config"], small_seg_video, models=seg_start_models(golden_seg))
    assert abs(float(np.abs(O.flat_params(tr.m1)).sum()) - float(golden_seg["start_m1_sum"])) < 1e-3
    assert 2.5 < float(golden_seg["losses"][0][2]) < 5.0 and 2.5 < float(golden_seg["losses"][0][3]) < 5.0    # pre-trained: J ~ identity
    inds = torch.from_numpy(golden_seg["inds"].astype(np.int64))
    for i in range(inds.shape[0]):
        t = tr.step(i, inds[i])
        got = np.array([t[k] for k in O.SEG_TERMS])
        assert np.allclose(got, golden_seg["losses"][i], rtol=2e-4, atol=1e-7), (i, got, golden_seg["losses"][i])
    ends = np.concatenate([O.flat_params(m)[::97] for m in (tr.m1, tr.m2, tr.atlas, tr.alpha)])
    assert np.abs(ends - golden_seg["end_samples"]).max() < 1e-5
    mean, _ = O.mean_psnr_seg(tr.m1, tr.m2, tr.atlas, tr.alpha, small_seg_video)
    assert abs(mean - float(golden_seg["psnr"])) < 1e-3


def test_oracle_imlp_matches_reference_fixture_for_every_architecture():
    """tests/golden/arch_variants.npz (oracle/make_golden_arch.py: forward outputs of the REFERENCE's IMLP for 2..8 layers per net
    kind, mapping nets with positional encoding, smaller encodings): the restatement rebuilt from the seed reproduces them bit for
    bit — the CPU pin of the oracle for the architectures tests/test_gpu_arch.py holds the HIP chains against."""
    import os
    import torch
    from oracle import atlas_oracle as O
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arch_variants.npz")))
    assert len(g["variants"]) >= 27

    def kind_args(kind):       # (input_dim, output_dim, use_positional, positional_dim, skip_layers): the constructor calls of the two stage-1 scripts
        if kind.startswith("mappingpe"):
            return 3, 2, True, int(kind[len("mappingpe"):]), []
        if kind.startswith("atlaspe"):
            return 2, 3, True, int(kind[len("atlaspe"):]), [4, 7]
        if kind.startswith("alphape"):
            return 3, 1, True, int(kind[len("alphape"):]), []
        return {"mapping": (3, 2, False, 4, []), "atlas": (2, 3, True, 10, [4, 7]), "alpha": (3, 1, True, 5, [])}[kind]
    for name in [str(v) for v in g["variants"]]:
        kind, nl = name.split("_")[0], int(name.split("_")[1])
        ind, outd, pos, pdim, skips = kind_args(kind)
        torch.manual_seed(int(g[name + "_seed"]))
        m = O.OracleIMLP(ind, outd, 256, pos, pdim, skips, nl)
        assert sum(p.numel() for p in m.parameters()) == int(g[name + "_nparams"]), name
        with torch.no_grad():
            y = m(torch.from_numpy(g[name + "_rows"])).numpy()
        assert np.array_equal(y, g[name + "_out"]), name


def test_complete_schedule_fixtures_describe_the_videos_the_gpu_tests_rebuild():
    """The configs[0] / configs[4] acceptance fixtures store only results; the GPU tests rebuild the seeded videos and replay the
    draws.  Here (CPU): the videos the oracle's generators build for the fixtures' seeds have the checksums the reference runs
    recorded, every run reached a plausible fit, and the configs[4] fixture holds every seed at two thread counts."""
    import os
    from oracle import atlas_oracle as O
    gd = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for fn in ("c1_reference.npz", "c1_reference_more.npz"):
        g = dict(np.load(os.path.join(gd, fn)))
        for k, s in enumerate(g["seeds"]):
            flow = str(g["flow_kind"][k]) if "flow_kind" in g else "constant"
            v = O.synthetic_video(int(g["resx"]), int(g["resy"]), int(g["nframes"]), seed=int(s), flow=flow)
            assert abs(float(v.video_frames.double().sum()) - float(g["video_checksum"][k])) < 1e-6, (fn, int(s))
        # the field videos carry flow-estimate errors the fit cannot remove: their total loss ends at ~0.25 of its start, not ~0.08
        assert (g["psnr"] > g["psnr_pre"] + 5.0).all() and (g["curves"][:, -1, 5] < 0.35 * g["curves"][:, 0, 5]).all()
    g = dict(np.load(os.path.join(gd, "c1_seg_reference.npz")))
    seeds = sorted({int(s) for s in g["seeds"]})
    assert len(seeds) >= 3
    pairs = 0
    for s in seeds:
        runs = [i for i in range(len(g["seeds"])) if int(g["seeds"][i]) == s and int(g["double"][i]) == 0]
        pairs += len({int(g["threads"][i]) for i in runs}) >= 2
        flow = str(g["flow_kind"][runs[0]]) if "flow_kind" in g else "constant"
        v = O.synthetic_seg_video(int(g["resx"]), int(g["resy"]), int(g["nframes"]), seed=s, flow=flow)
        for i in runs:
            assert abs(float(v.video_frames.double().sum()) - float(g["video_checksum"][i])) < 1e-6
            assert abs(float(v.mask_frames.double().sum()) - float(g["mask_checksum"][i])) < 1e-6
            assert g["psnr"][i] > g["psnr_pre"][i] + 3.0 and g["curves"][i][-1, 11] < 0.35 * g["curves"][i][0, 11]
    assert pairs >= 3          # the reference against itself (two thread counts) on at least three seeds: the tolerance construction needs pairs
    # configs[1] (round 5): the reference's complete 10 001-iteration schedule at 80 x 768x432.  The full-size videos are rebuilt and their checksums
    # compared in the GPU test (50 s of numpy each); here the records themselves: every seed fitted, the global-rigidity term is there for
    # iterations 0..5000 and gone afterwards (config_flow_100.json:44), the PSNR was taken at the switch as well
    f2 = os.path.join(gd, "c2_reference.npz")
    if os.path.exists(f2):
        g = dict(np.load(f2))
        assert (int(g["resx"]), int(g["resy"]), int(g["nframes"]), int(g["iters"])) == (768, 432, 80, 10001) and len(g["seeds"]) >= 3
        assert "field" in {str(k) for k in g["flow_kind"]} and "constant" in {str(k) for k in g["flow_kind"]}
        its = np.arange(g["curves"].shape[1]) * int(g["log_every"])
        assert ((g["curves"][:, :, 3] > 0) == (its <= 5000)[None, :]).all()
        assert 5000 in [int(i) for i in g["psnr_at_iter"]]
        assert (g["psnr"] > g["psnr_pre"] + 5.0).all() and (g["psnr"] >= g["psnr_at"][:, 0] - 0.5).all()
        assert (g["curves"][:, -1, 5] < 0.35 * g["curves"][:, 0, 5]).all()


def test_one_randint_call_replays_the_per_iteration_draws():
    """tests/test_gpu_c2.py replays a reference run's index draws (stage1_neural_atlas.py:159: torch.randint(P, (N, 1)) per iteration, global CPU
    generator) with ONE call per segment of the schedule: the same values in the same order, and the generator left in the same state."""
    P, N, K = 80 * 768 * 432, 10000, 7
    torch.manual_seed(11)
    per_iteration = torch.stack([torch.randint(P, (N, 1)).view(-1) for _ in range(K)])
    after_a = torch.randint(P, (5,))
    torch.manual_seed(11)
    one_call = torch.randint(P, (K * N, 1)).view(K, N)
    after_b = torch.randint(P, (5,))
    assert torch.equal(per_iteration, one_call) and torch.equal(after_a, after_b)
