"""tests/pretrain_ref.py against what it restates, without a GPU: the sampler against the published Philox4x32-10 vectors; the rows and the loss twin
against oracle.atlas_oracle.pre_train_mapping and torch autograd on injected draws; fp32 emulations of k_pre_loss (plain and contracted) inside the
bounds; seven one-line mutations outside them, by the printed factors; the mask layout of csrc/mlp16.hip against a packer written from the kernel's
loop.  And the conditions tests/test_gpu_pretrain_entries.py relies on, for the states and draws it uses: no sample undecided, the seed bounds bite."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pretrain_ref as PR  # noqa: E402
from oracle import atlas_oracle as O  # noqa: E402

U = PR.U
_models = {}


def _cfg(kind, golden, golden_seg):
    two, over, which, _ = PR.KINDS[kind]
    cfg = dict((golden_seg if two else golden)["config"]); cfg.update(over)
    return two, cfg, which


def _mapping(kind, golden, golden_seg):
    """The kind's pre-trained mapping net (fp32, the oracle's): seeded as tests/test_gpu_adam.start_state seeds it, PRETRAIN iterations at batch 500 on 5 frames."""
    if kind not in _models:
        two, cfg, which = _cfg(kind, golden, golden_seg)
        models = O.build_seg_models(cfg, seed=2) if two else O.build_single_atlas_models(cfg, seed=2)
        m = models[which - 1]
        torch.manual_seed(4 + which)
        O.pre_train_mapping(m, 5, cfg["uv_mapping_scale"], PR.RESX, PR.RESY, max(PR.RESX, PR.RESY), PR.PRETRAIN, batch=500)
        _models[kind] = (m, float(cfg["uv_mapping_scale"]))
    return _models[kind]


def _case(kind, NB, golden, golden_seg, F=1, f=0, seed=21, resx=PR.RESX, resy=PR.RESY):
    """(rows (NB, 4) fp32, the net's fp32 outputs on them (NB, 2), uv_scale, the net, ys, xs)."""
    m, s = _mapping(kind, golden, golden_seg)
    ys, xs = PR.draws(seed, F, NB, resx, resy)
    rows = PR.pre_prep_rows(ys[f], xs[f], resx, resy, F, f)
    with torch.no_grad():
        out = m(torch.from_numpy(rows[:, :3].copy())).numpy()
    return rows, out, s, m, ys, xs


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_reproduces_the_published_vectors(ctr, key, want):
    o = PR.philox4x32(np.array(ctr, np.uint64), np.array(key, np.uint64))
    assert " ".join("%08x" % int(x) for x in o) == want


def test_philox_is_vectorised_over_counters():
    ctr = np.array([k[0] for k in KAT], np.uint64); key = np.array([k[1] for k in KAT], np.uint64)
    o = PR.philox4x32(ctr, key)
    assert [" ".join("%08x" % int(x) for x in row) for row in o] == [k[2] for k in KAT]


@pytest.mark.parametrize("bound", [1, 21, 37, 2 ** 32 + 5])
def test_draws_lie_below_the_bound_and_fill_it(bound):
    n = 4000
    d = PR.rand_below(5, 3, n, 1, bound)
    assert d.dtype == np.int64 and d.min() >= 0 and d.max() < bound
    if bound == 1:
        assert not d.any()
        return
    # the draw is floor(r bound / 2^64), r uniform on 64 bits: mean (bound - 1) / 2 and variance (bound^2 - 1) / 12 to 2^-64; six standard errors
    assert abs(d.mean() - (bound - 1) / 2.0) <= 6.0 * np.sqrt((bound * bound - 1) / 12.0 / n), (bound, d.mean())
    if bound <= 37:
        assert np.unique(d).size == bound
    # the counter words and both key words reach the output
    same = lambda **kw: np.array_equal(d, PR.rand_below(**dict(dict(seed=5, it=3, n=n, stream=1, bound=bound), **kw)))      # noqa: E731
    assert same() and not same(seed=6) and not same(seed=5 + 2 ** 32) and not same(it=4) and not same(stream=2)
    assert np.array_equal(PR.rand_below(5, 3, n // 2, 1, bound), d[:n // 2])            # sample j depends on j alone


# ---- the twin against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,f", [(1, 0), (2, 1), (5, 3)])
@pytest.mark.parametrize("kind", ["S", "N"])
def test_rows_and_loss_equal_the_oracle_on_injected_draws(kind, F, f, golden, golden_seg):
    NB = 272
    rows, out, s, m, ys, xs = _case(kind, NB, golden, golden_seg, F=F, f=f)
    # rows: the reference's own expressions in torch float32 (unwrap_utils.py:183-189), bit for bit
    i_s, j_s = torch.from_numpy(ys[f]).view(-1, 1), torch.from_numpy(xs[f]).view(-1, 1)
    larger = max(PR.RESX, PR.RESY)
    yy, xx = i_s / (larger / 2) - 1, j_s / (larger / 2) - 1
    xyt = torch.cat((xx, yy, (f / (F / 2.0) - 1) * torch.ones_like(yy)), dim=1)
    assert xyt.dtype == torch.float32 and np.array_equal(xyt.numpy().view(np.uint32), rows[:, :3].view(np.uint32)) and not rows[:, 3].any()
    if F == 2:
        assert rows[0, 2] == 0.0
    tw = PR.pre_loss_ref(rows, out, s, NB)
    assert not tw.und.any()
    # loss and the gradient on the outputs: torch fp64 autograd of the reference's expression on the same fp32 inputs
    o64 = torch.from_numpy(out.astype(np.float64)).requires_grad_(True)
    loss = (torch.from_numpy(rows[:, :2].astype(np.float64)) * float(np.float32(s)) - o64).norm(dim=1).mean()
    g, = torch.autograd.grad(loss, o64)
    assert abs(float(loss.detach()) - tw.mean) <= 1e-13 * abs(tw.mean)
    assert np.allclose(g.numpy(), tw.d, rtol=1e-11, atol=0.0)
    # and the oracle's own step 0 of a one-frame run on the same draws (fp32: inside the record bound of the twin); F = 1 only, where step 0 is frame f
    if F == 1:
        losses = O.pre_train_mapping(copy.deepcopy(m), 1, s, PR.RESX, PR.RESY, larger, 1, ys=torch.from_numpy(ys), xs=torch.from_numpy(xs), batch=NB)
        print("%s: oracle fp32 loss %.9g, twin %.9g, error / bound %.4f" % (kind, losses[0], tw.mean, abs(losses[0] - tw.mean) / tw.mean_bound))
        assert abs(losses[0] - tw.mean) <= tw.mean_bound


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["S", "T2", "N", "P5"])
def test_fp32_emulations_of_the_loss_stay_inside_the_bound(kind, fused, golden, golden_seg):
    rows, out, s, _, _, _ = _case(kind, 500, golden, golden_seg)
    tw = PR.pre_loss_ref(rows, out, s, 500)
    l32, d32 = PR.pre_loss_f32(rows, out, s, 500, fused)
    ok = ~tw.und
    rd = np.abs(d32 - tw.d)[ok] / (PR.BOUND_FACTOR * tw.de[ok])
    rl = np.abs(l32 - tw.l)[ok] / (PR.BOUND_FACTOR * tw.le[ok])
    mean32 = float(np.float32(np.sum(l32.astype(np.float32), dtype=np.float32)) / np.float32(500))
    print("%s %s: seed error / bound rms %.4f worst %.4f; term worst %.4f; record error / bound %.4f" % (
        kind, "fma" if fused else "plain", np.sqrt((rd * rd).mean()), rd.max(), rl.max(), abs(mean32 - tw.mean) / tw.mean_bound))
    assert rd.max() <= 1.0 and rl.max() <= 1.0 and abs(mean32 - tw.mean) <= tw.mean_bound


def test_a_row_on_its_target_has_a_zero_seed_and_is_decided():
    """c s == o exactly (the zeroed output layer of the GPU test: o = tanh(0) = 0 at the row (0, 0, t)): l = 0 with error 0, seed exactly 0, not left out;
    a row one ulp off its target is undecided or decided, never a NaN."""
    rows = np.zeros((4, 4), np.float32); out = np.zeros((4, 4), np.float32)
    rows[1, :2] = (0.25, -0.5); out[1, :2] = np.float32(0.8) * rows[1, :2]           # not exact in general: a tiny e
    rows[2, :2] = (0.5, 0.5)
    tw = PR.pre_loss_ref(rows, out, 0.8, 4)
    assert tw.l[0] == 0 and not tw.d[0].any() and not tw.de[0].any() and not tw.und[0]
    assert np.isfinite(tw.d).all() and np.isfinite(tw.de).all() and np.isfinite(tw.mean_bound)
    assert not tw.und[2] and tw.l[2] > 0.5


# ---- mutations ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", PR.LOSS_MUTATIONS)
def test_loss_mutations_leave_the_bound(mut, golden, golden_seg):
    rows, out, s, _, _, _ = _case("S", 500, golden, golden_seg)
    tw, bad = PR.pre_loss_ref(rows, out, s, 500), PR.pre_loss_ref(rows, out, s, 500, mut=(mut,))
    r = np.abs(bad.d - tw.d) / (PR.BOUND_FACTOR * tw.de)
    print("mutation %-12s seed error / bound: median %.3g, least %.3g" % (mut, np.median(r), r.min()))
    assert np.median(r) > 100.0 and (r > 1.0).mean() > 0.95


@pytest.mark.parametrize("mut,resx,resy", [("x_y", PR.RESX, PR.RESY), ("half_resx", PR.RESY, PR.RESX)])
def test_row_mutations_break_the_equality_and_the_seeds(mut, resx, resy, golden, golden_seg):
    """half_main = resx / 2 is the same number on a landscape frame: that mutation shows on a portrait one (the seeded F = 3 case of the GPU test)."""
    ys, xs = PR.draws(22, 1, 500, resx, resy)
    rows = PR.pre_prep_rows(ys[0], xs[0], resx, resy, 1, 0)
    bad = PR.pre_prep_rows(ys[0], xs[0], resx, resy, 1, 0, mut=(mut,))
    differ = (rows.view(np.uint32) != bad.view(np.uint32)).any(1)
    m, s = _mapping("S", golden, golden_seg)
    with torch.no_grad():
        out = m(torch.from_numpy(bad[:, :3].copy())).numpy()               # the chain runs on the rows the (mutated) kernel wrote
    tw = PR.pre_loss_ref(rows, out, s, 500)
    got = PR.pre_loss_ref(bad, out, s, 500)
    r = np.abs(got.d - tw.d)[differ] / (PR.BOUND_FACTOR * tw.de[differ])
    print("mutation %-10s %d of 500 rows differ; seed error / bound on them: median %.3g" % (mut, differ.sum(), np.median(r)))
    assert differ.mean() > 0.9 and np.median(r) > 100.0
    if mut == "half_resx":
        assert np.array_equal(PR.pre_prep_rows(ys[0], xs[0], resy, resx, 1, 0, mut=(mut,)), PR.pre_prep_rows(ys[0], xs[0], resy, resx, 1, 0))


# ---- the mask layout ----------------------------------------------------------------------------------------------------------------------------
def pack16(acts):
    """relu_out of k_mlp16_fwd, as its loop runs: per lane (j, q) of a 16-row tile, for T, for r: mk[T >> 3] = alignbit(mk[T >> 3], bits of (0 - v), 31)
    = mk << 1 | sign(0 - v), v = acts[row j][16 T + 4 q + r].  acts (16 nt16, 256) -> (nt16 / 2, 64, 4) uint32 as af_debug_tiles returns a plane."""
    acts = np.asarray(acts, np.float32)
    nt16 = len(acts) // 16
    words = np.zeros((nt16, 64, 2), np.uint32)
    for t in range(nt16):
        for lane in range(64):
            j, q = lane & 15, lane >> 4
            mk = [0, 0]
            for T in range(16):
                for r in range(4):
                    v = np.float32(0.0) - acts[16 * t + j, 16 * T + 4 * q + r]
                    mk[T >> 3] = ((mk[T >> 3] << 1) | int(np.signbit(v))) & 0xFFFFFFFF
            words[t, lane] = mk
    return words.reshape(-1, 64, 4)


def test_mask_bits16_inverts_the_kernels_packer():
    rng = np.random.default_rng(3)
    acts = np.maximum(rng.standard_normal((64, 256)), 0.0).astype(np.float32)
    acts[:, 5] = 0.0; acts[17] = 0.0
    words = pack16(acts)
    assert words.shape == (2, 64, 4)
    assert np.array_equal(PR.mask_bits16(words), acts > 0)
    assert np.array_equal(PR.mask_bits16(words, 40), (acts > 0)[:40])
    for mut in PR.MASK_MUTATIONS:
        wrong = float((PR.mask_bits16(words, mut=(mut,)) != (acts > 0)).mean())
        print("mutation %-10s %.3f of the mask bits differ" % (mut, wrong))
        assert wrong > 0.3


# ---- the conditions the GPU test relies on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["S", "T2", "N", "P5"])
def test_no_sample_is_undecided_and_the_seed_bounds_bite(kind, golden, golden_seg):
    for NB in PR.BATCHES + ((PR.BIG_BATCH,) if kind == "S" else ()):
        rows, out, s, _, _, _ = _case(kind, NB, golden, golden_seg)
        tw = PR.pre_loss_ref(rows, out, s, NB)
        share = PR.loose_share(tw)
        print("%s batch %5d: %d samples undecided; loss %.4f, least l / its error %.3g; loose seed bounds %.4f" % (
            kind, NB, int(tw.und.sum()), tw.mean, float((tw.l / tw.le).min()), share))
        assert not tw.und.any() and share <= 0.05
