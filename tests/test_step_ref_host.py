"""tests/step_ref.py held to the reference, without a GPU.

  * prep_rows equals the oracle's batch construction exactly: oracle.loop_body / seg_loop_body run with nets that RECORD their input rows (get_tuples, the
    rigidity / gradient neighbours, flow_matches' torch.where compaction); every recorded row must be the twin's row, bit for bit, at the place k_prep puts it.
  * the twin's loss terms equal the oracle's in fp64 to 1e-12 and its seeds equal torch autograd of that loss written on LEAF output rows (nets that hand out
    slices of a leaf tensor): the twin is tied to the reference, not to a kernel.  Run with coeffs(exact=True): the reference's doubles.
  * a numpy-fp32 emulation of both loss kernels and of chain_dpe_to_uv, plain and with fused multiply-adds, stays inside 2 x the running error on every entry,
    and the bounds bite: at most 5 % of a class's entries with 2 bound > 2^-6 max(|ref|, median |ref|).
  * eleven one-line mutations each leave the bounds or break the equality.
States: kinds S, T, N of tests/test_gpu_adam.py on the 37x21x5 "field" video (seed 4), seeded nets with the mapping nets pre-trained 40 iterations by the
oracle (the narrow kind 640: PRETRAIN below), samples_batch 250 and 700, iterations 0 (nseg 9, global rigidity and bootstrapping on) and 10001 (nseg 7, both off); outputs from the oracle's nets."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_ref as SR  # noqa: E402
from oracle import atlas_oracle as O  # noqa: E402

NARROW = dict(number_of_channels_mapping1=40, number_of_layers_mapping1=3, use_positional_encoding_mapping1=True, number_of_positional_encoding_mapping1=3,
              number_of_channels_atlas=200, number_of_layers_atlas=6, positional_encoding_num_atlas=6)
KINDS = {"S": (False, {}), "T": (True, {}), "N": (False, NARROW)}
# Pre-train iterations of the mapping nets.  The narrow kind's PE mapping net is still far from the identity map after 40 (median rigidity seed 62 against
# 20 of kind S): (J^T J + eps)^-1 is badly conditioned on a tenth of its samples and 7-10 % of the centre-row bounds miss the 2^-6 condition — a property
# of that state, not of the bound, and the remedy the condition names is to pre-train longer: 3 % at 360 iterations, below 1 % at 680.
PRETRAIN = {"S": 40, "T": 40, "N": 640}
CASES = [(k, b, it) for k in "STN" for b in (250, 700) for it in (0, 10001)]
_models, _cases = {}, {}


def cfg_of(d, video, batch):
    ns = SimpleNamespace(**d)
    ns.resx, ns.resy, ns.number_of_frames, ns.samples_batch = int(video.resx), int(video.resy), int(video.F), batch
    return ns


def _state(kind, golden, golden_seg):
    """(config dict, video, models) of a kind: seeded nets, mapping nets pre-trained PRETRAIN iterations (batch 500, seeded draws)."""
    if kind not in _models:
        two, over = KINDS[kind]
        cfg = dict((golden_seg if two else golden)["config"]); cfg.update(over)
        video = (O.synthetic_seg_video if two else O.synthetic_video)(37, 21, 5, seed=4, flow="field")
        models = O.build_seg_models(cfg, seed=2) if two else O.build_single_atlas_models(cfg, seed=2)
        for i, m in enumerate(models[:2] if two else models[:1]):
            torch.manual_seed(5 + i)
            O.pre_train_mapping(m, video.F, cfg["uv_mapping_scale"], video.resx, video.resy, video.larger_dim, PRETRAIN[kind], batch=500)
        _models[kind] = (cfg, video, models)
    return _models[kind]


def _rows4(x):
    out = np.zeros((len(x), 4), np.float32); out[:, :x.shape[1]] = x
    return out


def case(kind, batch, it, golden, golden_seg):
    """Everything the checks need of one (kind, batch, iteration): rows, the oracle nets' fp32 outputs on them, the atlas net's dZ_0 / PE / W_0."""
    key = (kind, batch, it)
    if key in _cases:
        return _cases[key]
    cfgd, video, models = _state(kind, golden, golden_seg)
    two = KINDS[kind][0]
    cfg = cfg_of(cfgd, video, batch)
    inds = torch.randint(video.F * video.resx * video.resy, (batch,), generator=torch.Generator().manual_seed(12)).numpy()
    rec = SR.records_from_video(video, inds, two)
    R = SR.prep_rows(rec, inds, cfg, it, two)
    N = batch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))       # noqa: E731
    with torch.no_grad():
        if two:
            m1, m2, atlas, alpha = models
            o1, o2, oal = m1(t(R["map1"])).numpy(), m2(t(R["map2"])).numpy(), alpha(t(R["alpha"])).numpy()
            xin = torch.cat((t(o1[:3 * N]) * 0.5 + 0.5, t(o2[:3 * N]) * 0.5 - 0.5))
        else:
            m1, atlas = models
            o1 = m1(t(R["map1"])).numpy(); o2 = oal = None
            xin = t(o1[:3 * N]) * 0.5 + 0.5
    # the atlas net with its layer-0 pre-activation kept: dZ_0 of a seed is its gradient
    pe = O.positional_encoding(xin, atlas.b)
    z0 = atlas.hidden[0](pe); z0.retain_grad()
    x = z0
    for i, layer in enumerate(atlas.hidden[1:], 1):
        x = torch.relu(x)
        if i in atlas.skip_layers:
            x = torch.cat((x, pe.detach()), 1)
        x = layer(x)
    oat = torch.tanh(x)
    c = dict(kind=kind, two=two, cfg=cfg, cfgd=cfgd, video=video, inds=inds, rec=rec, R=R, N=N, it=it, o1=_rows4(o1), o2=None if o2 is None else _rows4(o2),
             oal=None if oal is None else _rows4(oal), oat=_rows4(oat.detach().numpy()), K=SR.coeffs(cfg, it, two), atlas_out=oat, z0=z0, pe=pe.detach().numpy(),
             W0=atlas.hidden[0].weight.detach().numpy())
    _cases[key] = c
    return c


def run(c, fn_single, fn_seg, K=None, **kw):
    K = c["K"] if K is None else K
    if c["two"]:
        return fn_seg(c["o1"], c["o2"], c["oal"], c["oat"], c["rec"], c["R"]["rank"], c["R"]["counts"], K, **kw)
    return fn_single(c["o1"], c["oat"], c["rec"], c["R"]["rank"], c["R"]["counts"], K, **kw)


def map_names(c):
    return ("dout_m1", "dout_m2") if c["two"] else ("dout_map",)


def dz0_of(c, atlas_seed):
    """dZ_0 of the atlas net (rows, hid) fp32 for the seed on its outputs."""
    c["z0"].grad = None
    c["atlas_out"].backward(torch.from_numpy(atlas_seed[:, :3].astype(np.float32)), retain_graph=True)
    return c["z0"].grad.numpy().copy()


# ---- the logf constant ---------------------------------------------------------------------------------------------------------------------------
def test_logf_constant_is_twice_the_measured_worst():
    rng = np.random.default_rng(0)
    x = rng.uniform(0.001, 0.999, 4_000_000).astype(np.float32)
    t = np.log(x.astype(np.float64))
    worst = float((np.abs(np.log(x).astype(np.float64) - t) / (SR.U * np.abs(t))).max())
    print("numpy-fp32 log against fp64 on [0.001, 0.999]: worst %.4f u of the result" % worst)
    assert 2.0 * worst <= SR.C_LOG * 1.0001 and worst > 0.25 * SR.C_LOG


# ---- rows ----------------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self, nout):
        self.nout, self.seen = nout, []

    def __call__(self, x):
        self.seen.append(x.detach().numpy().copy())
        return torch.zeros(x.shape[0], self.nout)


def oracle_rows(c):
    """{net: [input rows of every call]} of the oracle's loop body on the case's batch."""
    jif = O.get_tuples(c["video"].F, c["video"].resy, c["video"].resx)[:, torch.from_numpy(c["inds"]).view(-1, 1)]
    if c["two"]:
        r = [Recorder(2), Recorder(2), Recorder(3), Recorder(1)]
        O.seg_loop_body(c["it"], jif, c["video"], r[0], r[1], r[2], r[3], c["cfgd"])
        return dict(map1=r[0].seen, map2=r[1].seen, alpha=r[3].seen)
    r = [Recorder(2), Recorder(3)]
    O.loop_body(c["it"], jif, c["video"], r[0], r[1], c["cfgd"])
    return dict(map1=r[0].seen)


def call_index(c, net):
    """Row indices (into the twin's batch of `net`) of the oracle's calls of that net, in call order."""
    N, R = c["N"], c["R"]
    n = np.arange(N)
    vf, vb = R["rank"][:, 0] >= 0, R["rank"][:, 1] >= 0
    if net == "alpha":
        return [n, 2 * N + n, N + n, 3 * N + R["rank"][vf, 0], 3 * N + R["rank"][vb, 1]]
    idx = [n, N + n, 2 * N + n, np.arange(3 * N, 5 * N)]
    if R["nseg"] > 7:
        idx.append(np.arange(5 * N, 7 * N))
    return idx + [R["flow_base"] + R["rank"][vf, 0], R["flow_base"] + R["rank"][vb, 1]]


def rows_differ(c, R):
    """Number of oracle rows the row set R does not reproduce bit for bit."""
    seen = oracle_rows(c)
    bad = 0
    for net, calls in seen.items():
        idx = call_index(c, net)
        assert len(idx) == len(calls), (net, len(idx), len(calls))
        covered = np.zeros(len(c["R"][net]), bool)
        for i, x in zip(idx, calls):
            assert x.dtype == np.float32 and x.shape == (len(i), 3)
            ok = i < len(R[net])
            got = np.zeros_like(x); got[ok] = R[net][i[ok]]
            bad += int((got.view(np.uint32) != x.view(np.uint32)).any(1).sum())
            covered[i] = True
        assert covered.all(), (net, "rows of the twin the oracle never evaluates")
    return bad


@pytest.mark.parametrize("kind,batch,it", CASES)
def test_prep_rows_equal_the_oracle_batch(kind, batch, it, golden, golden_seg):
    c = case(kind, batch, it, golden, golden_seg)
    R = c["R"]
    assert rows_differ(c, R) == 0
    vid = c["video"]
    f = c["inds"] // (vid.resx * vid.resy)
    assert R["counts"] == (int((c["rec"][:, 13] != 0).sum()), int((c["rec"][:, 14] != 0).sum())) and R["live"] == sum(R["counts"])
    assert not (c["rec"][f == vid.F - 1, 13] != 0).any() and 0 < R["live"] < 2 * batch          # the last frame has no forward match; holes in the masks
    assert R["flow_base"] == (7 if it == 0 else 5) * batch
    tile, written = SR.x0_tiles(R["map1"])
    assert np.array_equal(tile.transpose(0, 2, 1).reshape(-1, 32)[:len(R["map1"]), :3], R["map1"]) and written.sum() == 3 * len(R["map1"])


# ---- the twin against the oracle and autograd ----------------------------------------------------------------------------------------------------
class Leaf:
    """A net that hands out slices of a leaf tensor in the oracle's call order."""

    def __init__(self, rows, idx):
        self.leaf = torch.tensor(np.asarray(rows, np.float64), requires_grad=True)
        self.idx, self.k = idx, 0

    def __call__(self, x):
        i = torch.from_numpy(np.asarray(self.idx[self.k], np.int64)); self.k += 1
        assert len(i) == x.shape[0]
        return self.leaf[i]


@pytest.mark.parametrize("kind,batch,it", [(k, 250, it) for k in "STN" for it in (0, 10001)] + [("T", 700, 0)])
def test_twin_terms_equal_the_oracle_and_seeds_equal_autograd(kind, batch, it, golden, golden_seg):
    c = case(kind, batch, it, golden, golden_seg)
    N, two = c["N"], c["two"]
    n = np.arange(N)
    Kx = SR.coeffs(cfg_of(c["cfgd"], c["video"], batch), it, two, exact=True)
    ref = run(c, SR.loss_single_ref, SR.loss_seg_ref, K=Kx)
    jif = O.get_tuples(c["video"].F, c["video"].resy, c["video"].resx)[:, torch.from_numpy(c["inds"]).view(-1, 1)]
    video = c["video"]
    if two:
        # the reference forms 1 - a_gt in the mask's own dtype, fp32; the twin holds that difference exact plus its rounding in the bound.  The same mask
        # values as an fp64 tensor make the reference's difference exact too: the comparison is then of the formulas alone
        video = O.SegVideo(video.video_frames, video.optical_flows, video.optical_flows_reverse, video.optical_flows_mask, video.optical_flows_reverse_mask,
                           video.mask_frames.double())
        nets = dict(dout_m1=Leaf(c["o1"][:, :2], call_index(c, "map1")), dout_m2=Leaf(c["o2"][:, :2], call_index(c, "map2")),
                    dout_atlas=Leaf(c["oat"][:, :3], [n, 3 * N + n, N + n, 2 * N + n, 4 * N + n, 5 * N + n]), dout_alpha=Leaf(c["oal"][:, :1], call_index(c, "alpha")))
        total, terms = O.seg_loop_body(it, jif, video, nets["dout_m1"], nets["dout_m2"], nets["dout_atlas"], nets["dout_alpha"], c["cfgd"])
    else:
        nets = dict(dout_map=Leaf(c["o1"][:, :2], call_index(c, "map1")), dout_atlas=Leaf(c["oat"][:, :3], [n, N + n, 2 * N + n]))
        total, terms = O.loop_body(it, jif, c["video"], nets["dout_map"], nets["dout_atlas"], c["cfgd"])
    assert total.dtype == torch.float64
    total.backward()
    rec = SR.record_terms(ref["terms"], c["R"]["counts"], N, two)
    for name, (v, _) in rec.items():
        want = float(terms[name].detach())
        assert abs(v - want) <= 1e-12 * abs(want), (name, v, want)
    for name, leaf in nets.items():
        g = leaf.leaf.grad.numpy()
        got = ref[name].v[:len(g), :g.shape[1]]
        assert np.abs(got - g).max() <= 1e-9 * np.abs(g).max(), (name, float(np.abs(got - g).max()), float(np.abs(g).max()))
        assert not ref[name].v[len(g):].any() and not ref[name].v[:, g.shape[1]:].any()                    # pad rows and spare columns: exactly 0
        assert not ref[name].e[len(g):].any()
    for name in map_names(c):
        assert not ref[name].v[N:3 * N].any() and not ref[name].e[N:3 * N].any()                            # the (x, y+1) and (x+1, y) rows: exact zeros


# ---- emulations inside the bounds, bounds that bite ------------------------------------------------------------------------------------------------
def classes_of(c, ref, emu=None, fused=False, mut=()):
    """{class: (got or None, ref value, running error, usable mask)} over the five tensor classes; the uv classes come from dpe_to_uv on the atlas net's dZ_0."""
    N = c["N"]
    out = {}
    names = map_names(c)
    out["atlas seed"] = (None if emu is None else emu["dout_atlas"].v, ref["dout_atlas"].v, ref["dout_atlas"].e, ~ref["dout_atlas"].und)
    if c["two"]:
        out["alpha seed"] = (None if emu is None else emu["dout_alpha"].v, ref["dout_alpha"].v, ref["dout_alpha"].e, ~ref["dout_alpha"].und)
    out["mapping seed"] = (None if emu is None else np.concatenate([emu[m].v[3 * N:] for m in names]), np.concatenate([ref[m].v[3 * N:] for m in names]),
                           np.concatenate([ref[m].e[3 * N:] for m in names]), ~np.concatenate([ref[m].und[3 * N:] for m in names]))
    # the uv gradient: the atlas seed the kernel under test wrote goes through the atlas net's backward chain (here: torch fp32)
    seed_at = ref["dout_atlas"].v if emu is None else emu["dout_atlas"].v
    dz0 = dz0_of(c, seed_at)
    seed_v = np.concatenate([ref[m].v[:3 * N, :2] for m in names]); seed_e = np.concatenate([ref[m].e[:3 * N, :2] for m in names])
    und = np.concatenate([ref[m].und[:3 * N, :2] for m in names])
    v, e = SR.dpe_to_uv_ref(dz0, c["W0"], c["pe"], seed_v, seed_e)
    got = None
    if emu is not None:
        got = SR.dpe_to_uv_emu(dz0, c["W0"], c["pe"], np.concatenate([emu[m].v[:3 * N, :2] for m in names]), fused=fused, mut=mut)
    centre = (np.arange(len(v)) % (3 * N)) < N
    out["uv gradient"] = (None if got is None else got[~centre], v[~centre], e[~centre], ~und[~centre])
    out["seed + uv gradient"] = (None if got is None else got[centre], v[centre], e[centre], ~und[centre])
    return out


def outside(classes):
    """{class: entries outside 2 x the running error (exactly equal where the bound is 0)}."""
    return {k: int((ok & ~(np.abs(got - v) <= SR.BOUND_FACTOR * e)).sum()) for k, (got, v, e, ok) in classes.items()}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind,batch,it", CASES)
def test_fp32_emulations_stay_inside_the_bounds_and_the_bounds_bite(kind, batch, it, fused, golden, golden_seg):
    c = case(kind, batch, it, golden, golden_seg)
    ref = run(c, SR.loss_single_ref, SR.loss_seg_ref)
    emu = run(c, SR.loss_single_emu, SR.loss_seg_emu, fused=fused)
    cl = classes_of(c, ref, emu, fused)
    assert not any(outside(cl).values()), outside(cl)
    rec = SR.record_terms(ref["terms"], c["R"]["counts"], c["N"], c["two"])
    got = SR.record_terms({k: SR.V(t.done()[0]) for k, t in emu["terms"].items()}, c["R"]["counts"], c["N"], c["two"])
    for name, (v, b) in rec.items():
        assert abs(got[name][0] - v) <= b, (name, got[name][0], v, b)
    left = int(ref["undecided_samples"].sum())
    assert left <= 0.01 * max(c["R"]["live"], 1), left
    for name, (got_, v, e, ok) in cl.items():
        worst = float((np.abs(got_ - v)[ok & (e > 0)] / e[ok & (e > 0)]).max())
        loose = float((SR.BOUND_FACTOR * e[ok] > 2.0 ** -6 * np.maximum(np.abs(v[ok]), np.median(np.abs(v[ok])))).mean())
        print("%s %d it %d %s %-18s worst error / running error %.3f, share of loose bounds %.4f (at 2^-10: %.4f), left out %d" % (
            kind, batch, it, "fused" if fused else "plain", name, worst, loose,
            float((SR.BOUND_FACTOR * e[ok] > 2.0 ** -10 * np.maximum(np.abs(v[ok]), np.median(np.abs(v[ok])))).mean()), left))
        assert loose <= 0.05, (name, loose)


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", ["y+d", "rank_b", "flow_base"])
@pytest.mark.parametrize("kind", ["S", "T"])
def test_row_mutations_break_the_equality(kind, mut, golden, golden_seg):
    c = case(kind, 700, 10001, golden, golden_seg)                 # nseg 7: the flow rows sit at 5N
    bad = rows_differ(c, SR.prep_rows(c["rec"], c["inds"], c["cfg"], c["it"], c["two"], mut=(mut,)))
    print("rows mutation %s, kind %s: %d oracle rows not reproduced" % (mut, kind, bad))
    assert bad > 0


SEED_MUTATIONS = [(k, it, m) for k, it in (("S", 0), ("T", 0), ("T", 10001), ("N", 10001))
                  for m in ("dtx_dty", "du_xm_ym", "eps", "aflow_sign", "fg_weight", "cnt_bwd", "octave", "assign")
                  if k == "T" or m not in ("aflow_sign", "fg_weight")]            # the alpha net exists in the two-layer path only


@pytest.mark.parametrize("kind,it,mut", SEED_MUTATIONS)
def test_seed_mutations_leave_the_bounds(kind, it, mut, golden, golden_seg):
    c = case(kind, 250, it, golden, golden_seg)
    ref = run(c, SR.loss_single_ref, SR.loss_seg_ref)
    emu = run(c, SR.loss_single_emu, SR.loss_seg_emu, mut=(mut,))
    bad = outside(classes_of(c, ref, emu, mut=(mut,)))
    tot = {k: int(ok.sum()) for k, (_, _, _, ok) in classes_of(c, ref).items()}
    print("mutation %s, kind %s it %d: entries outside / entries: %s" % (mut, kind, it, {k: "%d / %d" % (bad[k], tot[k]) for k in bad}))
    assert sum(bad.values()) > 0
    assert set(SR.MUTATIONS) >= {mut}
