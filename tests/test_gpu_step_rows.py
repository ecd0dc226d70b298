"""The links of a training step AROUND the chains, per row: k_prep's batch rows, the loss kernels' seed gradients and chain_dpe_to_uv (csrc/elem.hip,
mlp_common.h), against tests/step_ref.py — recomputed from the kernels' OWN inputs (the pixel records, the nets' output rows, the atlas net's dZ_0 and PE
tile of the same step), through af_train_steps with debug on, like tests/test_gpu_chain_entries.py.  tests/test_step_ref_host.py ties the twin to the
oracle and shows that the mutations listed there leave these bounds; MEASUREMENTS.md has the kernel mutations that fail the cases of this file.

Configurations: kinds S, T, N of tests/test_gpu_adam.py (N: a mapping net with PE) on the 37x21x5 "field" video (seed 4: masks with holes, 72 % of the
matches valid, no forward match on the last frame); samples_batch 250 (one block of k_prep, last wave partial) and 700 (three blocks, the last of 188
threads: the wave, block and look-back prefixes); one debug step from the pre-trained state at iteration 0 (nseg 9, global rigidity and bootstrapping on)
and one at iteration 10001 (nseg 7, both off: the flow rows sit at 5N); mlp modes 0, 1, 3 on kind S, 3 on T and N.

Per case:
  rows        "rows" of every mapping and alpha net == prep_rows on every live row, BIT FOR BIT (the fourth column 0); the "x0" tile == its transpose;
              valid_fwd / valid_bwd of the loss record == the mask counts.  Rows behind the live ones are not asserted: k_prep does not write them.
  seeds       atlas dout, alpha dout and mapping dout rows >= 3N hold the loss seed alone: within 2 x the running error, exactly 0 where the twin says 0
              (the pad rows of the last live tile, the spare columns); mapping rows N..3N hold chain_dpe_to_uv alone (their seed is exactly 0), rows
              0..N seed + uv gradient; kind T: atlas rows 3N..6N go to mapping2.
  loss record |hip - fp64 sum of the twin's per-sample terms| <= summed running error + N u sum |term|.
  kinks       entries that depend on an alpha-flow difference or a flow norm within its own error of 0 are left out: at most 1 % of the valid matches.
  bite        per tensor class at most 5 % of the entries with 2 bound > 2^-6 max(|ref|, median |ref| of the class): a condition on the INPUTS.
State: P0 of test_gpu_adam.start_state (mapping nets pre-trained 40 iterations); kind N pre-trains 600 more — its PE mapping net is far from the
identity after 40 and the rigidity terms' (J^T J + eps)^-1 too badly conditioned for the bite condition (tests/test_step_ref_host.py PRETRAIN).
The figures printed per class (rms and worst error / bound) are figures, not assertions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_ref as CR  # noqa: E402
import step_ref as SR  # noqa: E402
import test_gpu_adam as TA  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = {0: "fp32 MFMA", 1: "bf16x6", 3: "f16x3"}
EXTRA_PRETRAIN = {"S": 0, "T": 0, "N": 600}
CLASSES = ("atlas seed", "alpha seed", "mapping seed", "uv gradient", "seed + uv gradient")
_states = {}


def state(kind, golden, golden_seg):
    """The parameters the step runs on: P0 of start_state, the mapping net of kind N pre-trained EXTRA_PRETRAIN iterations more."""
    if kind not in _states:
        P = TA.start_state(kind, golden, golden_seg)["P0"]
        if EXTRA_PRETRAIN[kind]:
            af, _ = TA.make_fit(kind, golden, golden_seg)
            try:
                TA.load_flat(af, P)
                af.pre_train_mapping(EXTRA_PRETRAIN[kind], seed=7)
                P = {net: af.get_params_flat(net) for net in af.nets}
            finally:
                af.close()
        _states[kind] = P
    return _states[kind]


class Stats:
    def __init__(self):
        self.d, self.loose, self.failed = {}, {}, []

    def hold(self, tag, cls, got, v, e, ok):
        """|got - v| <= 2 e at every usable entry (exactly equal where e is 0); the class's figures."""
        got = np.asarray(got, np.float64)
        err, bound = np.abs(got - v), SR.BOUND_FACTOR * e
        s = self.d.setdefault(cls, [0.0, 0, 0.0, 0, 0])
        pos = ok & (bound > 0)
        if pos.any():
            r = err[pos] / bound[pos]
            s[0] += float((r * r).sum()); s[1] += int(pos.sum()); s[2] = max(s[2], float(r.max()))
        s[3] += int((ok & (bound == 0)).sum()); s[4] += int((~ok).sum())
        ref = np.abs(v[ok])
        self.loose.setdefault(cls, []).append(bound[ok] > 2.0 ** -6 * np.maximum(ref, np.median(ref)))
        bad = np.argwhere(ok & ~(err <= bound))
        if bad.size:            # asserted by report(), behind the figures of every class
            self.failed.append((tag, cls, "%d of %d entries outside the bound; first at %s: kernel %.9g twin %.9g bound %.3g" % (
                len(bad), int(ok.sum()), tuple(bad[0]), got[tuple(bad[0])], v[tuple(bad[0])], bound[tuple(bad[0])])))

    def report(self, tag):
        for cls in CLASSES:
            if cls in self.d:
                ss, n, worst, zeros, left = self.d[cls]
                loose = float(np.concatenate(self.loose[cls]).mean())
                print("%s %-18s error / bound: rms %.4f worst %.4f over %d entries; %d exact zeros; %d entries left out; loose bounds %.4f" % (
                    tag, cls, np.sqrt(ss / max(n, 1)), worst, n, zeros, left, loose), flush=True)
                if loose > 0.05:
                    self.failed.append((tag, cls, "share of entries with 2 bound > 2^-6 max(|ref|, median |ref|)", loose))
        assert not self.failed, self.failed


def check_step(af, P, inds, it, losses, tag):
    import aiod_amd
    A = aiod_amd.atlasfit
    two, N = af.two_layer, af.N
    names = af.LOSS_NAMES_TWO_LAYER if two else af.LOSS_NAMES
    caps, _ = af.step_work(it)
    rec = af.read_records(inds)
    R = SR.prep_rows(rec, inds, af.cfg, it, two)
    K = SR.coeffs(af.cfg, it, two)
    assert R["nseg"] == (9 if it == 0 else 7) and caps[A.NET_MAPPING1] == R["nseg"] * N
    rows4 = lambda net, which, n: CR.rows4_of(af.debug_tiles(net, which, 0, caps[net], 0, (n + 31) // 32))[:n]          # noqa: E731
    # ---- rows, bit for bit
    assert (int(losses[names.index("valid_fwd")]), int(losses[names.index("valid_bwd")])) == R["counts"], (tag, "valid match counts")
    nets = [("map1", A.NET_MAPPING1)] + ([("map2", A.NET_MAPPING2), ("alpha", A.NET_ALPHA)] if two else [])
    for name, net in nets:
        want = R[name]
        got = rows4(net, "rows", len(want))
        wrong = np.flatnonzero((got[:, :3].view(np.uint32) != want.view(np.uint32)).any(1) | (got[:, 3] != 0))
        assert wrong.size == 0, (tag, name, "%d of %d live rows differ from prep_rows; first row %d: kernel %s twin %s" % (
            wrong.size, len(want), wrong[0], got[wrong[0]], want[wrong[0]]))
        if A.imlp_shapes(net, af.cfg)[0][1] == 3:
            tile, written = SR.x0_tiles(want)
            x0 = af.debug_tiles(net, "x0", 0, caps[net], 0, len(tile))
            assert np.array_equal(x0.view(np.uint32)[written], tile.view(np.uint32)[written]), (tag, name, "x0 tile is not the transpose of the rows")
    with pytest.raises(A.AtlasFitError, match="no such tensor"):
        af.debug_tiles(A.NET_ATLAS, "rows", 0, caps[A.NET_ATLAS], 0, 1)
    # ---- seeds
    st = Stats()
    RA = (6 if two else 3) * N
    o1 = rows4(A.NET_MAPPING1, "out", len(R["map1"]))
    oat = rows4(A.NET_ATLAS, "out", RA)
    if two:
        o2, oal = rows4(A.NET_MAPPING2, "out", len(R["map2"])), rows4(A.NET_ALPHA, "out", len(R["alpha"]))
        tw = SR.loss_seg_ref(o1, o2, oal, oat, rec, R["rank"], R["counts"], K)
        maps = [("dout_m1", A.NET_MAPPING1), ("dout_m2", A.NET_MAPPING2)]
        d = rows4(A.NET_ALPHA, "dout", len(tw["dout_alpha"].v))
        st.hold(tag, "alpha seed", d, tw["dout_alpha"].v, tw["dout_alpha"].e, ~tw["dout_alpha"].und)
    else:
        tw = SR.loss_single_ref(o1, oat, rec, R["rank"], R["counts"], K)
        maps = [("dout_map", A.NET_MAPPING1)]
    st.hold(tag, "atlas seed", rows4(A.NET_ATLAS, "dout", RA), tw["dout_atlas"].v, tw["dout_atlas"].e, ~tw["dout_atlas"].und)
    dmap = {}
    for name, net in maps:
        t = tw[name]
        dmap[name] = rows4(net, "dout", len(t.v))
        assert len(t.v) % 32 == 0 and len(t.v) >= (R["nseg"] - 2) * N + R["live"]
        st.hold(tag + " " + name, "mapping seed", dmap[name][3 * N:], t.v[3 * N:], t.e[3 * N:], ~t.und[3 * N:])
        assert not t.v[N:3 * N].any() and not t.e[N:3 * N].any()
    # ---- the uv gradient: atlas rows [0, 3N) land on mapping1, [3N, 6N) on mapping2 (split_row)
    shapes = A.imlp_shapes(A.NET_ATLAS, af.cfg)
    hid = shapes[0][0]
    W0 = CR.unflatten(P[A.NET_ATLAS], shapes)[0][0]
    nt = (RA + 31) // 32
    dz0 = CR.rows_of(af.debug_tiles(A.NET_ATLAS, "dz", 0, caps[A.NET_ATLAS], 0, nt))[:RA, :hid]
    pe = CR.rows_of(af.debug_tiles(A.NET_ATLAS, "pe", 0, caps[A.NET_ATLAS], 0, nt))[:RA, :40]
    seed_v = np.concatenate([tw[m].v[:3 * N, :2] for m, _ in maps]); seed_e = np.concatenate([tw[m].e[:3 * N, :2] for m, _ in maps])
    und = np.concatenate([tw[m].und[:3 * N, :2] for m, _ in maps])
    got = np.concatenate([dmap[m][:3 * N, :2] for m, _ in maps])
    v, e = SR.dpe_to_uv_ref(dz0, W0, pe, seed_v, seed_e)
    centre = (np.arange(len(v)) % (3 * N)) < N
    st.hold(tag, "uv gradient", got[~centre], v[~centre], e[~centre], ~und[~centre])
    st.hold(tag, "seed + uv gradient", got[centre], v[centre], e[centre], ~und[centre])
    for m, _ in maps:
        assert not dmap[m][:3 * N, 2:].any(), (tag, m, "gradient on the spare columns")
    # ---- the loss record
    for name, (val, bound) in SR.record_terms(tw["terms"], R["counts"], N, two).items():
        hip = float(losses[names.index(name)])
        print("%s loss record %-20s hip %.9g twin %.9g error / bound %.4f" % (tag, name, hip, val, abs(hip - val) / bound if bound > 0 else 0.0), flush=True)
        if not abs(hip - val) <= bound:
            st.failed.append((tag, "loss record", name, hip, val, bound))
    # ---- kinks
    left = int(tw["undecided_samples"].sum())
    print("%s %d live rows (%d + %d valid matches of %d samples); %d samples left out at a kink" % (tag, R["live"], R["counts"][0], R["counts"][1], N, left), flush=True)
    assert left <= 0.01 * R["live"], (tag, "samples left out at a kink", left)
    st.report(tag)


@pytest.mark.parametrize("it", [0, 10001])
@pytest.mark.parametrize("batch", [250, 700])
@pytest.mark.parametrize("kind,mlp_mode", [("S", 0), ("S", 1), ("S", 3), ("T", 3), ("N", 3)])
def test_rows_seeds_and_uv_gradient_of_one_step(kind, mlp_mode, batch, it, golden, golden_seg):
    P = state(kind, golden, golden_seg)
    af, _ = TA.make_fit(kind, golden, golden_seg, mlp_mode=mlp_mode, batch=batch, flow="field")
    try:
        TA.load_flat(af, P)
        af.set_debug(True)
        inds = TA.step_inds(af, 12, batch=batch)[0]
        losses = af.train_steps(it, 1, inds)[0]
        check_step(af, P, inds, it, losses, "%s %s batch %d iteration %d:" % (kind, MODES[mlp_mode], batch, it))
    finally:
        af.close()


@pytest.mark.parametrize("seed", [2 ** 32 + 7])
def test_the_device_sampler_draws_the_batch_of_a_training_step(seed, golden, golden_seg):
    """The production path of k_prep: no injected indices, the batch of iteration `it` is af_rand_below(seed, it, n, 0, resx resy F) — the twin's draws
    (tests/pretrain_ref.py rand_below; the seed's high word is the second key word), and from them the same rows, seeds and uv gradient as above."""
    import pretrain_ref as PR
    kind, batch, it = "S", 250, 10001
    P = state(kind, golden, golden_seg)
    af, _ = TA.make_fit(kind, golden, golden_seg, mlp_mode=3, batch=batch, flow="field")
    try:
        TA.load_flat(af, P)
        af.set_debug(True)
        c = af.cfg
        inds = PR.rand_below(seed, it, batch, 0, int(c.resx) * int(c.resy) * int(c.number_of_frames))
        assert np.unique(inds).size > batch // 2
        losses = af.train_steps(it, 1, None, seed=seed)[0]
        check_step(af, P, inds, it, losses, "%s %s batch %d iteration %d, device sampler seed %d:" % (kind, MODES[3], batch, it, seed))
    finally:
        af.close()
