"""ONE pre-train step (af_pretrain) per element, as tests/test_gpu_step_rows.py, test_gpu_chain_entries.py, test_gpu_dw_entries.py and test_gpu_adam.py hold
the training step — recomputed in fp64 from the kernels' OWN inputs (af_debug_tiles, af_get_last_grads, the parameters the step ran on), every entry
inside a DERIVED bound (tests/chain_ref.py, tests/adam_ref.py, the dW bound of tests/test_gpu_dw_entries.py, the head of tests/pretrain_ref.py) — and the
device sampler af_rand_below per draw.  Pre-training runs code no other route reaches: the 16-row chains of csrc/mlp16.hip (mlp modes 0-2; their own
register and mask layout, the in-place five-octave PE, half-tile stores, dead waves), k_pre_prep / k_pre_loss, the 32-row chains on pretrain_batch rows
(mode 3), the schedules sched[2] / sched[3] of k_dw and the optimizer pre_m / pre_v.

Isolating a step.  af_pretrain runs pretrain_iters x F steps and the debug tensors hold the last one; a handle of ONE frame needs no video, and
pre_train_mapping(1, ys, xs) on it is exactly one step from known parameters and zero moments, counter 1, t = -1.  t != -1: a two-frame handle runs
step 0 at t = -1 and step 1 at t = 0; its step 0 is the launch sequence of the one-frame handle's only step, so the parameters step 1 ran on come from
there.

Kinds (tests/pretrain_ref.py KINDS): S mapping1 of the shipped single-atlas nets (NsMap1); T2 mapping2 of the shipped two-layer nets (NsMap2); N mapping1
of width 40, 3 layers, PE with 3 frequencies (NsMapPe: 12 of the 30 slots the kernel always writes meet zero weights, units >= 40 are padding); P5
mapping2 with PE of 5 frequencies, width 256 (every slot live).  37x21 frames, starting from the 40-iteration pre-trained state of
tests/test_gpu_adam.start_state (mapping1's dead unit included).  pretrain_batch 16 (one 32-row tile: a live 16-row tile of pad rows only, two dead
waves), 272 (17 + 1 16-row tiles, five workgroups, two dead waves), 490 (a partial half and an all-pad half), 500, and the shipped 10 000 once.
mlp modes 0, 1, 3 on S; 1, 3 on the others; dw mode 1, and 0 on S.

Per case: rows and the x0 tile BIT FOR BIT; the PE tile (all 30 features) and its identities; every layer's activations on every row of every live
tile, masks, outputs; the loss seed and the loss the call returns; dz_last and every dz plane, exactly 0 where the activation is 0 and on the pad rows
of the last tile ("pad rows of the last tile must carry zero gradient" — also with rows an earlier training step left behind NB); every weight
gradient per entry; the parameters after the step against fp64 Adam fed the kernel's own gradient, every other net bit-identical.  The figures printed
per class (rms and worst error / bound) are figures, not assertions; tests/test_pretrain_ref_host.py shows the mutations these bounds catch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402
import chain_ref as CR  # noqa: E402
import pretrain_ref as PR  # noqa: E402
import test_gpu_adam as TA  # noqa: E402
import test_gpu_chain_entries as CE  # noqa: E402
import test_gpu_dw_entries as DW  # noqa: E402
import test_gpu_step_rows as RS  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = CE.MODES
_states = {}


def make(kind, golden, golden_seg, F=1, batch=500, mlp_mode=1, dw_mode=1, resx=PR.RESX, resy=PR.RESY):
    """(AtlasFit without a video, the mapping net the kind pre-trains)."""
    import aiod_amd
    two, over, which, _ = PR.KINDS[kind]
    cfg = dict((golden_seg if two else golden)["config"]); cfg.update(over); cfg.update(samples_batch=TA.BATCH)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(resx, resy, F, cfg, two_layer=two, pretrain_batch=batch))
    af.set_mlp_mode(mlp_mode); af.set_dw_mode(dw_mode)
    return af, (aiod_amd.NET_MAPPING1 if which == 1 else aiod_amd.NET_MAPPING2)


def state(kind, golden, golden_seg):
    """{net: flat parameters} the steps start from: P0 of test_gpu_adam.start_state; kind P5 (no such state there) built the same way."""
    import aiod_amd
    from oracle import atlas_oracle as O
    base = PR.KINDS[kind][3]
    if base:
        return TA.start_state(base, golden, golden_seg)["P0"]
    if kind not in _states:
        af, net = make(kind, golden, golden_seg, F=5, mlp_mode=3)
        try:
            cfg = dict(golden_seg["config"]); cfg.update(PR.KINDS[kind][1])
            for n, m in zip(af.nets, O.build_seg_models(cfg, seed=2)):
                af.load_state_dict(n, m.state_dict())
            af.pre_train_mapping(PR.PRETRAIN, seed=5)
            af.pre_train_mapping(PR.PRETRAIN, seed=6, net=aiod_amd.NET_MAPPING2)
            P = {n: af.get_params_flat(n) for n in af.nets}
            t = {name: sl for name, sl, _ in TA.tensors_of(af, 0)}
            P[0][t["hidden.%d.bias" % TA.DEAD_LAYER].start + TA.DEAD_UNIT] = -100.0
        finally:
            af.close()
        _states[kind] = P
    return _states[kind]


def check_pre_step(af, net, P, F, f, ys, xs, loss, mlp_mode, dw_mode, tag, adam=True, forward=True, dw=True, und_cap=0, res=(PR.RESX, PR.RESY)):
    """The last step of an af_pretrain call on `af` was step `f` of an F-frame handle on the draws ys, xs (None: not checked), from the parameters P
    ({net: flat}; None with forward=False).  Holds every tensor the step left; returns (chain Stats, seed Stats)."""
    import aiod_amd
    A = aiod_amd.atlasfit
    NB = int(af.cfg.pretrain_batch)
    nt = (NB + 31) // 32
    R_ = 32 * nt
    tiles = lambda which, l=0: af.debug_tiles(net, which, l, NB, 0, nt)            # noqa: E731   plane stride tiles_of(NB)
    shapes = A.imlp_shapes(net, af.cfg)
    nl, hid, enc, nout = len(shapes), shapes[0][0], shapes[0][1], shapes[-1][0]
    xyt = enc == 3
    m16 = mlp_mode != 3                                     # the 16-row chains: every layer on the fp32 pipe, the private mask layout
    st, sd = CE.Stats(), RS.Stats()
    # ---- rows, bit for bit
    rows = CR.rows4_of(tiles("rows"))
    assert rows.shape == (R_, 4)
    if ys is not None:
        want = PR.pre_prep_rows(ys, xs, res[0], res[1], F, f)
        wrong = np.flatnonzero((rows[:NB].view(np.uint32) != want.view(np.uint32)).any(1))
        assert wrong.size == 0, (tag, "%d of %d rows differ from pre_prep_rows; first row %d: kernel %s twin %s" % (wrong.size, NB, wrong[0], rows[wrong[0]], want[wrong[0]]))
        if xyt:
            tile, written = PR.pre_x0_tiles(want)
            assert np.array_equal(tiles("x0").view(np.uint32)[written], tile.view(np.uint32)[written]), (tag, "x0 tile is not the transpose of the rows")
    assert not rows[:NB, 3].any(), (tag, "rows: the fourth column")
    out = CR.rows4_of(tiles("out"))
    dout = CR.rows4_of(tiles("dout"))
    acts = [CR.rows_of(tiles("acts", l)) for l in range(nl - 1)]
    dz = [CR.rows_of(tiles("dz", l)) for l in range(nl - 1)]
    dzl = CR.rows_of(tiles("dz_last"))
    layers = CR.unflatten(P[net], shapes) if P is not None else None
    # ---- the input stage: every row of every live tile, the pad rows from whatever the rows buffer holds
    if xyt:
        X0 = rows[:, :3].astype(np.float64)
        pe = None
    else:
        pet = CR.rows_of(tiles("pe"))
        assert not pet[:, 30:].any(), (tag, "PE tile: slots behind the last feature")
        ref, bound = CR.pe_ref(rows[:, :3].astype(np.float64), 5, CR.C_ARG_XYT)              # all 30 features the kernel writes, whatever the net's count
        st.hold(tag + " PE tile", "PE", pet[:, :30], ref, bound, np.ones_like(ref))
        for name, val, want_, bound in CR.pe_identities(pet[:NB], 3, 5, CR.C_ARG_XYT):       # |x| <= 1 on the rows of the batch
            st.hold(tag + " PE tile, " + name, "PE", val, want_, bound, np.ones_like(want_))
        X0 = pet[:, :enc]
    # ---- forward
    for l in range(nl - 1):
        assert not acts[l][:, hid:].any(), (tag, l, "activation on a padding unit")
        words = tiles("masks", l)
        bits = PR.mask_bits16(words) if m16 else CR.mask_bits(words)
        wrong = np.argwhere(bits != (acts[l] > 0))
        assert wrong.size == 0, (tag, "mask words of layer %d: %d bits differ from [acts > 0]; first at (row, feature) %s" % (l, len(wrong), tuple(wrong[0])))
        if forward:
            W, b = layers[l]
            X = X0 if l == 0 else acts[l - 1][:, :hid]
            ref, bound = CR.forward_layer(W, b, X, mlp_mode, None if (l == 0 or m16) else hid)
            st.hold("%s acts[%d]" % (tag, l), "layer 0" if l == 0 else "hidden", acts[l][:, :hid], ref, bound, np.abs(X) @ np.abs(W).T + np.abs(b))
    if forward:
        W, b = layers[-1]
        X = acts[nl - 2][:, :hid]
        ref, bound = CR.output_layer(W, b, X)
        st.hold(tag + " outputs", "output", out[:, :nout], ref, bound, np.abs(X) @ np.abs(W).T + np.abs(b))
    assert not out[:, nout:].any(), (tag, "output columns behind the net's outputs")
    # ---- the loss seed and the loss
    tw = PR.pre_loss_ref(rows[:NB], out[:NB], float(af.cfg.uv_mapping_scale), NB)
    und = np.repeat(tw.und[:, None], 2, axis=1)
    sd.hold(tag, "mapping seed", dout[:NB, :2], tw.d, tw.de, ~und)
    assert not dout[:NB, 2:].any(), (tag, "seed on the spare columns")
    assert not dout[NB:].any(), (tag, "seed on the pad rows of the last tile")
    assert int(tw.und.sum()) <= und_cap, (tag, "samples left out: l within its own error of 0", int(tw.und.sum()))
    if loss is not None:
        print("%s loss: hip %.9g twin %.9g error / bound %.4f; %d samples left out" % (tag, loss, tw.mean, abs(loss - tw.mean) / tw.mean_bound, int(tw.und.sum())), flush=True)
        if not abs(float(loss) - tw.mean) <= tw.mean_bound:
            sd.failed.append((tag, "loss record", float(loss), tw.mean, tw.mean_bound))
    # ---- backward
    ref, bound = CR.seed(out[:, :nout], dout[:, :nout])
    st.hold(tag + " dz_last", "seed", dzl[:, :nout], ref, bound, np.abs(dout[:, :nout].astype(np.float64)))
    assert not dzl[:, nout:].any(), (tag, "dz_last: rows behind the net's outputs")
    assert not dzl[NB:].any(), (tag, "dz_last on the pad rows of the last tile")
    for l in range(nl - 1):
        assert not dz[l][:, hid:].any(), (tag, l, "gradient on a padding unit")
        assert not dz[l][NB:].any(), (tag, l, "gradient on the pad rows of the last tile")
        assert not dz[l][acts[l] == 0].any(), (tag, l, "gradient where the kernel's own activation is 0")
    if forward:
        ref, bound, rowmax = CR.backward_layer(dzl[:, :nout], layers[-1][0][:, :hid], acts[nl - 2][:, :hid], mlp_mode, fp32_pipe=True)
        st.hold("%s dz[%d]" % (tag, nl - 2), "top backward", dz[nl - 2][:, :hid], ref, bound, np.abs(dzl[:, :nout]) @ np.abs(layers[-1][0][:, :hid]))
        for l in range(nl - 2, 0, -1):
            Wh = layers[l][0][:, :hid]
            ref, bound, rowmax = CR.backward_layer(dz[l][:, :hid], Wh, acts[l - 1][:, :hid], mlp_mode, rowmax=rowmax, fp32_pipe=m16)
            st.hold("%s dz[%d]" % (tag, l - 1), "backward", dz[l - 1][:, :hid], ref, bound, np.abs(dz[l][:, :hid]) @ np.abs(Wh))
    bias = {name: sl for name, sl, _ in TA.tensors_of(af, net)}["hidden.%d.bias" % TA.DEAD_LAYER]
    if net == A.NET_MAPPING1 and af.get_params_flat(net)[bias.start + TA.DEAD_UNIT] < -99.0:          # the dead unit of the starting state
        assert not acts[TA.DEAD_LAYER][:, TA.DEAD_UNIT].any(), (tag, "the dead unit is active")
        assert not dz[TA.DEAD_LAYER][:, TA.DEAD_UNIT].any(), (tag, "gradient on the dead unit")
    # ---- weight gradients: dZ^T X from the kernel's own tiles, every row of the live tiles entering
    if dw:
        w = DW.check_net(af, net, NB, R_, DW._slots_max(af, 2 if net == A.NET_MAPPING1 else 3), dw_mode, tag)
        print("%s %s: worst weight-gradient error / bound %.4f" % (tag, DW.DW_NAMES[dw_mode], w), flush=True)
    # ---- Adam: zero moments, counter 1, fed the kernel's own gradient
    if adam:
        g, p1, p0 = af.last_grads(net), af.get_params_flat(net), P[net]
        z = np.zeros_like(p0)
        ref = R.adam_fp64(p0, z, z, g, 1)[0]
        bp = R.adam_bounds(p0, z, z, g, 1)[0]
        err = np.abs(p1.astype(np.float64) - ref)
        bad = np.flatnonzero(~(err <= bp))
        print("%s Adam: worst parameter error / bound %.4f" % (tag, float((err / bp).max())), flush=True)
        assert bad.size == 0, (tag, "%d parameters outside the fp32 round-off bound of the first Adam step" % bad.size, bad[:5], err[bad[:5]], bp[bad[:5]])
        still = g == 0
        assert np.array_equal(p1[still].view(np.uint32), p0[still].view(np.uint32)), (tag, "a parameter with a zero gradient and zero moments moved")
        for o in af.nets:
            if o != net:
                assert TA._same(af.get_params_flat(o), P[o]), (tag, "pre-training net %d moved net %d" % (net, o))
    return st, sd


def report(st, sd, tag):
    st.report(tag)
    sd.report(tag)          # asserts what hold() collected and the bite condition of the seed class


def one_step(af, net, P, ys, xs):
    TA.load_flat(af, P)
    af.set_debug(True)
    return float(af.pre_train_mapping(1, ys, xs, net=net, return_losses=True)[-1])


CASES = [("S", 0), ("S", 1), ("S", 3), ("T2", 1), ("T2", 3), ("N", 1), ("N", 3), ("P5", 1), ("P5", 3)]


@pytest.mark.parametrize("batch", PR.BATCHES)
@pytest.mark.parametrize("kind,mlp_mode", CASES)
def test_one_pretrain_step_entry_by_entry(kind, mlp_mode, batch, golden, golden_seg):
    P = state(kind, golden, golden_seg)
    af, net = make(kind, golden, golden_seg, F=1, batch=batch, mlp_mode=mlp_mode)
    try:
        ys, xs = PR.draws(21, 1, batch)
        loss = one_step(af, net, P, ys, xs)
        tag = "%s %s batch %d:" % (kind, MODES[mlp_mode], batch)
        report(*check_pre_step(af, net, P, 1, 0, ys[0], xs[0], loss, mlp_mode, 1, tag), tag)
    finally:
        af.close()


@pytest.mark.parametrize("mlp_mode", [1, 3])
def test_one_pretrain_step_with_the_fp32_weight_gradient(mlp_mode, golden, golden_seg):
    P = state("S", golden, golden_seg)
    af, net = make("S", golden, golden_seg, F=1, batch=490, mlp_mode=mlp_mode, dw_mode=0)
    try:
        ys, xs = PR.draws(23, 1, 490)
        loss = one_step(af, net, P, ys, xs)
        tag = "S %s batch 490, dw fp32:" % MODES[mlp_mode]
        report(*check_pre_step(af, net, P, 1, 0, ys[0], xs[0], loss, mlp_mode, 0, tag), tag)
    finally:
        af.close()


def test_one_pretrain_step_at_the_shipped_batch(golden, golden_seg):
    """pretrain_batch 10 000: 157 workgroups of the 16-row chains, 626 16-row tiles (625 with rows, the last one padding)."""
    P = state("S", golden, golden_seg)
    af, net = make("S", golden, golden_seg, F=1, batch=PR.BIG_BATCH, mlp_mode=1)
    try:
        ys, xs = PR.draws(21, 1, PR.BIG_BATCH)
        loss = one_step(af, net, P, ys, xs)
        tag = "S %s batch %d:" % (MODES[1], PR.BIG_BATCH)
        report(*check_pre_step(af, net, P, 1, 0, ys[0], xs[0], loss, 1, 1, tag), tag)
    finally:
        af.close()


@pytest.mark.parametrize("kind,mlp_mode", [("S", 1), ("S", 3), ("N", 1), ("P5", 3)])
def test_the_second_frame_of_a_two_frame_handle(kind, mlp_mode, golden, golden_seg):
    """t = 0: step 1 of an F = 2 handle, held against the parameters the F = 1 handle's only step (the same launch sequence as step 0) leaves."""
    NB = 272
    P = state(kind, golden, golden_seg)
    ys, xs = PR.draws(24, 2, NB)
    a1, net = make(kind, golden, golden_seg, F=1, batch=NB, mlp_mode=mlp_mode)
    a2, _ = make(kind, golden, golden_seg, F=2, batch=NB, mlp_mode=mlp_mode)
    try:
        one_step(a1, net, P, ys[:1], xs[:1])
        rows1 = CR.rows4_of(a1.debug_tiles(net, "rows", 0, NB))[:NB]
        assert np.array_equal(rows1.view(np.uint32), PR.pre_prep_rows(ys[0], xs[0], PR.RESX, PR.RESY, 2, 0).view(np.uint32))      # step 0 of F = 2: the same rows, t = -1
        P1 = dict(P); P1[net] = a1.get_params_flat(net)
        loss = one_step(a2, net, P, ys, xs)
        rows2 = CR.rows4_of(a2.debug_tiles(net, "rows", 0, NB))[:NB]
        assert np.all(rows2[:, 2].view(np.uint32) == 0), "t of the second of two frames is fl32(1 / (2 / 2.0) - 1) = +0"
        tag = "%s %s batch %d, frame 1 of 2:" % (kind, MODES[mlp_mode], NB)
        report(*check_pre_step(a2, net, P1, 2, 1, ys[1], xs[1], loss, mlp_mode, 1, tag, adam=False), tag)       # (its Adam step has moments: the three-step test)
    finally:
        a1.close(); a2.close()


def test_pad_rows_carry_no_gradient_behind_rows_of_a_training_step(golden, golden_seg):
    """The rows buffer behind NB holds what an earlier training step wrote there (9 N = 2250 > NB = 490): the chains evaluate those rows of the last
    tile like any other, and they must carry zero gradient.  A five-frame handle (train_steps needs the video): the LAST of its five pre-train steps is
    held from the kernels' own tiles — the zeros, the masks, the seed, the weight gradients over every row of the live tiles."""
    P = state("S", golden, golden_seg)
    for mlp_mode in (1, 3):
        af, _ = TA.make_fit("S", golden, golden_seg, mlp_mode=mlp_mode, batch=TA.BATCH)
        try:
            assert int(af.cfg.pretrain_batch) == 500
            TA.load_flat(af, P)
            af.train_steps(0, 1, TA.step_inds(af, 12), return_losses=False)
            af.set_debug(True)
            F = int(af.cfg.number_of_frames)
            ys, xs = PR.draws(25, F, 500)
            loss = float(af.pre_train_mapping(1, ys, xs, return_losses=True)[-1])
            stale = CR.rows4_of(af.debug_tiles(0, "rows", 0, 500))[500:512]
            assert stale[:, :3].any(), "the pad rows of the last tile hold nothing: the case does not test what it is there for"
            tag = "S %s batch 500 behind a training step:" % MODES[mlp_mode]
            report(*check_pre_step(af, 0, None, F, F - 1, ys[-1], xs[-1], loss, mlp_mode, 1, tag, adam=False, forward=False), tag)
        finally:
            af.close()


@pytest.mark.parametrize("kind", ["S", "N"])
def test_three_steps_carry_the_moments_and_the_counter(kind, golden, golden_seg):
    """pre_train_mapping(3) on a one-frame handle is three steps of ONE optimizer (counters 1, 2, 3, moments carried).  The gradient of step k is
    af_get_last_grads of a k-iteration call from the same state (every call restarts the optimizer, so the k-iteration call repeats the first k steps
    bit for bit); the parameters of a call WITHOUT debug must equal an fp64 Adam replayed from the three gradients within the summed adam_bounds.  A
    counter that restarted or moments zeroed per step move the result by about lr: orders of magnitude outside."""
    NB = 272
    P = state(kind, golden, golden_seg)
    ys, xs = PR.draws(26, 3, NB)
    a, net = make(kind, golden, golden_seg, F=1, batch=NB, mlp_mode=1)
    b, _ = make(kind, golden, golden_seg, F=1, batch=NB, mlp_mode=1)
    try:
        grads, after = [], []
        for k in (1, 2, 3):
            TA.load_flat(a, P); a.set_debug(True)
            a.pre_train_mapping(k, ys[:k], xs[:k], net=net)
            grads.append(a.last_grads(net)); after.append(a.get_params_flat(net))
        TA.load_flat(b, P)
        b.pre_train_mapping(3, ys, xs, net=net)
        got = b.get_params_flat(net)
        assert TA._same(got, after[2]), "the debug switch changed the parameters"
        p = P[net].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p); bound = np.zeros_like(p)
        for k, g in enumerate(grads, 1):
            bound += R.adam_bounds(p, m, v, g, k)[0]
            p, m, v = R.adam_fp64(p, m, v, g, k)
            err = np.abs(after[k - 1].astype(np.float64) - p)
            print("%s after step %d: worst parameter error / summed bound %.4f" % (kind, k, float((err / bound).max())), flush=True)
        err = np.abs(got.astype(np.float64) - p)
        assert np.all(err <= bound), (kind, "parameters after three steps of one call", int((~(err <= bound)).sum()), float((err / bound).max()))
        # what the bound tells apart: the same three gradients through an optimizer that restarts at every step
        q = P[net].astype(np.float64)
        for g in grads:
            q = R.adam_fp64(q, 0.0 * q, 0.0 * q, g, 1)[0]
        moved = np.abs(q - p)
        print("%s: a restarted optimizer differs by up to %.3g (lr 1e-4), %.3g x the bound there" % (kind, moved.max(), float((moved / bound).max())), flush=True)
        assert float((moved / bound).max()) > 100.0
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("mlp_mode", [1, 3])
def test_a_sample_on_its_target_has_a_zero_seed(mlp_mode, golden, golden_seg):
    """l == 0: the output layer zeroed (o = tanh(0) = 0 on every row) and one draw at x = y = half_main, whose row is (0, 0, t): its seed is exactly 0
    (torch's norm: the zero subgradient), the loss is finite and no NaN flag is raised (the call returns)."""
    import aiod_amd
    NB, resx, resy = 16, 42, 30
    P = {n: p.copy() for n, p in state("S", golden, golden_seg).items()}
    af, net = make("S", golden, golden_seg, F=1, batch=NB, mlp_mode=mlp_mode, resx=resx, resy=resy)
    try:
        tens = {name: sl for name, sl, _ in TA.tensors_of(af, net)}
        last = len(aiod_amd.atlasfit.imlp_shapes(net, af.cfg)) - 1
        P[net][tens["hidden.%d.weight" % last]] = 0.0; P[net][tens["hidden.%d.bias" % last]] = 0.0
        ys, xs = PR.draws(27, 1, NB, resx, resy)
        ys[0, 3] = 21; xs[0, 3] = 21
        loss = one_step(af, net, P, ys, xs)
        assert np.isfinite(loss) and loss > 0
        rows = CR.rows4_of(af.debug_tiles(net, "rows", 0, NB))
        assert rows[3].view(np.uint32)[:2].tolist() == [0, 0] and rows[3, 2] == -1.0
        assert not CR.rows4_of(af.debug_tiles(net, "out", 0, NB))[:NB].any()
        dout = CR.rows4_of(af.debug_tiles(net, "dout", 0, NB))
        assert not dout[3].any(), ("the seed of the sample on its target", dout[3])
        assert np.isfinite(dout).all() and np.isfinite(af.get_params_flat(net)).all()
        tag = "S %s batch 16, output layer zeroed:" % MODES[mlp_mode]
        report(*check_pre_step(af, net, P, 1, 0, ys[0], xs[0], loss, mlp_mode, 1, tag, res=(resx, resy)), tag)
    finally:
        af.close()


SEEDS = (0, 5, 2 ** 32 + 7)


@pytest.mark.parametrize("F,mlp_mode,resx,resy", [(1, 1, PR.RESX, PR.RESY), (3, 3, PR.RESY, PR.RESX)])
def test_the_device_sampler_draws_what_the_twin_draws(F, mlp_mode, resx, resy, golden, golden_seg):
    """pre_train_mapping(1, seed=S) without draws: the last step's rows are pre_prep_rows of rand_below(S, s, n, 1, resy) / rand_below(S, s, n, 2, resx),
    s the step index, bit for bit.  The three-frame handle is a portrait one (half_main = resy / 2) and runs the 32-row chains."""
    NB = 272
    P = state("S", golden, golden_seg)
    af, net = make("S", golden, golden_seg, F=F, batch=NB, mlp_mode=mlp_mode, resx=resx, resy=resy)
    try:
        for seed in SEEDS:
            TA.load_flat(af, P); af.set_debug(True)
            loss = float(af.pre_train_mapping(1, seed=seed, net=net, return_losses=True)[-1])
            s = F - 1
            ys, xs = PR.rand_below(seed, s, NB, 1, resy), PR.rand_below(seed, s, NB, 2, resx)
            assert ys.max() < resy and xs.max() < resx
            tag = "S %s seed %d, step %d of %d:" % (MODES[mlp_mode], seed, s, F)
            st, sd = check_pre_step(af, net, P if F == 1 else None, F, s, ys, xs, loss, mlp_mode, 1, tag, adam=F == 1, forward=F == 1, res=(resx, resy))
            report(st, sd, tag)
    finally:
        af.close()
