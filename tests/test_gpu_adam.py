"""k_adam (csrc/elem.hip) element by element: the split-K sum, the Adam update and every weight view the chains read.

The update.  One training step from a set state (parameters, exp_avg, exp_avg_sq, step) with debug on; the kernel's OWN reduced gradient
(af_get_last_grads: what k_adam summed from the partial blocks and fed to the update) goes into an fp64 Adam (tests/adam_ref.py), so the update is
held apart from the gradient's round-off.  Every element of p, m and v must lie within adam_bounds — the COUNTED fp32 round-off of the formulation,
which torch.optim.Adam's own fp32 step stays inside (tests/test_adam_ref_host.py) — and every state-dict tensor's max / rms error within twice
torch-fp32's (or one fp32 ulp of the tensor's largest magnitude).  Steps 1, 4, 2, 100 000 and 2^31 + 6 of the counter; zero moments, the moments three
real steps leave, and synthetic moments over eleven decades; one hidden unit of mapping1 dead (bias -100: exactly zero gradients on its incoming
row, its bias and its outgoing column).  Three configurations: S the shipped single-atlas nets, T the shipped two-layer nets, N a narrow single-atlas
architecture (widths 40 and 200, 3 and 6 layers, mapping PE with 3 frequencies, 6 atlas frequencies; each feature is one tests/test_gpu_arch.py trains),
all on a 37x21x5 video with samples_batch 250 (the last row tile of every net padded).

The views.  The fp32 forward and W^T images, the bias image and the 16-bit streams of the arithmetic in force are written by k_adam as a side effect
of the update; a stale or misplaced view shows nowhere in the parameters.  After three steps handle A's (parameters, moments, step) go into a fresh
handle B: forward outputs (forward views, bias image), the loss record, the next step's gradients and parameters (W^T views, 16-bit streams) must be
equal bit for bit.  The same after every af_set_mlp_mode switch of the cycle 3 -> 1 -> 2 -> 0 -> 3 and across af_set_dw_mode 1 -> 0 -> 2 -> 1.

pre_train_mapping runs its own optimizer (unwrap_utils.py:178): the loop's moments and step are untouched by it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NARROW = dict(number_of_channels_mapping1=40, number_of_layers_mapping1=3, use_positional_encoding_mapping1=True, number_of_positional_encoding_mapping1=3,
              number_of_channels_atlas=200, number_of_layers_atlas=6, positional_encoding_num_atlas=6)
KINDS = {"S": (False, {}), "T": (True, {}), "N": (False, NARROW)}
BATCH = 250
DEAD_LAYER, DEAD_UNIT = 1, 5          # of mapping1
_videos, _starts = {}, {}


def _video(two_layer, flow="constant"):
    from oracle import atlas_oracle as O
    if (two_layer, flow) not in _videos:
        _videos[two_layer, flow] = (O.synthetic_seg_video if two_layer else O.synthetic_video)(37, 21, 5, seed=4, flow=flow)
    return _videos[two_layer, flow]


def make_fit(kind, golden, golden_seg, mlp_mode=3, dw_mode=1, batch=BATCH, flow="constant"):
    """(AtlasFit, config dict) of configuration `kind` with the video uploaded and the arithmetic modes set.  batch: samples_batch; flow: the kind of
    synthetic video (oracle.synthetic_video)."""
    import aiod_amd
    two, over = KINDS[kind]
    cfg = dict((golden_seg if two else golden)["config"]); cfg.update(over); cfg.update(samples_batch=batch)
    v = _video(two, flow)
    af = aiod_amd.AtlasFit(aiod_amd.default_config(v.resx, v.resy, v.F, cfg, two_layer=two, pretrain_batch=500))
    vid = [v.video_frames, v.optical_flows, v.optical_flows_reverse, v.optical_flows_mask, v.optical_flows_reverse_mask]
    af.upload_video(*(vid + ([v.mask_frames] if two else [])))
    af.set_mlp_mode(mlp_mode); af.set_dw_mode(dw_mode)
    return af, cfg


def tensors_of(af, net):
    """[(state-dict key, slice into the flat vector, shape)] of a net."""
    import aiod_amd
    out, off = [], 0
    for i, (o, k) in enumerate(aiod_amd.atlasfit.imlp_shapes(net, af.cfg)):
        out.append(("hidden.%d.weight" % i, slice(off, off + o * k), (o, k))); off += o * k
        out.append(("hidden.%d.bias" % i, slice(off, off + o), (o,))); off += o
    assert off == af.param_count(net)            # the flat buffers have the configured sizes
    return out


def dead_entries(af):
    """Flat indices of mapping1 whose gradient torch computes as exactly 0 for the dead unit: its incoming row, its bias, its outgoing column."""
    t = {name: (sl, shp) for name, sl, shp in tensors_of(af, 0)}
    (sw, (o, k)), (sb, _) = t["hidden.%d.weight" % DEAD_LAYER], t["hidden.%d.bias" % DEAD_LAYER]
    sn, (o2, k2) = t["hidden.%d.weight" % (DEAD_LAYER + 1)]
    idx = np.concatenate([sw.start + DEAD_UNIT * k + np.arange(k), [sb.start + DEAD_UNIT], sn.start + np.arange(o2) * k2 + DEAD_UNIT])
    assert idx.size == k + 1 + o2
    return idx


def load_flat(af, params, adam=None, step=0):
    """Parameters (and the optimizer state) of every net from flat vectors.  The step counter is handle-wide: every af_set_adam_state call sets it,
    the last one wins — all nets are given the same value."""
    import aiod_amd
    for net in af.nets:
        af.load_state_dict(net, aiod_amd.atlasfit.unflatten_state_dict(params[net], net, af.cfg))
        z = np.zeros(af.param_count(net), np.float32)
        m, v = adam[net] if adam is not None else (z, z)
        af.set_adam_state(net, m, v, step)


def step_inds(af, seed, k=1, batch=BATCH):
    c = af.cfg
    g = torch.Generator().manual_seed(seed)
    return torch.randint(c.number_of_frames * c.resx * c.resy, (k, batch), generator=g).numpy()


def start_state(kind, golden, golden_seg):
    """Seeded nets, mapping nets pre-trained 40 iterations, mapping1's unit dead (P0); and the parameters / moments three real steps later (P3, A3)."""
    import aiod_amd
    from oracle import atlas_oracle as O
    if kind in _starts:
        return _starts[kind]
    af, cfg = make_fit(kind, golden, golden_seg)
    try:
        models = O.build_seg_models(cfg, seed=2) if af.two_layer else O.build_single_atlas_models(cfg, seed=2)
        for net, m in zip(af.nets, models):
            af.load_state_dict(net, m.state_dict())
        af.pre_train_mapping(40, seed=5)
        if af.two_layer:
            af.pre_train_mapping(40, seed=6, net=aiod_amd.NET_MAPPING2)
        P0 = {net: af.get_params_flat(net) for net in af.nets}
        t = {name: sl for name, sl, _ in tensors_of(af, 0)}
        P0[0][t["hidden.%d.bias" % DEAD_LAYER].start + DEAD_UNIT] = -100.0        # biases are not range-checked
        load_flat(af, P0)
        af.train_steps(0, 3, step_inds(af, 11, 3), return_losses=False)
        P3 = {net: af.get_params_flat(net) for net in af.nets}
        A3 = {net: af.adam_state(net)[:2] for net in af.nets}
        assert af.adam_state(0)[2] == 3
    finally:
        af.close()
    _starts[kind] = dict(P0=P0, P3=P3, A3=A3)
    return _starts[kind]


def _stats(d):
    d = np.abs(d.astype(np.float64))
    return float(d.max()), float(np.sqrt((d * d).mean()))


CASES = [("zero", 0), ("real", 3), ("synthetic", 1), ("synthetic", 99999), ("synthetic", 2 ** 31 + 5)]


@pytest.mark.parametrize("moments,t0", CASES)
@pytest.mark.parametrize("kind,mlp_mode", [("S", 0), ("S", 1), ("S", 3), ("T", 3), ("N", 3)])
def test_one_step_element_by_element(kind, mlp_mode, moments, t0, golden, golden_seg):
    st = start_state(kind, golden, golden_seg)
    af, _ = make_fit(kind, golden, golden_seg, mlp_mode=mlp_mode)
    try:
        rng = np.random.default_rng(t0 % 9973)
        P = st["P3"] if moments == "real" else st["P0"]
        if moments == "zero":
            adam = {net: (np.zeros_like(P[net]), np.zeros_like(P[net])) for net in af.nets}
        elif moments == "real":
            adam = st["A3"]
        else:
            adam = {net: R.synthetic_moments(rng, P[net].size) for net in af.nets}       # mixed signs of m
        load_flat(af, P, adam, t0)
        af.set_debug(True)
        af.train_steps(0, 1, step_inds(af, 12))
        dead = dead_entries(af)
        worst = {"p": 0.0, "m": 0.0, "v": 0.0}
        for net in af.nets:
            g, p1 = af.last_grads(net), af.get_params_flat(net)
            m1, v1, t1 = af.adam_state(net)
            assert t1 == t0 + 1, (t0, t1)                                  # also beyond 2^31
            p0, (m0, v0) = P[net], adam[net]
            ref = R.adam_fp64(p0, m0, v0, g, t0 + 1)
            t32 = R.adam_torch32(p0, m0, v0, g, t0 + 1)
            bounds = R.adam_bounds(p0, m0, v0, g, t0 + 1)
            tens = tensors_of(af, net)
            for what, got, want, ref32, b in zip("pmv", (p1, m1, v1), ref, t32, bounds):
                err = np.abs(got.astype(np.float64) - want)
                worst[what] = max(worst[what], float((err / b).max()))
                bad = np.flatnonzero(~(err <= b))
                assert bad.size == 0, (kind, mlp_mode, moments, t0, "net %d" % net, what, "%d elements outside the fp32 round-off bound" % bad.size,
                                       bad[:5], err[bad[:5]], b[bad[:5]])
                for name, sl, shp in tens:
                    hm, hr = _stats(got[sl] - want[sl]); rm, rr = _stats(ref32[sl] - want[sl])
                    ulp = float(np.spacing(np.float32(np.abs(want[sl]).max())))
                    assert hm <= max(2 * rm, ulp) and hr <= max(2 * rr, ulp), (kind, mlp_mode, moments, t0, "net %d" % net, name, what,
                                                                              "hip max %.3g rms %.3g, torch fp32 max %.3g rms %.3g, ulp %.3g" % (hm, hr, rm, rr, ulp))
                    last = sl.stop - 1                                     # the last real row and column of the layer
                    assert err[last] <= b[last], (net, name, what)
            # ---- elements whose gradient is exactly zero
            z = g == 0
            if net == 0:
                assert z[dead].all(), ("non-zero gradient on the dead unit", g[dead][g[dead] != 0][:5])
                assert z.sum() >= dead.size
            still = z & (m0 == 0) & (v0 == 0)
            for got, was in ((p1, p0), (m1, m0), (v1, v0)):
                assert np.array_equal(got[still].view(np.uint32), was[still].view(np.uint32))     # nothing to decay, nothing to move: unchanged bit for bit
            dec = z & ((m0 != 0) | (v0 != 0))
            if dec.any():      # torch does not skip such parameters: the moments decay and the weight moves by the momentum term
                assert np.all(np.abs(m1[dec].astype(np.float64) - 0.9 * m0[dec].astype(np.float64)) <= bounds[1][dec])
                assert np.all(np.abs(v1[dec].astype(np.float64) - 0.999 * v0[dec].astype(np.float64)) <= bounds[2][dec])
                moved = dec & (np.abs(ref[0] - p0) > 2 * np.spacing(np.abs(p0)))
                assert np.all(p1[moved] != p0[moved])
            if net == 0 and moments == "synthetic":
                assert dec[dead].all()
        print("%s mlp_mode %d, %s moments, step %d: worst error / bound: p %.3f m %.3f v %.3f" % (kind, mlp_mode, moments, t0 + 1, worst["p"], worst["m"], worst["v"]))
    finally:
        af.close()


def _snapshot(af):
    return ({net: af.get_params_flat(net) for net in af.nets}, {net: af.adam_state(net)[:2] for net in af.nets}, af.adam_state(af.nets[0])[2])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _hold_equal(A_, B_, it, seed, what):
    """Forward outputs, then one debug step on both handles with the same indices: loss record, gradients, parameters and moments, bit for bit."""
    rows = np.random.default_rng(seed).uniform(-1.0, 1.0, (1000, 4)).astype(np.float32)
    for net in A_.nets:
        assert _same(A_.debug_forward(net, rows), B_.debug_forward(net, rows)), (what, "forward views / bias image of net %d" % net)
    inds = step_inds(A_, seed)
    A_.set_debug(True); B_.set_debug(True)
    la, lb = A_.train_steps(it, 1, inds), B_.train_steps(it, 1, inds)
    assert _same(la, lb), (what, "loss record", la, lb)
    for net in A_.nets:
        assert _same(A_.last_grads(net), B_.last_grads(net)), (what, "gradients of net %d (W^T views, 16-bit streams)" % net)
        assert _same(A_.get_params_flat(net), B_.get_params_flat(net)), (what, "parameters of net %d" % net)
        for x, y in zip(A_.adam_state(net)[:2], B_.adam_state(net)[:2]):
            assert _same(x, y), (what, "moments of net %d" % net)
    assert A_.adam_state(A_.nets[0])[2] == B_.adam_state(B_.nets[0])[2]


MLP_CYCLE = (3, 1, 2, 0)


@pytest.mark.parametrize("start_mode", [0, 1, 3])
@pytest.mark.parametrize("kind", ["S", "T", "N"])
def test_views_follow_the_parameters(kind, start_mode, golden, golden_seg):
    st = start_state(kind, golden, golden_seg)
    A_, _ = make_fit(kind, golden, golden_seg, mlp_mode=start_mode)
    others = []
    try:
        load_flat(A_, st["P0"])
        A_.train_steps(0, 3, step_inds(A_, 13, 3), return_losses=False)
        P, adam, step = _snapshot(A_)
        assert step == 3
        B_, _ = make_fit(kind, golden, golden_seg, mlp_mode=start_mode); others.append(B_)
        load_flat(B_, P, adam, step)
        _hold_equal(A_, B_, 3, 14, "after 3 steps in mode %d" % start_mode)
        B_.close()
        # the cycle 3 -> 1 -> 2 -> 0 -> 3 entered at the starting mode; 1 -> 2 stays inside the bf16 stream family (nothing is re-emitted, nothing may be stale)
        k = MLP_CYCLE.index(start_mode)
        for i in range(1, 5):
            mode = MLP_CYCLE[(k + i) % 4]
            A_.set_mlp_mode(mode)
            P, adam, step = _snapshot(A_)
            C_, _ = make_fit(kind, golden, golden_seg, mlp_mode=mode); others.append(C_)
            load_flat(C_, P, adam, step)
            _hold_equal(A_, C_, 3 + i, 14 + i, "after the switch to mode %d (from %d)" % (mode, MLP_CYCLE[(k + i - 1) % 4]))
            C_.close()
    finally:
        A_.close()
        for o in others:
            o.close()


def test_views_follow_the_parameters_across_dw_modes(golden, golden_seg):
    st = start_state("S", golden, golden_seg)
    A_, _ = make_fit("S", golden, golden_seg, dw_mode=1)
    others = []
    try:
        load_flat(A_, st["P0"])
        A_.train_steps(0, 3, step_inds(A_, 13, 3), return_losses=False)
        for i, mode in enumerate((0, 2, 1)):
            A_.set_dw_mode(mode)
            P, adam, step = _snapshot(A_)
            C_, _ = make_fit("S", golden, golden_seg, dw_mode=mode); others.append(C_)
            load_flat(C_, P, adam, step)
            _hold_equal(A_, C_, 3 + i, 20 + i, "after the switch to dw mode %d" % mode)
            C_.close()
    finally:
        A_.close()
        for o in others:
            o.close()


@pytest.mark.parametrize("kind", ["S", "T", "N"])
def test_pre_train_mapping_leaves_the_loop_optimizer_alone(kind, golden, golden_seg):
    import aiod_amd
    st = start_state(kind, golden, golden_seg)
    af, _ = make_fit(kind, golden, golden_seg)
    try:
        rng = np.random.default_rng(5)
        adam = {net: R.synthetic_moments(rng, st["P0"][net].size) for net in af.nets}
        load_flat(af, st["P0"], adam, 7)
        af.pre_train_mapping(1, seed=9)
        if af.two_layer:
            af.pre_train_mapping(1, seed=10, net=aiod_amd.NET_MAPPING2)
        pre = (aiod_amd.NET_MAPPING1, aiod_amd.NET_MAPPING2) if af.two_layer else (aiod_amd.NET_MAPPING1,)
        for net in af.nets:
            m, v, step = af.adam_state(net)
            assert step == 7
            assert _same(m, adam[net][0]) and _same(v, adam[net][1]), "pre_train_mapping touched the loop's moments of net %d" % net
            assert _same(af.get_params_flat(net), st["P0"][net]) == (net not in pre)         # it trained its own net and no other
    finally:
        af.close()
