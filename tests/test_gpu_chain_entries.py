"""Every tile the forward and backward chains leave behind (csrc/mlp.hip, mlpbf.hip, mlphf.hip; mlp_common.h), per ENTRY, against the fp64 layer twin of
tests/chain_ref.py — recomputed from the kernels' OWN inputs (the parameters the step ran on and the tile one layer down / up), so each layer, net and
tile position is held on its own:

    PE tile             atlas: from the mapping net's output rows (af_debug_tiles "out") through in_scale / in_shift, every octave the kernel writes;
                        alpha: from the xyt rows of mapping1 ("x0": k_prep writes the same (x, y, t) to both nets' rows);
                        a mapping net with PE: from its own xyt rows in k_prep's buffer ("rows"), and through its identities — sin^2 + cos^2 = 1
                        and every octave against the angle recovered from the lowest one
    layer 0             the xyt pass-through (the "x0" tile) or the PE tile, fp32 pipe in every mode
    hidden layers       acts[l] = relu(W_l acts[l-1] + b_l), a skip layer on cat([acts, PE]); padding units (o >= width) exactly 0
    output layer        o = tanh(.) on v_mfma_f32_4x4x1_f32 ("out"), columns past the net's outputs exactly 0
    mask words          bit = [acts > 0], the lane / word layout of chain_ref.mask_bits
    seed                dz_last = dout (1 - o^2) from the kernel's own o and dout ("dout")
    backward            dz[l-1] = (dz[l] W_l[:, :hid]) [acts[l-1] > 0], exactly 0 where the kernel's own activation is 0; the top product through the
                        output weights
    tail rows           rows of the last tile behind the live rows: the kernels compute them like any other row from whatever the input buffers hold
                        (mlp_common.h chain_rows / TileStore: only tiles past the last live one are dropped) and the contract is the one host.hip
                        states — "pad rows of the last tile must carry zero gradient": dz_last and every dz plane exactly 0 there
    dead unit           mapping1's unit with bias -100: acts 0 on every row, mask bits clear, dz 0 in its column

for every net of the handle, kinds S, T, N of tests/test_gpu_adam.py (37x21x5 video, samples_batch 250: the last row tile of every net is partly
padding; a skip layer, both PE layouts, a narrow zero-padded net, all four nets) x mlp_mode 0, 1, 3.  The bounds are DERIVED (chain_ref's docstring),
30-100x above the typical error: a dropped k-term, a shifted row or column, a stale mask word break them by orders of magnitude.  The figures
printed per tensor class (rms and worst error in units of 2^-24 of the class's denominator, worst error / bound) are figures, not assertions.

Scaled weights (kind S, modes 3 and 0): hidden layer 2 of each net times 2^-10, then rescaled to max |w| = 4 — half the documented limit of the fp16
weight images; nothing here goes nearer — with the layer's bias scaled alike (a pure scale of its activations) and the next layer's hidden columns
divided by the same factor, as far as that keeps THEIR max |w| <= 4 (for 2^-10 the full inverse would be 2^10 x 0.06 = 64, outside the range: the
rest stays uncompensated and the outputs shrink, still inside tanh's range).  The same bounds; af_train_steps must return 0, not AF_ERANGE.

Inference chain (af_debug_forward: FIN 2, another epilogue), from the parameters the step ran on (loaded again: the step has moved them), on the
step's own input rows — xyt nets: the "x0" rows; atlas: fl32(v in_scale + in_shift); alpha: the mapping rows k_prep writes the same (x, y, t) to; a
mapping net with PE: its own "rows", and seeded rows over [-1, 1]^3 with the first check only:
  * within the per-layer bounds PROPAGATED through the fp64 forward of the whole net (chain_ref.net_forward: E_l = bound_l + |W_l| E_{l-1}).  Rigorous
    and therefore loose — |W| sums to ~8 per layer, the bound reaches 10^-2 .. 10^1 at the outputs: it sees a broken epilogue, not a lost bit;
  * within ONE output-layer bound of the training step's outputs: the two chains run the same fp32 operations in the same order (FIN 1 differs from
    FIN 2 by recording the sign bit), so the rows are expected bit-equal (the count is printed); this is the check that bites."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_ref as CR  # noqa: E402
import test_gpu_adam as TA  # noqa: E402

pytestmark = pytest.mark.gpu
U = CR.U
MODES = {0: "fp32 MFMA", 1: "bf16x6", 3: "f16x3"}
CLASSES = ("PE", "layer 0", "hidden", "skip layer", "output", "seed", "backward", "top backward")


class Stats:
    def __init__(self):
        self.d = {}

    def hold(self, tag, cls, got, ref, bound, den):
        """Assert |got - ref| <= bound at every entry; record the class's figures (error / den in units of 2^-24, error / bound)."""
        got = np.asarray(got, np.float64)
        err = np.abs(got - ref)
        bad = np.argwhere(~(err <= bound))
        nz = np.asarray(den) > 0
        rel = (err[nz] / np.asarray(den)[nz]) / U if nz.any() else np.zeros(1)
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
        s = self.d.setdefault(cls, [0.0, 0, 0.0, 0.0])
        s[0] += float((rel * rel).sum()); s[1] += rel.size; s[2] = max(s[2], float(rel.max())); s[3] = max(s[3], ratio)
        assert bad.size == 0, (tag, cls, "%d of %d entries outside the bound; first at (row, column) %s: kernel %.9g fp64 %.9g bound %.3g, worst error / bound %.3g"
                               % (len(bad), err.size, tuple(bad[0]), got[tuple(bad[0])], np.asarray(ref)[tuple(bad[0])], np.asarray(bound)[tuple(bad[0])], ratio))

    def report(self, tag):
        for cls in CLASSES:
            if cls in self.d:
                ss, n, worst, ratio = self.d[cls]
                print("%s %-13s (units of 2^-24): rms %.3f worst %.2f, worst error / bound %.4f" % (tag, cls, np.sqrt(ss / max(n, 1)), worst, ratio), flush=True)


def _live_rows(af, losses):
    """{net: (rows of the net's batch, live rows)} as tests/test_gpu_dw_entries.py check_step."""
    import aiod_amd
    A = aiod_amd.atlasfit
    names = af.LOSS_NAMES_TWO_LAYER if af.two_layer else af.LOSS_NAMES
    live = int(losses[names.index("valid_fwd")] + losses[names.index("valid_bwd")])
    rows4, _ = af.step_work(0)
    N = af.N
    out = {}
    for net in af.nets:
        cap = rows4[net]
        R_ = {A.NET_MAPPING1: cap - 2 * N + live, A.NET_MAPPING2: cap - 2 * N + live, A.NET_ATLAS: cap, A.NET_ALPHA: 3 * N + live}[net]
        assert 0 < R_ <= cap
        out[net] = (cap, R_)
    return out


def _atlas_rows_in(af, rows, R_):
    """The atlas net's input rows of the step: (v fp32 (R_, 2), in_shift per row) from the mapping nets' output rows."""
    import aiod_amd
    A = aiod_amd.atlasfit
    N = af.N
    cap1 = rows[A.NET_MAPPING1][0]
    v1 = CR.rows4_of(af.debug_tiles(A.NET_MAPPING1, "out", 0, cap1, 0, (3 * N + 31) // 32))[:3 * N, :2]
    if not af.two_layer:
        assert R_ == 3 * N
        return v1, np.full(R_, 0.5)
    cap2 = rows[A.NET_MAPPING2][0]
    v2 = CR.rows4_of(af.debug_tiles(A.NET_MAPPING2, "out", 0, cap2, 0, (3 * N + 31) // 32))[:3 * N, :2]
    assert R_ == 6 * N
    return np.concatenate([v1, v2]), np.concatenate([np.full(3 * N, 0.5), np.full(3 * N, -0.5)])


def check_chains(af, P, losses, mode, tag, infer=True):
    """One debug step at iteration 0 has run on `af` from the parameters P: hold every tile of every net.  Returns the Stats."""
    import aiod_amd
    A = aiod_amd.atlasfit
    st = Stats()
    rows = _live_rows(af, losses)
    todo = []
    for net in af.nets:
        cap, R_ = rows[net]
        nt = (R_ + 31) // 32
        shapes = A.imlp_shapes(net, af.cfg)
        layers = CR.unflatten(P[net], shapes)
        nl, hid, enc, nout = len(shapes), shapes[0][0], shapes[0][1], shapes[-1][0]
        xyt = net in (A.NET_MAPPING1, A.NET_MAPPING2) and enc == 3
        t = "%s net %d" % (tag, net)
        full = lambda which, l=0: CR.rows_of(af.debug_tiles(net, which, l, cap, 0, nt))      # noqa: E731   every row of the live tiles
        acts = [full("acts", l) for l in range(nl - 1)]
        dz = [full("dz", l) for l in range(nl - 1)]
        dzl = full("dz_last")
        out = CR.rows4_of(af.debug_tiles(net, "out", 0, cap, 0, nt))
        dout = CR.rows4_of(af.debug_tiles(net, "dout", 0, cap, 0, nt))
        # ---- the input stage
        pe = None
        if xyt:
            x0t = full("x0")
            assert not x0t[:, 3:].any(), (t, "x0 tile: features behind xyt")
            X = x0t[:R_, :3]
            x_inf = np.zeros((R_, 4), np.float32); x_inf[:, :3] = X
        else:
            pet = full("pe")
            d = 2 if net == A.NET_ATLAS else 3
            nfreq = 10 if d == 2 else 5                         # what the kernel writes (chain_input), whatever the net's own frequency count
            assert enc <= 2 * d * nfreq and not pet[:, 2 * d * nfreq:].any(), (t, "PE tile: slots behind the last feature")
            if net == A.NET_ATLAS:
                v, sh = _atlas_rows_in(af, rows, R_)
                x64 = v.astype(np.float64) * 0.5 + sh[:, None]
                ref, bound = CR.pe_ref(x64, nfreq, CR.C_ARG_ATLAS)
                st.hold(t + " PE tile", "PE", pet[:R_, :4 * nfreq], ref, bound, np.ones_like(ref))
                x_inf = np.zeros((R_, 4), np.float32); x_inf[:, :2] = v * np.float32(0.5) + sh[:, None].astype(np.float32)      # one rounding: the device's
            elif net == A.NET_ALPHA and A.imlp_shapes(A.NET_MAPPING1, af.cfg)[0][1] == 3:
                # k_prep (elem.hip put_row / put_row_at) writes one (x, y, t) to the mapping nets' row and to alpha's: alpha rows [0, 3N) are mapping
                # rows [0, 3N), alpha's flow-match rows 3N + i are mapping rows 7N + i (the ninth-segment batch of iteration 0)
                c1, _ = rows[A.NET_MAPPING1]
                N = af.N
                assert c1 == 9 * N
                m1 = CR.rows_of(af.debug_tiles(A.NET_MAPPING1, "x0", 0, c1, 0, (c1 + 31) // 32))[:, :3]
                x64 = np.concatenate([m1[:3 * N], m1[7 * N:7 * N + R_ - 3 * N]])
                ref, bound = CR.pe_ref(x64, nfreq, CR.C_ARG_XYT)
                st.hold(t + " PE tile", "PE", pet[:R_, :6 * nfreq], ref, bound, np.ones_like(ref))
                x_inf = np.zeros((R_, 4), np.float32); x_inf[:, :3] = x64
            else:
                for name, val, want, bound in CR.pe_identities(pet[:R_], d, nfreq, CR.C_ARG_XYT):
                    st.hold(t + " PE tile, " + name, "PE", val, want, bound, np.ones_like(want))
                # and against the net's own xyt rows as k_prep wrote them ("rows"; tests/test_gpu_step_rows.py holds those rows themselves)
                xr = CR.rows4_of(af.debug_tiles(net, "rows", 0, cap, 0, nt))[:R_]
                assert not xr[:, 3].any(), (t, "input rows: the fourth column")
                ref, bound = CR.pe_ref(xr[:, :3].astype(np.float64), nfreq, CR.C_ARG_XYT)
                st.hold(t + " PE tile", "PE", pet[:R_, :6 * nfreq], ref, bound, np.ones_like(ref))
                x_inf = np.zeros((R_, 4), np.float32); x_inf[:, :3] = xr[:, :3]
            pe = pet[:R_, :enc]
            X = pe
        # ---- forward
        for l in range(nl - 1):
            W, b = layers[l]
            if l > 0:
                X = acts[l - 1][:R_, :hid]
                if W.shape[1] > hid:
                    X = np.concatenate([X, pe], axis=1)
            ref, bound = CR.forward_layer(W, b, X, mode, None if l == 0 else hid)
            den = np.abs(X) @ np.abs(W).T + np.abs(b)
            cls = "layer 0" if l == 0 else ("skip layer" if W.shape[1] > hid else "hidden")
            st.hold("%s acts[%d]" % (t, l), cls, acts[l][:R_, :hid], ref, bound, den)
            assert not acts[l][:, hid:].any(), (t, l, "activation on a padding unit")
            bits = CR.mask_bits(af.debug_tiles(net, "masks", l, cap, 0, nt), R_)
            wrong = np.argwhere(bits != (acts[l][:R_] > 0))
            assert wrong.size == 0, (t, "mask words of layer %d: %d bits differ from [acts > 0]; first at (row, feature) %s" % (l, len(wrong), tuple(wrong[0])))
        W, b = layers[-1]
        X = acts[nl - 2][:R_, :hid]
        if W.shape[1] > hid:
            X = np.concatenate([X, pe], axis=1)
        ref, bound = CR.output_layer(W, b, X)
        bound_out = bound
        st.hold(t + " outputs", "output", out[:R_, :nout], ref, bound, np.abs(X) @ np.abs(W).T + np.abs(b))
        assert not out[:R_, nout:].any(), (t, "output columns behind the net's outputs")
        # ---- backward
        ref, bound = CR.seed(out[:R_, :nout], dout[:R_, :nout])
        st.hold(t + " dz_last", "seed", dzl[:R_, :nout], ref, bound, np.abs(dout[:R_, :nout].astype(np.float64)))
        assert not dzl[:, nout:].any(), (t, "dz_last: rows behind the net's outputs")
        ref, bound, rowmax = CR.backward_layer(dzl[:R_, :nout], layers[-1][0][:, :hid], acts[nl - 2][:R_, :hid], mode, fp32_pipe=True)
        st.hold("%s dz[%d]" % (t, nl - 2), "top backward", dz[nl - 2][:R_, :hid], ref, bound, np.abs(dzl[:R_, :nout]) @ np.abs(layers[-1][0][:, :hid]))
        for l in range(nl - 2, 0, -1):
            Wh = layers[l][0][:, :hid]
            ref, bound, rowmax = CR.backward_layer(dz[l][:R_, :hid], Wh, acts[l - 1][:R_, :hid], mode, rowmax=rowmax)
            st.hold("%s dz[%d]" % (t, l - 1), "backward", dz[l - 1][:R_, :hid], ref, bound, np.abs(dz[l][:R_, :hid]) @ np.abs(Wh))
        for l in range(nl - 1):
            assert not dz[l][:, hid:].any(), (t, l, "gradient on a padding unit")
            assert not dz[l][R_:].any(), (t, l, "gradient on a row behind the live rows")
        assert not dzl[R_:].any(), (t, "dz_last on a row behind the live rows")
        if net == A.NET_MAPPING1:
            assert not acts[TA.DEAD_LAYER][:, TA.DEAD_UNIT].any(), (t, "the dead unit is active")
            assert not CR.mask_bits(af.debug_tiles(net, "masks", TA.DEAD_LAYER, cap, 0, nt))[:, TA.DEAD_UNIT].any(), (t, "mask bit of the dead unit")
            assert not dz[TA.DEAD_LAYER][:, TA.DEAD_UNIT].any(), (t, "gradient on the dead unit")
        todo.append((net, t, layers, x_inf, out[:R_, :nout].astype(np.float64), bound_out, xyt, enc, nout))
    # ---- the inference chain (FIN 2) on the same rows, from the parameters the step ran on (the step has moved them: loaded again)
    if infer:
        TA.load_flat(af, P)
        for net, t, layers, x_step, o_train, bound_out, xyt, enc, nout in todo:
            runs = [(x_step, True)]
            if not xyt and net in (A.NET_MAPPING1, A.NET_MAPPING2):      # a mapping net with PE: seeded rows over the whole of [-1, 1]^3 as well (the first check only)
                x_seed = np.zeros((700, 4), np.float32)
                x_seed[:, :3] = np.random.default_rng(31 + net).uniform(-1.0, 1.0, (700, 3)).astype(np.float32)
                runs.append((x_seed, False))
            for x_inf, step_rows in runs:
                got = af.debug_forward(net, x_inf)
                if xyt:
                    x0 = x_inf[:, :3].astype(np.float64); pe64 = None; E0 = None
                else:
                    d = 2 if net == A.NET_ATLAS else 3
                    pe64, E0 = CR.pe_ref(x_inf[:, :d].astype(np.float64), enc // (2 * d), CR.C_ARG_XYT)       # af_debug_forward: in_scale 1, in_shift 0 (exact)
                    x0 = pe64
                o64, E = CR.net_forward(layers, x0, pe64, mode, E0)
                d64 = np.abs(got[:, :nout].astype(np.float64) - o64)
                assert np.all(d64 <= E), (t, "inference chain against the fp64 net", float((d64 / E).max()))
                assert not got[:, nout:].any()
                msg = "%s inference chain: worst distance from the fp64 net %.2f u (propagated worst-case bound %.3g u)" % (t, d64.max() / U, E.max() / U)
                if step_rows:
                    dtr = np.abs(got[:, :nout].astype(np.float64) - o_train)
                    assert np.all(dtr <= bound_out), (t, "inference chain against the training step's outputs", float((dtr / bound_out).max()))
                    msg += ", from the training step's outputs %.2f u (%d of %d rows bit-equal)" % (dtr.max() / U, int((dtr.max(1) == 0).sum()), len(dtr))
                print(msg, flush=True)
    return st


def _step_rc(af, inds):
    """af_train_steps of one step at iteration 0 through the C entry point itself: (return code, loss record)."""
    import aiod_amd
    A = aiod_amd.atlasfit
    losses = np.zeros((1, af.loss_width), np.float32)
    inds = np.ascontiguousarray(inds, np.int64)
    rc = af.lib.af_train_steps(af.h, 0, 1, A._ptr(inds), 0, A._ptr(losses))
    return rc, losses[0]


def _debug_step(af, P):
    TA.load_flat(af, P)
    af.set_debug(True)
    rc, losses = _step_rc(af, TA.step_inds(af, 12))
    assert rc == 0, (rc, af.lib.af_last_error(af.h).decode())
    return losses


@pytest.mark.parametrize("mlp_mode", [0, 1, 3])
@pytest.mark.parametrize("kind", ["S", "T", "N"])
def test_every_tile_entry_of_both_chains(kind, mlp_mode, golden, golden_seg):
    st0 = TA.start_state(kind, golden, golden_seg)
    af, _ = TA.make_fit(kind, golden, golden_seg, mlp_mode=mlp_mode)
    try:
        losses = _debug_step(af, st0["P0"])
        st = check_chains(af, st0["P0"], losses, mlp_mode, "%s %s" % (kind, MODES[mlp_mode]))
        st.report("%s %s:" % (kind, MODES[mlp_mode]))
    finally:
        af.close()


SCALED_LAYER = 2


def _scaled(af, P0, how):
    """P0 with hidden layer SCALED_LAYER of every net (weights and bias) scaled — by 2^-10, or to max |w| = 4 — and the next layer's hidden columns
    divided by the same factor as far as their own max |w| stays <= 4 (powers of two: the scaling itself is exact)."""
    import aiod_amd
    A = aiod_amd.atlasfit
    P = {}
    for net in af.nets:
        shapes = A.imlp_shapes(net, af.cfg)
        hid = shapes[0][0]
        assert len(shapes) > SCALED_LAYER + 2 and shapes[SCALED_LAYER][1] == hid and shapes[SCALED_LAYER + 1][1] == hid       # two plain hidden layers
        flat = P0[net].copy()
        tens = {name: (sl, shp) for name, sl, shp in TA.tensors_of(af, net)}
        sw, _ = tens["hidden.%d.weight" % SCALED_LAYER]; sb, _ = tens["hidden.%d.bias" % SCALED_LAYER]
        sn, _ = tens["hidden.%d.weight" % (SCALED_LAYER + 1)]
        wmax = float(np.abs(flat[sw]).max())
        f = 2.0 ** -10 if how == "2^-10" else 2.0 ** np.floor(np.log2(4.0 / wmax))
        g = min(1.0 / f, 2.0 ** np.floor(np.log2(4.0 / float(np.abs(flat[sn]).max()))))
        flat[sw] *= np.float32(f); flat[sb] *= np.float32(f); flat[sn] *= np.float32(g)
        if how != "2^-10":
            assert 2.0 < float(np.abs(flat[sw]).max()) <= 4.0
        assert float(np.abs(flat[sn]).max()) <= 4.0 and float(np.abs(flat[sw]).max()) <= 4.0
        P[net] = flat
    return P


@pytest.mark.parametrize("how", ["2^-10", "max 4"])
@pytest.mark.parametrize("mlp_mode", [3, 0])
def test_scaled_hidden_layers_hold_the_same_bounds(mlp_mode, how, golden, golden_seg):
    st0 = TA.start_state("S", golden, golden_seg)
    af, _ = TA.make_fit("S", golden, golden_seg, mlp_mode=mlp_mode)
    try:
        P = _scaled(af, st0["P0"], how)
        losses = _debug_step(af, P)                               # asserts the return code: 0, not AF_ERANGE
        assert np.isfinite(losses).all()
        st = check_chains(af, P, losses, mlp_mode, "S %s, layer %d %s" % (MODES[mlp_mode], SCALED_LAYER, how))
        st.report("S %s, layer %d scaled %s:" % (MODES[mlp_mode], SCALED_LAYER, how))
    finally:
        af.close()
