"""Every gradient tensor of a training step per ENTRY: k_dw's narrow jobs (csrc/dw.hip: the 8x2, 8x1, 1x8 and 1x2 job shapes — PE and xyt first
layers, PE skip columns, output layers), every bias gradient, and the hidden blocks of the nets tests/test_gpu_gemm_error.py never reaches (mapping2,
alpha, zero-padded narrow nets), recomputed in fp64 from the kernels' OWN tiles (af_debug_tiles) and compared with af_get_last_grads:

    db_l[o]    = sum_r dZ_l[r][o]                      dW_l[o][i] = sum_r dZ_l[r][o] X_l[r][i]
    X_0 = the xyt rows or the PE tile, X_l = relu(Z_{l-1}) (a skip layer: cat([X_l, PE])), dZ of the output layer from the dz_last tile.

Per entry |hip - fp64| <= B sum_r |dZ[r][o] X[r][i]|, B = (R + nslots_max) 2^-24 in dw modes 0 (fp32 MFMA) and 1 (bf16x6): the worst case of an fp32
sum of the R live rows of the net in that step plus the split-K slot sum of k_adam (bf16x6's dropped terms, <= 2^-23 per product —
tests/test_split_precision.py — are absorbed); mode 2 (two bf16 per operand, 2^-16 each) adds 2^-15.  The bound is derived, not measured: one dropped
row of R breaks it on a typical entry by ~1 / (R^2 2^-24) (>= 3x at R = 2250, 30x at R = 750), a swapped or shifted entry by orders of magnitude.
Entries whose bound is 0 (the dead unit of tests/test_gpu_adam.py, units no row activates) must be exactly 0.  The rms and worst error per tensor
are printed in units of 2^-24, as tests/test_gpu_gemm_error.py does; they are figures, not assertions.

The PE tile holds the features in the reference's feature order (mlp_common.h chain_input: "PE features in reference feature order"), which is the
column order of the state dict, so no permutation enters here; the slot order (af_pe_slot_of_feature, twin in tests/test_layout_model.py) belongs to
the weight IMAGES k_adam writes — tests/test_gpu_adam.py holds those through the forward outputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_adam as TA  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DW_NAMES = {0: "fp32 MFMA", 1: "bf16x6", 2: "bf16x3"}


def _rows(tiles, n):                # (nt, F, 32) T-layout tiles -> the first n rows, (n, F) fp64
    return np.ascontiguousarray(tiles).transpose(0, 2, 1).reshape(-1, tiles.shape[1])[:n].astype(np.float64)


def _slots_max(af, which=0):
    """Most split-K slots any job of schedule `which` has (0: the step's nine-segment iterations; 2 / 3: pre-training mapping1 / mapping2): what k_adam
    sums per entry."""
    seg = af.dw_schedule(which)
    jobs = seg[:, :, 3][seg[:, :, 0] >= 0]
    return int(np.bincount(jobs).max())


def check_net(af, net, cap, R_, slots, dw_mode, tag):
    """Every gradient tensor of one net from the kernels' own tiles of the last step: `cap` rows of the net's batch (its tile planes are ceil(cap / 32)
    tiles apart), of which the first R_ enter; `slots`: what k_adam sums per entry.  Returns the worst error / bound."""
    import aiod_amd
    A = aiod_amd.atlasfit
    worst_ratio = 0.0
    nt = (R_ + 31) // 32
    B = (R_ + slots) * U + (2.0 ** -15 if dw_mode == 2 else 0.0)
    shapes = A.imlp_shapes(net, af.cfg)
    nl, hid = len(shapes), shapes[0][0]
    enc = shapes[0][1]
    has_pe = not (net in (A.NET_MAPPING1, A.NET_MAPPING2) and enc == 3)
    grads = af.last_grads(net).astype(np.float64)
    tens = {name: (sl, shp) for name, sl, shp in TA.tensors_of(af, net)}
    pe = _rows(af.debug_tiles(net, "pe", 0, cap, 0, nt), R_)[:, :enc] if has_pe else None
    x0 = pe if has_pe else _rows(af.debug_tiles(net, "x0", 0, cap, 0, nt), R_)[:, :3]
    acts = {}
    for l in range(nl):
        o, k = shapes[l]
        if l < nl - 1:
            dz_full = _rows(af.debug_tiles(net, "dz", l, cap, 0, nt), R_)
            assert not dz_full[:, o:].any(), (tag, net, l, "gradient on a padding unit")
            acts_full = _rows(af.debug_tiles(net, "acts", l, cap, 0, nt), R_)
            assert not acts_full[:, o:].any(), (tag, net, l, "activation on a padding unit")
            acts[l] = acts_full[:, :o]
            dz = dz_full[:, :o]
        else:
            dz = _rows(af.debug_tiles(net, "dz_last", 0, cap, 0, nt), R_)[:, :o]
        X = x0 if l == 0 else acts[l - 1]
        if l > 0 and k > hid:                                    # a skip layer: cat([x, PE(input)]) (implicit_neural_networks.py:66-69)
            X = np.concatenate([X, pe], axis=1)
        assert X.shape[1] == k, (net, l, X.shape, k)
        acts.pop(l - 2, None)
        refs = {"hidden.%d.weight" % l: (dz.T @ X, np.abs(dz).T @ np.abs(X)), "hidden.%d.bias" % l: (dz.sum(0), np.abs(dz).sum(0))}
        for name, (ref, den) in refs.items():
            sl, shp = tens[name]
            got = grads[sl].reshape(shp)
            err = np.abs(got - ref)
            nz = den > 0
            assert not got[~nz].any(), (tag, "net %d" % net, name, "non-zero gradient where no row contributes")
            rel = err[nz] / den[nz] if nz.any() else np.zeros(1)
            ratio = float(rel.max() / B)
            worst_ratio = max(worst_ratio, ratio)
            blocks = [("", slice(None))] if name.endswith("bias") or k <= hid or l == 0 else [(" hidden block", slice(0, hid)), (" PE skip columns", slice(hid, k))]
            for bname, cs in blocks:
                e = (err[..., cs][nz[..., cs]] / den[..., cs][nz[..., cs]]) if nz[..., cs].any() else np.zeros(1)
                print("%s net %d %-16s%-17s %s (R %d, units of 2^-24): rms %.2f worst %.1f, worst / bound %.4f"
                      % (tag, net, name, bname, DW_NAMES[dw_mode], R_, float(np.sqrt((e * e).mean())) / U, float(e.max()) / U, float(e.max()) / B), flush=True)
            bad = np.argwhere(~(err <= B * den))
            assert bad.size == 0, (tag, "net %d" % net, name, DW_NAMES[dw_mode], "%d entries outside the bound; first at %s: hip %.9g fp64 %.9g, error / bound %.3g"
                                   % (len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])], ratio))
    if net == A.NET_MAPPING1:
        dead = TA.dead_entries(af)
        assert not grads[dead].any(), "non-zero gradient on the dead unit"
    return worst_ratio


def check_step(af, losses, dw_mode, tag):
    """One debug step at iteration 0 has run on `af` (`losses`: its loss record): recompute every tensor of every net and hold af_get_last_grads to the bound.  Returns the worst error / bound."""
    import aiod_amd
    A = aiod_amd.atlasfit
    names = af.LOSS_NAMES_TWO_LAYER if af.two_layer else af.LOSS_NAMES
    live = int(losses[names.index("valid_fwd")] + losses[names.index("valid_bwd")])
    rows4, _ = af.step_work(0)
    N = af.N
    slots = _slots_max(af)
    worst_ratio = 0.0
    for net in af.nets:
        cap = rows4[net]                                             # rows of the net's batch: its tile planes are ceil(cap / 32) tiles apart
        R_ = {A.NET_MAPPING1: cap - 2 * N + live, A.NET_MAPPING2: cap - 2 * N + live, A.NET_ATLAS: cap, A.NET_ALPHA: 3 * N + live}[net]
        assert 0 < R_ <= cap
        worst_ratio = max(worst_ratio, check_net(af, net, cap, R_, slots, dw_mode, tag))
    return worst_ratio


def _debug_step(af, st):
    TA.load_flat(af, st["P0"])
    af.set_debug(True)
    return af.train_steps(0, 1, TA.step_inds(af, 12))[0]


@pytest.mark.parametrize("dw_mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ["S", "T", "N"])
def test_every_gradient_tensor_per_entry(kind, dw_mode, golden, golden_seg):
    st = TA.start_state(kind, golden, golden_seg)
    af, _ = TA.make_fit(kind, golden, golden_seg, mlp_mode=3, dw_mode=dw_mode)
    try:
        w = check_step(af, _debug_step(af, st), dw_mode, kind)
        print("%s %s: worst error / bound over every tensor %.4f" % (kind, DW_NAMES[dw_mode], w))
    finally:
        af.close()


def test_other_split_k_partitions_per_entry(golden, golden_seg):
    """Two non-shipped cost rows (af_debug_set_dw_cost): other slot counts through k_adam's 8 / 4 / 2 / 1 summation tail.  The same bound."""
    st = TA.start_state("S", golden, golden_seg)
    af, _ = TA.make_fit("S", golden, golden_seg, mlp_mode=3, dw_mode=1)
    try:
        for part in ("306,150,126,129,87", "306,170,145,148,100"):
            af.set_dw_cost(part)
            w = check_step(af, _debug_step(af, st), 1, "S partition %s" % part)
            print("S bf16x6, partition %s: %d slots at most, worst error / bound %.4f" % (part, _slots_max(af), w))
        af.set_dw_cost(None)
    finally:
        af.close()
