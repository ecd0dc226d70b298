"""tests/chain_ref.py checked without the kernels: numpy emulations of one layer in the three arithmetics of the chains — an fp32 sequential fma
chain (mlp.hip), the three-bf16 split with six products (mlpbf.hip; the split and the product order of tests/test_split_precision.py), the two-fp16
split with a scale per row, 2^12 on the weights and three products (mlphf.hip) — stay INSIDE chain_ref's bounds at every entry, forward and backward,
on seeded tensors of the narrow (N) and shipped (S) layer shapes, with one row spanning 2^24 and with a weight matrix scaled by 2^-10; and every
mutation a kernel could suffer leaves them on at least one entry: one k-term dropped, the bias added twice, the h l product dropped (f16x3), one row
scale off by a factor of 2, a row shifted by one, two output columns swapped, a mask taken from the neighbouring layer, sin and cos swapped in one
octave, the PE skip columns omitted.  tests/test_gpu_chain_entries.py holds the kernels' own tiles to the same bounds.

Measured here (numpy, these draws): the clean emulations reach 0.003-0.08 of the bound (a worst-case bound: (K + c) u against a typical sqrt(K) u);
numpy-fp32 sin / cos stay within 1.21 u and tanh within 1.02 u of fp64 — half of chain_ref's C_FN / C_TANH, as their derivation says."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_ref as CR  # noqa: E402
import test_split_precision as SP  # noqa: E402

U = CR.U
ARITH = {0: "fp32 fma chain", 1: "bf16x6", 3: "f16x3"}
# (name, units, hidden columns, PE skip columns): the hidden layers of N (mapping 40 wide, atlas 200 wide + 24 skip columns) and S (256, 256 + 40)
SHAPES = [("N mapping", 40, 40, 0), ("N atlas skip", 200, 200, 24), ("S hidden", 256, 256, 0), ("S atlas skip", 256, 256, 40)]
ROWS = 96


def f32(a):
    return np.asarray(a, np.float32)


def _fma(a, b, c):
    """fp32 fma of fp32 arrays: the product is exact in fp64; one rounding of the sum to fp64 in front of the fp32 one (innocuous double rounding)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chain32(X, W, b, drop=None):
    """acc = b; acc = fma(w_k, x_k, acc) for k in order: the fp32 matrix pipe.  drop: a k that is skipped."""
    acc = np.broadcast_to(f32(b), (X.shape[0], W.shape[0])).copy()
    for k in range(X.shape[1]):
        if k != drop:
            acc = _fma(X[:, k:k + 1], W[None, :, k], acc)
    return acc


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(f32(a)))


def prod_bf(X, Wh):
    return SP.contract_x6(_t(X), _t(Wh.T)).numpy()


def split_f16(x, s):
    h = (x * s).astype(np.float16).astype(np.float32)
    l = (x * s - h).astype(np.float16).astype(np.float32)
    return h, l


def row_scale(X):
    mx = np.abs(X).max(1)
    e = np.where(mx > 0, 15 - np.frexp(np.where(mx > 0, mx, 1.0))[1], 0)
    return np.ldexp(np.float32(1), e).astype(np.float32)[:, None]


def prod_hf(X, Wh, drop_hl=False, scale_off_row=None):
    """(W x) as mlphf.hip forms it: l h + h l + h h of the scaled operands in fp32, then the scale removed.  Returns (acc, 1 / (s 2^12)) so that the
    caller's epilogue is ONE fma."""
    s = row_scale(X)
    xh, xl = split_f16(f32(X), s)
    wh, wl = split_f16(f32(Wh), np.float32(4096))
    acc = _t(xh) @ _t(wl).T
    if not drop_hl:
        acc = acc + _t(xl) @ _t(wh).T
    acc = (acc + _t(xh) @ _t(wh).T).numpy()
    inv = (1.0 / (s * 4096)).astype(np.float32)
    if scale_off_row is not None:
        inv = inv.copy(); inv[scale_off_row] *= 2
    return acc, inv


def emulate_pre(mode, X, W, b, hid, drop=None, bias_twice=False, drop_hl=False, scale_off_row=None, no_skip=False):
    """Z of a hidden layer (hid columns on arithmetic `mode`, the PE skip columns behind them on the fp32 pipe) as fp32."""
    X, W, b = f32(X), f32(W), f32(b)
    Xh, Wh = X[:, :hid].copy(), W[:, :hid].copy()
    if drop is not None and drop < hid and mode != 0:
        Xh[:, drop] = 0
    K = hid if no_skip else X.shape[1]
    if mode == 0:
        Z = chain32(X[:, :K], W[:, :K], b, drop)
    else:
        if mode == 1:
            Z = prod_bf(Xh, Wh)
            if K > hid:
                Z = chain32(X[:, hid:K], W[:, hid:K], Z, None if drop is None or drop < hid else drop - hid)
            Z = Z + b
        else:
            acc, inv = prod_hf(Xh, Wh, drop_hl, scale_off_row)
            if K > hid:         # the skip columns land in the same scaled accumulators: B = 2^12 s pe (exact powers of two)
                acc = chain32(X[:, hid:K] / inv, W[:, hid:K], acc, None if drop is None or drop < hid else drop - hid)
            Z = _fma(acc, inv, np.broadcast_to(b, acc.shape))
    if bias_twice:
        Z = Z + b
    return Z


def draw(shape, variant, seed):
    """(X, W, b, hid) of a hidden layer: X = relu activations (+ PE-like columns in [-1, 1]), nn.Linear-sized weights."""
    _, o, hid, npe = shape
    rng = np.random.default_rng(seed)
    X = np.maximum(rng.standard_normal((ROWS, hid)) * 0.5 + 0.1, 0.0)
    if variant == "wide row":            # one row spanning 2^24, as the mapping net's gradient rows do
        X[7] = np.abs(X[7]) * 2.0 ** rng.uniform(-24, 0, hid)
        X[7, 3] = 1.5
    W = rng.uniform(-1, 1, (o, hid + npe)) / np.sqrt(hid + npe)
    if variant == "small weights":
        W *= 2.0 ** -10
    if npe:
        X = np.concatenate([X, np.sin(rng.uniform(-3, 3, (ROWS, npe)))], axis=1)
    b = rng.uniform(-1, 1, o) / np.sqrt(hid + npe)
    return f32(X), f32(W), f32(b), hid


def outside(got, ref, bound):
    return int((~(np.abs(got.astype(np.float64) - ref) <= bound)).sum())


@pytest.mark.parametrize("variant", ["plain", "wide row", "small weights"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_clean_emulations_stay_inside(mode, shape, variant):
    X, W, b, hid = draw(shape, variant, 11)
    ref, bound = CR.forward_layer(W, b, X, mode, hid)
    got = np.maximum(emulate_pre(mode, X, W, b, hid), 0)
    ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    assert outside(got, ref, bound) == 0, (ARITH[mode], shape[0], variant, ratio)
    # backward through the same weights: dZ rows spanning many decades, gated by the activations of the layer below
    rng = np.random.default_rng(12)
    dz = f32(rng.standard_normal((ROWS, W.shape[0])) * 10.0 ** rng.uniform(-6, 0, (ROWS, 1)) * (rng.random((ROWS, W.shape[0])) > 0.5))
    if variant == "wide row":
        dz[7] = dz[7] * 2.0 ** rng.uniform(-24, 0, dz.shape[1]); dz[7, 2] = 0.3
    gate = X[:, :hid]
    bref, bbound, _ = CR.backward_layer(dz, W[:, :hid], gate, mode)
    bgot = emulate_back(mode, dz, W[:, :hid]) * (gate > 0)
    bratio = float((np.abs(bgot - bref)[bbound > 0] / bbound[bbound > 0]).max())
    assert outside(bgot, bref, bbound) == 0, (ARITH[mode], shape[0], variant, bratio)
    assert not bgot[gate == 0].any()
    print("%s, %s, %s: worst error / bound forward %.4f backward %.4f" % (ARITH[mode], shape[0], variant, ratio, bratio))


def emulate_back(mode, dz, Wh, drop=None):
    """dz W (no bias; the accumulators start at zero)."""
    z = np.zeros(Wh.shape[1], np.float32)
    dzz = dz.copy()
    if drop is not None:
        dzz[:, drop] = 0
    if mode == 0:
        return chain32(dz, Wh.T.copy(), z, drop)
    if mode == 1:
        return prod_bf(dzz, Wh.T.copy())
    acc, inv = prod_hf(dzz, Wh.T.copy())
    return acc * inv


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_every_mutation_leaves_the_bounds(mode, shape):
    X, W, b, hid = draw(shape, "plain", 21)
    ref, bound = CR.forward_layer(W, b, X, mode, hid)
    clean = np.maximum(emulate_pre(mode, X, W, b, hid), 0)
    assert outside(clean, ref, bound) == 0
    seen = {}
    seen["k-term dropped"] = outside(np.maximum(emulate_pre(mode, X, W, b, hid, drop=hid // 2), 0), ref, bound)
    seen["bias twice"] = outside(np.maximum(emulate_pre(mode, X, W, b, hid, bias_twice=True), 0), ref, bound)
    seen["row shifted"] = outside(np.roll(clean, 1, axis=0), ref, bound)
    sw = clean.copy(); sw[:, [4, 5]] = sw[:, [5, 4]]
    seen["columns swapped"] = outside(sw, ref, bound)
    if shape[3]:
        seen["skip columns omitted"] = outside(np.maximum(emulate_pre(mode, X, W, b, hid, no_skip=True), 0), ref, bound)
        seen["skip k-term dropped"] = outside(np.maximum(emulate_pre(mode, X, W, b, hid, drop=hid + 3), 0), ref, bound)
    if mode == 3:
        seen["h l product dropped"] = outside(np.maximum(emulate_pre(mode, X, W, b, hid, drop_hl=True), 0), ref, bound)
        seen["row scale off by 2"] = outside(np.maximum(emulate_pre(mode, X, W, b, hid, scale_off_row=9), 0), ref, bound)
    # backward: a dropped k-term, a shifted row, swapped columns, and the gate of the neighbouring layer (a stale mask)
    rng = np.random.default_rng(22)
    dz = f32(rng.standard_normal((ROWS, W.shape[0])) * 1e-3)
    gate = X[:, :hid]
    other = np.roll(gate, 1, axis=1)                    # another layer's activation pattern
    bref, bbound, _ = CR.backward_layer(dz, W[:, :hid], gate, mode)
    raw = emulate_back(mode, dz, W[:, :hid])
    assert outside(raw * (gate > 0), bref, bbound) == 0
    seen["backward k-term dropped"] = outside(emulate_back(mode, dz, W[:, :hid], drop=W.shape[0] // 2) * (gate > 0), bref, bbound)
    seen["backward row shifted"] = outside(np.roll(raw * (gate > 0), 1, axis=0), bref, bbound)
    seen["mask of the neighbouring layer"] = outside(raw * (other > 0), bref, bbound)
    for name, n in seen.items():
        assert n > 0, (ARITH[mode], shape[0], name, "not detected")
    print("%s, %s: entries outside the bound: %s" % (ARITH[mode], shape[0], ", ".join("%s %d" % kv for kv in seen.items())))


def _bits_as_the_kernels_write_them(acts_tile):
    """mlp.hip relu_out restated literally for one tile (32 rows, 256 features): lane (j, h), register e = 16 T + r <-> feature 32 T + 8 (r >> 2) + 4 h +
    (r & 3); word T >> 1, the sign of (0 - v) shifted in from the right, register by register."""
    words = np.zeros((64, 4), np.uint32)
    for lane in range(64):
        j, h = lane & 31, lane >> 5
        for T in range(8):
            for r in range(16):
                v = acts_tile[j, 32 * T + 8 * (r >> 2) + 4 * h + (r & 3)]
                words[lane, T >> 1] = ((int(words[lane, T >> 1]) << 1) & 0xFFFFFFFF) | int(v > 0)
    return words


def test_mask_layout_and_a_stale_mask():
    rng = np.random.default_rng(3)
    a0 = np.maximum(rng.standard_normal((64, 256)), 0); a1 = np.maximum(rng.standard_normal((64, 256)), 0)
    w0 = np.stack([_bits_as_the_kernels_write_them(a0[:32]), _bits_as_the_kernels_write_them(a0[32:])])
    assert np.array_equal(CR.mask_bits(w0), a0 > 0)
    assert np.array_equal(CR.mask_words(a0 > 0), w0)
    assert np.array_equal(CR.mask_bits(w0, 40), (a0 > 0)[:40])
    assert not np.array_equal(CR.mask_bits(CR.mask_words(a1 > 0)), a0 > 0)            # the neighbouring layer's words
    one = (a0 > 0).copy(); one[33, 200] ^= True                                        # a single wrong bit is seen
    assert (CR.mask_bits(CR.mask_words(one)) != (a0 > 0)).sum() == 1
    # hf_mask_keep<E>: bit 31 - ((E >> 4) & 1) 16 - (E & 15) of word E >> 5 is the same bit
    for E in range(128):
        assert 31 - ((E >> 4) & 1) * 16 - (E & 15) == 31 - (E & 31)


def pe32(x, nfreq, swap_octave=None, octave_shift=0):
    """chain_input in numpy fp32: p = fl(x b_k), b_k = 2^k fl32(pi); (n, 2 d nfreq) in the reference's feature order."""
    x = f32(x)
    out = np.zeros((x.shape[0], nfreq, 2, x.shape[1]), np.float32)
    for k in range(nfreq):
        p = x * np.ldexp(np.float32(np.pi), k + octave_shift)
        s, c = np.sin(p), np.cos(p)
        out[:, k, 0], out[:, k, 1] = (c, s) if k == swap_octave else (s, c)
    return out.reshape(x.shape[0], -1)


def test_positional_encoding_bound_and_its_mutations():
    rng = np.random.default_rng(5)
    # xyt rows (mapping nets with PE, alpha): three inputs, five octaves
    x = f32(rng.uniform(-1, 1, (500, 3)))
    ref, bound = CR.pe_ref(x, 5, CR.C_ARG_XYT)
    assert ref.shape == (500, 30) and outside(pe32(x, 5), ref, bound) == 0
    # the atlas net: x = v 0.5 + 0.5 of the mapping net's fp32 outputs, contracted to an fma or not; also a scale that is not a power of two
    v = f32(np.tanh(rng.standard_normal((500, 2))))
    for scale, shift in ((0.5, 0.5), (0.5, -0.5), (0.3, 0.1)):
        xr, slack = CR.atlas_input(v, float(np.float32(scale)), float(np.float32(shift)))
        assert bool(slack.any()) == (scale != 0.5)
        ref, bound = CR.pe_ref(xr, 10, CR.C_ARG_ATLAS, slack)
        fused = _fma(v, np.full_like(v, scale), np.full_like(v, shift))
        plain = (v * np.float32(scale)).astype(np.float32) + np.float32(shift)
        for xin in (fused, plain):
            got = pe32(xin, 10)
            assert outside(got, ref, bound) == 0, (scale, shift, float((np.abs(got - ref) / bound).max()))
        if scale == 0.5:
            assert np.array_equal(fused, plain)               # the shipped scale: the multiplication is exact, both forms agree
            worst = float((np.abs(pe32(fused, 10) - ref) / bound).max())
    # the function's own error at these arguments: half of C_FN, as its derivation says
    for k in range(10):
        p = (fused * np.ldexp(np.float32(np.pi), k)).astype(np.float32)
        for fn in (np.sin, np.cos):
            assert float(np.abs(fn(p).astype(np.float64) - fn(p.astype(np.float64))).max()) <= 0.5 * CR.C_FN * U
    # mutations: sin and cos swapped in one octave, a wrong octave, a wrong slot
    xr, _ = CR.atlas_input(v, 0.5, 0.5); ref, bound = CR.pe_ref(xr, 10, CR.C_ARG_ATLAS); xin = _fma(v, np.full_like(v, 0.5), np.full_like(v, 0.5))
    for k in (0, 4, 9):
        assert outside(pe32(xin, 10, swap_octave=k), ref, bound) > 0
    assert outside(pe32(xin, 10, octave_shift=1), ref, bound) > 0
    assert outside(np.roll(pe32(xin, 10), 1, axis=1), ref, bound) > 0
    # the same through the identities (nets whose input rows are not exposed)
    x = f32(rng.uniform(-1, 1, (500, 3)))
    for name, val, want, b in CR.pe_identities(pe32(x, 5), 3, 5, CR.C_ARG_XYT):
        assert outside(val, want, b) == 0, name
    for bad in (pe32(x, 5, swap_octave=2), np.roll(pe32(x, 5), 1, axis=1), pe32(x, 5)[:, ::-1]):
        assert sum(outside(val, want, b) for _, val, want, b in CR.pe_identities(bad, 3, 5, CR.C_ARG_XYT)) > 0
    print("atlas PE in numpy fp32, shipped scale: worst error / bound %.3f" % worst)


def test_output_layer_seed_and_whole_net():
    rng = np.random.default_rng(8)
    hid, npe = 256, 40
    X = f32(np.concatenate([np.maximum(rng.standard_normal((ROWS, hid)) * 0.5, 0), np.sin(rng.uniform(-3, 3, (ROWS, npe)))], axis=1))
    W = f32(rng.uniform(-1, 1, (3, hid + npe)) / np.sqrt(hid + npe)); b = f32(rng.uniform(-0.1, 0.1, 3))
    ref, bound = CR.output_layer(W, b, X)
    z = chain32(X, W, b)
    assert outside(np.tanh(z), ref, bound) == 0
    assert outside(np.tanh(chain32(X, W, b, drop=100)), ref, bound) > 0
    assert outside(np.tanh(chain32(X[:, :hid], W[:, :hid], b)), ref, bound) > 0           # the skip columns of an output layer omitted
    assert outside(z, ref, bound) > 0                                                     # no tanh
    zz = np.abs(rng.uniform(-9, 9, 1000000)).astype(np.float32)
    assert float(np.abs(np.tanh(zz).astype(np.float64) - np.tanh(zz.astype(np.float64))).max()) <= 0.5 * CR.C_TANH * U
    # the seed
    o = np.tanh(z); dout = f32(rng.standard_normal(o.shape) * 10.0 ** rng.uniform(-8, 0, o.shape)); dout[5] = 0
    sref, sbound = CR.seed(o, dout)
    got = dout * (np.float32(1) - o * o)
    assert got.dtype == np.float32 and outside(got, sref, sbound) == 0
    assert not got[5].any() and not sbound[5].any()
    assert outside(dout * (np.float32(1) - o), sref, sbound) > 0
    assert outside(dout * (np.float32(1) - o * o) * (np.float32(1) + np.float32(4 * U)), sref, sbound) > 0      # four roundings too many
    # a whole (small) net: per-layer fp32 emulation against the propagated bound of net_forward
    shapes = [(40, 18), (40, 40), (40, 40 + 18), (2, 40)]
    flat = f32(np.concatenate([np.concatenate([rng.uniform(-1, 1, o * k) / np.sqrt(k), rng.uniform(-1, 1, o) / np.sqrt(k)]) for o, k in shapes]))
    layers = CR.unflatten(flat, shapes)
    x = f32(rng.uniform(-1, 1, (ROWS, 3)))
    pe = pe32(x, 3)
    oref, E = CR.net_forward(layers, pe, pe, 0)
    a = pe
    for l, (Wl, bl) in enumerate(layers):
        if Wl.shape[1] > 40:
            a = np.concatenate([a, pe], axis=1)
        a = chain32(a, f32(Wl), f32(bl))
        a = np.tanh(a) if l == len(layers) - 1 else np.maximum(a, 0)
    assert outside(a, oref, E) == 0 and float(E.max()) < 1e-4
