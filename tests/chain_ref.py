"""The fp64 twin of ONE layer of the forward / backward chains (csrc/mlp.hip, mlpbf.hip, mlphf.hip, mlp_common.h) and the bound every entry of what
the kernels wrote must lie inside.  Plain numpy, no GPU: tests/test_chain_ref_host.py shows that emulations of the three arithmetics stay inside the
bounds and that a dropped k-term, a shifted row, a swapped column, a stale mask ... leave them; tests/test_gpu_chain_entries.py holds the kernels' tiles
(af_debug_tiles) to them.  Every function returns (reference, bound), both fp64, one value per entry; an entry is held as |kernel - reference| <= bound.

The operation (implicit_neural_networks.py:62-80 and the dX half of loss.backward()), per net:
    PE       feature 2 d k + i = sin(x_i 2^k pi), 2 d k + d + i = cos(x_i 2^k pi)   (d inputs, k = octave: the reference's feature order,
             mlp_common.h chain_input); x = the xyt rows (mapping nets with PE, alpha), or v in_scale + in_shift of the mapping net's output v (atlas)
    forward  Z_l = W_l X_l + b_l, X_0 = xyt rows or PE, X_l = relu(Z_{l-1}) = acts[l-1], a skip layer: cat([X_l, PE]); output o = tanh(Z_last)
    seed     dZ_last = dout (1 - o^2)
    backward dZ_{l-1} = (dZ_l W_l[:, :hid]) [acts[l-1] > 0], the top product through the output weights from dZ_last
    masks    bit of entry e = [acts > 0]

Units: u = 2^-24, the unit round-off of fp32.  den = sum_k |w_k x_k| (+ |b|): what every dot-product bound is stated in.

DERIVATION OF B_l (the relative part) — nothing here is fitted to a kernel's output.
  fp32 pipe (mode 0; and in EVERY mode layer 0, the PE columns of a skip layer, the output layers, the top backward product): v_mfma_f32_32x32x2_f32 /
    v_mfma_f32_4x4x1_f32 are fmaf chains (mlp.hip head: "exact fp32 fmaf chains").  K terms accumulated onto the bias in any order take at most K
    roundings on the way of any one term: |err| <= gamma_K den, gamma_K = K u / (1 - K u) <= (K + 1) u for K (K + 1) u <= 1, i.e. every K here.  The
    output layer's four partial chains, their pairwise sum, the lane exchange and the bias add are the same K + 1 additions in another order.
        B = (K + 1) u                                                                                                                     c = 1
  bf16x6 (mode 1, hidden 256 -> 256 products): operands split exactly into three bf16 (tests/test_split_precision.py: h + m + l = x to 2^-24, and in
    fact exactly while no level underflows), six of the nine partial products kept.  Dropped: m l + l m + l l <= (2 2^-9 2^-17 + 2^-34) |a b| < 2^-24
    |a b|; the contract the unit states (mlpbf.hip / include/atlasfit.h: "dropped terms <= 2^-23 relative") is the figure used.  The accumulation is
    the unit's admission rule: fp32-faithful, no more than an fp32 fmaf chain's (K + 1) u.
        B = (K + 1) u + 2^-23 = (K + 3) u                                                                                                 c = 3
  f16x3 (mode 3, hidden products; mlphf.hip head): each operand is two fp16 terms of its scaled value, |x s - h - l| <= 2^-24 |x s| while l is a
    normal fp16 — one split error per operand, 2 u per product; three of four partial products kept, the dropped l l <= 2^-11 2^-11 |a b| = 2^-22
    |a b| = 4 u.  The scales are powers of two and the epilogue (remove the scale, add the bias) is ONE fma: the bias rounding is the "+ 1" already
    counted.  Accumulation by the admission rule (tests/test_gpu_gemm_error.py holds it: no larger than the fp32 chain's) (K + 1) u.
        B = (K + 1) u + 2 u + 4 u = (K + 7) u                                                                                             c = 7
    (Counted to the last bit a split can leave 2^-23 |x s| on an element at the very bottom of its binade with an odd 24th bit; the head of the unit
    and this bound count the binade's top, 2^-24.  The emulation of tests/test_chain_ref_host.py contains such elements and stays inside.)
  A_l, f16x3 only — the two ABSOLUTE floors the head of mlphf.hip states, summed; they matter only where l has become an fp16 subnormal (spacing
    2^-24, error <= 2^-25 in scaled units):
      * an activation / gradient element more than 2^17 below its row's maximum: the row's scale puts the maximum into [2^14, 2^15), so 1 / s <=
        2^-14 rowmax and the element's error is <= 2^-25 / s <= 2^-39 rowmax, times the weights it meets: 2^-39 rowmax_r sum_k |w_ok|;
      * a weight below 2^-16 (fixed scale 2^12): error <= 2^-25 2^-12 = 2^-37, times the activations: 2^-37 sum_k |x_rk|.
    In the backward chain the row's scale comes from the UNMASKED product (mlphf.hip hf_finish: "the unmasked maximum bounds the masked one"):
    backward_layer takes that maximum from the fp64 product one layer up (plus its bound).
  K is the layer's number of input columns (hid, hid + PE columns of a skip layer, 3 or the PE width of layer 0; the layer's number of units in the
  backward direction).  For K = 256 a dropped k-term costs ~den / 256 = 2^16 u den / 2^8: 2^8 above the bound on a typical entry.

PE bound 2^-24 (c_arg |p| + c_fn), p = x 2^k pi:
  c_arg: the device forms p = fl(x b_k), b_k = 2^k fl32(pi).  fl32(pi) = pi (1 + 0.467 u); the product rounds once (1 u): c_arg = 1.5 for xyt inputs.
    The atlas net's x = v in_scale + in_shift rounds once more, relative to |x|, when contracted to an fma: c_arg = 2.5.  Not contracted, the
    multiplication rounds too, relative to |v in_scale| (NOT to |x|: the sum may cancel): one more u |v in_scale| b_k, absolute, unless in_scale is a
    power of two (the shipped 0.5), where it is exact and both forms agree bit for bit.  sin and cos are 1-Lipschitz, so the argument's error is
    the feature's.
  c_fn: the ulp bound of the device's sinf / cosf.  The ROCm installation carries no document that states it (nothing under its share/ or doc/
    directories gives ulp figures for the device math library), so this is the MEASURED alternative: numpy-fp32 sin / cos against fp64 on 8 10^7
    arguments x 2^k fl32(pi), |x| <= 1.5, k = 0..9 — worst 1.201 u — with a 2x margin: c_fn = 2.402.  tests/test_chain_ref_host.py re-measures it.
  c_tanh, by the same measurement (numpy-fp32 tanh against fp64 on |z| <= 9: worst 1.0113 u) and margin: 2.023.
  A swapped sin / cos, a wrong octave or a wrong slot is an error of order 1: seven orders of magnitude above the bound at the low octaves."""
import numpy as np

U = 2.0 ** -24
C = {0: 1.0, 1: 3.0, 3: 7.0}              # B = (K + C[mode]) u on a 16-bit-pipe product of that mode; the fp32 pipe is C[0] in every mode
C_FN = 2.402
C_TANH = 2.023
C_ARG_XYT, C_ARG_ATLAS = 1.5, 2.5
PI32 = float(np.float32(np.pi))


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------------
def rows_of(tiles, n=None):
    """(nt, F, 32) T-layout tiles [feature][row] -> (n, F) fp64 rows."""
    t = np.ascontiguousarray(tiles)
    r = t.transpose(0, 2, 1).reshape(-1, t.shape[1])
    return (r if n is None else r[:n]).astype(np.float64)


def rows4_of(tiles, n=None):
    """(nt, 32, 4) row-major tiles (the "out" / "dout" rows) -> (n, 4) fp32."""
    r = np.ascontiguousarray(tiles).reshape(-1, 4)
    return r if n is None else r[:n]


def _entry_feature():
    """Feature of register e = 16 T + 4 q + p of lane half h (af_dev.h C-layout, mlp_common.h store_tile_part): 32 T + 8 q + 4 h + p."""
    e = np.arange(128)
    T, q, p = e >> 4, (e >> 2) & 3, e & 3
    return np.stack([32 * T + 8 * q + 4 * h + p for h in (0, 1)])        # (2, 128)


_FEAT = _entry_feature()


def mask_bits(words, n=None):
    """(nt, 64, 4) uint32 sign-mask words -> (n, 256) bool.  Lane = 32 h + j owns row j of the tile; the bit of register e sits in word e >> 5 at bit
    31 - (e & 31) (mlp.hip relu_out, mlpbf.hip bf_mask_keep, mlphf.hip hf_sign_in / hf_mask_keep) and register e of lane half h is feature _FEAT[h, e]."""
    w = np.ascontiguousarray(words).astype(np.uint32).reshape(-1, 2, 32, 4)                # (nt, h, j, word)
    e = np.arange(128)
    bits = (w[:, :, :, e >> 5] >> (31 - (e & 31)).astype(np.uint32)) & 1                  # (nt, h, j, e)
    out = np.zeros((w.shape[0], 32, 256), bool)
    for h in (0, 1):
        out[:, :, _FEAT[h]] = bits[:, h].astype(bool)
    out = out.reshape(-1, 256)
    return out if n is None else out[:n]


def mask_words(bits):
    """The inverse of mask_bits: (32 nt, 256) bool -> (nt, 64, 4) uint32, as a forward chain writes them."""
    b = np.asarray(bits, bool).reshape(-1, 32, 256)
    w = np.zeros((b.shape[0], 2, 32, 4), np.uint32)
    e = np.arange(128)
    for h in (0, 1):
        v = b[:, :, _FEAT[h]].astype(np.uint32) << (31 - (e & 31)).astype(np.uint32)      # (nt, j, e)
        for k in range(4):
            w[:, h, :, k] = np.bitwise_or.reduce(v[:, :, 32 * k:32 * k + 32], axis=2)
    return w.reshape(-1, 64, 4)


# ---- positional encoding ------------------------------------------------------------------------------------------------------------------------
def pe_args(x, nfreq):
    """p[r, k, i] = x[r, i] 2^k pi in fp64, x (n, d)."""
    x = np.asarray(x, np.float64)
    return x[:, None, :] * (np.ldexp(np.pi, np.arange(nfreq)))[None, :, None]


def pe_ref(x, nfreq, c_arg, slack=None):
    """PE features of inputs x (n, d) in the reference's feature order, (n, 2 d nfreq), and the bound per entry.  slack (n, d): a magnitude whose
    one rounding the input carries besides those counted in c_arg (atlas_input)."""
    p = pe_args(x, nfreq)
    ref = np.concatenate([np.sin(p), np.cos(p)], axis=2).reshape(p.shape[0], -1)
    arg = c_arg * np.abs(p)
    if slack is not None:
        arg = arg + pe_args(np.abs(slack), nfreq)
    bound = U * (np.concatenate([arg, arg], axis=2).reshape(p.shape[0], -1) + C_FN)
    return ref, bound


def atlas_input(v, scale, shift):
    """The atlas net's input from the mapping net's output rows v (n, >= 2) fp32: (v scale + shift exact in fp64, the slack of pe_ref: |v scale|
    where the multiplication is not exact, else 0)."""
    v = np.asarray(v, np.float32)[:, :2].astype(np.float64)
    exact = np.frexp(abs(scale))[0] == 0.5
    return v * scale + shift, np.zeros_like(v) if exact else np.abs(v * scale)


def pe_identities(pe, d, nfreq, c_arg):
    """Where the input rows of a net are not exposed (mapping nets with PE, alpha: their xyt rows stay in k_prep's buffer) the PE tile is held through
    its identities.  Returns [(name, value, reference, bound)]:
      norm    sin^2 + cos^2 = 1 within 4 u: both functions see the SAME fp32 argument, so only the two function errors enter, each doubled by the
              square and weighted by |sin|, |cos| (the argument's own rounding does not);
      octave every octave k >= 1 against sin / cos of 2^k theta_0, theta_0 = atan2(sin_0, cos_0) the angle recovered from the lowest octave (|x| <= 1:
              p_0 = x pi lies in [-pi, pi], atan2 recovers it without wrap).  d theta_0 <= |d sin_0| + |d cos_0| <= 2 u (c_arg |p_0| + c_fn) propagates
              times 2^k; on top the entry's own bound u (c_arg |p_k| + c_fn)."""
    pe = np.asarray(pe, np.float64)[:, :2 * d * nfreq].reshape(-1, nfreq, 2, d)
    s, c = pe[:, :, 0, :], pe[:, :, 1, :]
    norm = s * s + c * c
    th0 = np.arctan2(s[:, 0, :], c[:, 0, :])                                   # (n, d)
    pk = th0[:, None, :] * np.ldexp(1.0, np.arange(nfreq))[None, :, None]      # (n, nfreq, d)
    own = U * (c_arg * np.abs(pk) + C_FN)
    dth = 2.0 * own[:, :1, :] * np.ldexp(1.0, np.arange(nfreq))[None, :, None]
    out = [("norm", norm, np.ones_like(norm), np.full_like(norm, 4.0 * U))]
    out.append(("octave sin", s[:, 1:], np.sin(pk[:, 1:]), (own + dth)[:, 1:]))
    out.append(("octave cos", c[:, 1:], np.cos(pk[:, 1:]), (own + dth)[:, 1:]))
    return out


# ---- layers -------------------------------------------------------------------------------------------------------------------------------------
def _f16_floor(Wh, Xh, rowmax):
    """A_l of the f16x3 arithmetic: 2^-39 rowmax_r sum_k |w_ok| + 2^-37 sum_k |x_rk| over the columns of the 16-bit product."""
    return 2.0 ** -39 * np.outer(rowmax, np.abs(Wh).sum(1)) + 2.0 ** -37 * np.abs(Xh).sum(1)[:, None]


def forward_pre(W, b, X, mode=0, hid=None):
    """Z = X W^T + b of one layer and the bound on it.  X (n, K) fp64 (the kernel's own input), W (o, K), b (o).  hid: the first `hid` columns run
    on the arithmetic `mode` (a hidden 256 -> 256 product); None: the whole layer is on the fp32 pipe (layer 0, output layers)."""
    W, b, X = np.asarray(W, np.float64), np.asarray(b, np.float64), np.asarray(X, np.float64)
    K = W.shape[1]
    assert X.shape[1] == K, (X.shape, W.shape)
    Z = X @ W.T + b
    den = np.abs(X) @ np.abs(W).T + np.abs(b)
    c = C[0] if hid is None else C[mode]
    bound = (K + c) * U * den
    if hid is not None and mode == 3:
        bound = bound + _f16_floor(W[:, :hid], X[:, :hid], np.abs(X[:, :hid]).max(1))
    return Z, bound


def forward_layer(W, b, X, mode=0, hid=None):
    """acts = relu(Z) and its bound (ReLU is 1-Lipschitz: an entry whose Z lies inside its own bound may land on either side of zero)."""
    Z, bound = forward_pre(W, b, X, mode, hid)
    return np.maximum(Z, 0.0), bound


def output_layer(W, b, X):
    """o = tanh(Z) of the output layer (fp32 pipe in every mode): B den + c_tanh u (tanh' <= 1: no amplification term)."""
    Z, bound = forward_pre(W, b, X)
    return np.tanh(Z), bound + C_TANH * U


def seed(o, dout):
    """dZ_last = dout (1 - o^2) from the kernel's own o and dout (n, OUT) fp32.  fl(o o) 1 u of o^2 <= 1, fl(1 - .) 1 u of a value <= 1, the
    product 1 u: |err| <= |dout| (u + u + u (1 - o^2) + second order) <= 3.001 u |dout|."""
    o, dout = np.asarray(o, np.float64), np.asarray(dout, np.float64)
    return dout * (1.0 - o * o), 3.001 * U * np.abs(dout)


def backward_layer(dz, Wh, acts_prev, mode=0, rowmax=None, fp32_pipe=False):
    """dZ_{l-1} = (dZ_l W_l[:, :hid]) [acts_{l-1} > 0], gated by the kernel's OWN activations; the bound is 0 where acts == 0: exactly 0 there.
    dz (n, o) fp64, Wh (o, hid).  fp32_pipe: the top product through the output weights.  rowmax: the row maxima that set the f16x3 row scale of dz
    (default: of dz itself).  Returns (reference, bound, rowmax of the UNMASKED product incl. its bound: what scales the next product down)."""
    dz, Wh = np.asarray(dz, np.float64), np.asarray(Wh, np.float64)
    K = Wh.shape[0]
    raw = dz @ Wh
    den = np.abs(dz) @ np.abs(Wh)
    bound = (K + (C[0] if fp32_pipe else C[mode])) * U * den
    if mode == 3 and not fp32_pipe:
        rm = np.abs(dz).max(1) if rowmax is None else np.maximum(rowmax, np.abs(dz).max(1))
        bound = bound + _f16_floor(Wh.T, dz, rm)
    gate = np.asarray(acts_prev) > 0
    nxt = (np.abs(raw) + bound).max(1)
    return raw * gate, bound * gate, nxt


# ---- a whole net --------------------------------------------------------------------------------------------------------------------------------
def unflatten(flat, shapes):
    """[(W, b)] fp64 of a net from its flat parameter vector (state-dict order) and imlp_shapes."""
    out, off = [], 0
    flat = np.asarray(flat)
    for o, k in shapes:
        W = flat[off:off + o * k].reshape(o, k).astype(np.float64); off += o * k
        b = flat[off:off + o].astype(np.float64); off += o
        out.append((W, b))
    assert off == flat.size
    return out


def net_forward(layers, x0, pe, mode, E0=None):
    """fp64 forward of the whole net from its first-layer input x0 (n, K0: xyt rows, or the fp64 PE with its bound E0; pe: the same PE for the skip
    layers) with the per-layer bounds PROPAGATED: E_l = B_l den_l + A_l + |W_l| E_{l-1}, den taken at |X| + E (what the inference chain, which
    keeps no tiles, is held to).  Returns (o, E_out)."""
    hid = layers[0][0].shape[0]
    X = np.asarray(x0, np.float64); E = np.zeros_like(X) if E0 is None else np.asarray(E0, np.float64)
    Epe = E
    nl = len(layers)
    for l, (W, b) in enumerate(layers):
        if l > 0 and W.shape[1] > hid:
            X = np.concatenate([X, pe], axis=1); E = np.concatenate([E, Epe], axis=1)
        hd = None if (l == 0 or l == nl - 1) else hid
        Z, bound = forward_pre(W, b, X, mode, hd)
        _, bound_hi = forward_pre(W, b, np.abs(X) + E, mode, hd)              # den at |X| + E
        E = np.maximum(bound, bound_hi) + E @ np.abs(W).T
        X = np.tanh(Z) if l == nl - 1 else np.maximum(Z, 0.0)
    return X, E + C_TANH * U
