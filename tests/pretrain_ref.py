"""The twin of what a PRE-TRAIN step does around its chains (csrc/elem.hip af_rand_below, k_pre_prep, k_pre_loss) and of the private mask layout of the
16-row chains (csrc/mlp16.hip), with the bound every entry of what those kernels wrote must lie inside.  Plain numpy, no GPU:
tests/test_pretrain_ref_host.py ties the twin to the oracle (oracle.atlas_oracle.pre_train_mapping in torch fp64), to the published Philox vectors, and
shows that fp32 emulations stay inside the bounds while the mutations listed there leave them; tests/test_gpu_pretrain_entries.py holds the kernels'
rows and tiles (af_debug_tiles "rows", "x0", "out", "dout", "masks") to it.  The layer twin and its bounds are tests/chain_ref.py, unchanged.

SAMPLER (rand_below).  Philox4x32-10 as published (Salmon et al., SC'11: multipliers D2511F53 / CD9E8D57, Weyl key increments 9E3779B9 / BB67AE85, ten
rounds) on the counter (n, iter, stream, 0x41544c53) with the key (lo32(seed), hi32(seed)); r = o[1] << 32 | o[0]; the draw is the high 64 bits of
r * bound.  Integers: the twin is exact.  Streams: 0 the training batch (bound resx resy F), 1 the pre-train rows (resy), 2 the pre-train columns (resx).

ROWS (pre_prep_rows).  k_pre_prep forms (float)x / half_main - 1.f, (float)y / half_main - 1.f: a correctly rounded division and a subtraction, nothing a
compiler can contract — numpy float32 must match BIT FOR BIT.  half_main = fl32(max(resx, resy) / 2.0); t = fl32(f / (F / 2.0) - 1.0) is formed on the
host in fp64 and rounded once.  The fourth column is 0.

SEEDS (pre_loss_ref).  k_pre_loss, operation by operation, on step_ref's value type V (fp64 value + first-order running error: every fp32 operation adds
u |result|, u = 2^-24, to what its operands carry):
    e   = c s - o            the product rounds (u |c s|), the difference rounds (u |e|); contracted to an fma only the second.  Both roundings are
                             counted, so either compilation is covered — and the error is relative to |c s| + |o|, NOT to |e|: e is a cancelling
                             difference and its own cancellation enters the bound by itself
    q   = e_u e_u + e_v e_v  two products and a sum (an fma saves one rounding)
    l   = sqrtf(q)           correctly rounded: u l, on top of dq / (2 sqrt(q - dq))
    w   = l > 0 ? -1 / (l N) : 0     one product ((float)N is exact for N < 2^24), one correctly rounded division
    d   = (w e_u, w e_v)     one product each; d(e) propagates to first order through all of the above
Entries are held at BOUND_FACTOR (2) x the running error: the factor covers the second-order terms.  A row whose l lies within its own error of 0
(l <= 2 BOUND_FACTOR dl, step_ref's over_pos) is "undecided" — the kernel may have taken either branch — and is left out; the caller counts them.  A
row with c s == o exactly has l = 0 with error 0: decided, its seed is exactly 0 (torch's norm has the zero subgradient there).
Loss record: the call returns fl32(sum_n l_n) / (float)N; |hip - fp64 mean| <= (summed running error + N u sum |l_n|) / N — N u covers any order of the
N - 1 additions (lanes, waves, blocks, k_adam's fold) and the host's division, as step_ref.record_terms counts it.

MASKS (mask_bits16).  The 16-row chains keep their ReLU sign masks private (mlp16.hip head): per 16-row tile 64 lanes x 2 words, lane = 16 q + j owns row
j; its register e = 4 T + r (T = 0..15, r = 0..3) is feature 16 T + 4 q + r and sits at bit 31 - (e & 31) of word e >> 5 (relu_out shifts the words left
by one per element: v_alignbit by 31).  A layer's plane is nt_stride 32-row tiles = 2 nt_stride 16-row tiles of 128 words: the same 256 words per 32-row
tile as the other chains' planes, so af_debug_tiles "masks" serves both."""
import numpy as np

import step_ref as SR

U = SR.U
BOUND_FACTOR = SR.BOUND_FACTOR
F32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
STREAM_TAG = 0x41544C53
LOSS_MUTATIONS = ("no_1_over_N", "sign", "eu_ev")
ROW_MUTATIONS = ("x_y", "half_resx")
MASK_MUTATIONS = ("bit_order", "lane_quads")


# ---- the configurations both test files run (the names of tests/test_gpu_adam.py where they coincide) -------------------------------------------
NARROW = dict(number_of_channels_mapping1=40, number_of_layers_mapping1=3, use_positional_encoding_mapping1=True, number_of_positional_encoding_mapping1=3,
              number_of_channels_atlas=200, number_of_layers_atlas=6, positional_encoding_num_atlas=6)
PE5 = dict(use_positional_encoding_mapping2=True, number_of_positional_encoding_mapping2=5)
# kind: (two_layer, config overrides, the mapping net that is pre-trained: 1 or 2, the state of tests/test_gpu_adam.start_state it starts from)
KINDS = {"S": (False, {}, 1, "S"), "T2": (True, {}, 2, "T"), "N": (False, NARROW, 1, "N"), "P5": (True, PE5, 2, None)}
RESX, RESY = 37, 21
BATCHES = (16, 272, 490, 500)
BIG_BATCH = 10000
PRETRAIN = 40                          # iterations the starting state has been pre-trained (tests/test_gpu_adam.start_state)


def draws(seed, steps, NB, resx=RESX, resy=RESY):
    """The injected draws of the tests: (ys, xs), each (steps, NB) int64."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, resy, (steps, NB)), rng.integers(0, resx, (steps, NB))


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
def philox4x32(ctr, key, rounds=10):
    """Philox4x32 on counters ctr (..., 4) and keys key (..., 2) (broadcast against each other), uint32 values: the four output words (..., 4) uint32."""
    c = np.asarray(ctr, np.uint64) & M32
    k = np.asarray(key, np.uint64) & M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2              # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def rand_below(seed, it, n, stream, bound):
    """af_rand_below(seed, it, j, stream, bound) for j = 0 .. n-1: (n,) int64 draws in [0, bound)."""
    seed, bound = int(seed), int(bound)
    assert 0 <= seed < 2 ** 64 and 0 < bound < 2 ** 63 and 0 <= int(it) < 2 ** 32
    ctr = np.zeros((int(n), 4), np.uint64)
    ctr[:, 0] = np.arange(int(n)); ctr[:, 1] = int(it); ctr[:, 2] = int(stream); ctr[:, 3] = STREAM_TAG
    o = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)).astype(np.uint64)
    r = (o[:, 1] << np.uint64(32)) | o[:, 0]
    return np.array([(int(x) * bound) >> 64 for x in r], np.int64)      # __umul64hi: Python integers keep the 128-bit product


# ---- k_pre_prep ---------------------------------------------------------------------------------------------------------------------------------
def pre_prep_rows(ys, xs, resx, resy, F, f, mut=()):
    """(n, 4) float32 rows (x, y, t, 0) of pre-train step `f` (the frame of the step: step index mod F) of an F-frame handle, in the kernel's fp32
    operations."""
    ys, xs = np.asarray(ys, np.int64).reshape(-1), np.asarray(xs, np.int64).reshape(-1)
    assert ys.shape == xs.shape
    half = F32((resx if "half_resx" in mut else max(resx, resy)) / 2.0)
    one = F32(1.0)
    if "x_y" in mut:
        ys, xs = xs, ys
    out = np.zeros((ys.size, 4), np.float32)
    out[:, 0] = xs.astype(np.float32) / half - one
    out[:, 1] = ys.astype(np.float32) / half - one
    out[:, 2] = F32(float(f) / (F / 2.0) - 1.0)
    return out


def pre_x0_tiles(rows):
    """The T-layout copy k_pre_prep keeps of the xyt rows (value, written mask), as step_ref.x0_tiles."""
    return SR.x0_tiles(np.asarray(rows, np.float32)[:, :3])


# ---- k_pre_loss ---------------------------------------------------------------------------------------------------------------------------------
def _pre_loss(ar, rows, out, uv_scale, N, mut=()):
    """k_pre_loss on the arithmetic `ar` (step_ref.ArV: the twin; step_ref.ArF: an fp32 emulation).  Returns (l, d_u, d_v, undecided)."""
    rows, out = np.asarray(rows, np.float64), np.asarray(out, np.float64)
    s = float(F32(uv_scale))
    cu, cv, ou, ov = (ar.lift(x) for x in (rows[:, 0], rows[:, 1], out[:, 0], out[:, 1]))
    eu, ev = cu * s - ou, cv * s - ov
    l = ar.sqrt(eu * eu + ev * ev)
    den = l if "no_1_over_N" in mut else l * float(N)
    w, und = ar.over_pos(ar.lift(np.full(len(rows), 1.0 if "sign" in mut else -1.0)), den)
    if "eu_ev" in mut:
        eu, ev = ev, eu
    return l, w * eu, w * ev, und


class PreLoss:
    """What pre_loss_ref returns: l (n,) the fp64 terms and le their running error; d (n, 2) the seeds -(e_u, e_v) / (l N) and de their running
    error (held at BOUND_FACTOR x de); und (n,) rows left out; mean / mean_bound: the loss record."""

    def __init__(self, l, le, d, de, und, N):
        self.l, self.le, self.d, self.de, self.und = l, le, d, de, und
        self.mean = float(l.sum() / N)
        self.mean_bound = float((le.sum() + N * U * np.abs(l).sum()) / N)


def pre_loss_ref(rows, out, uv_scale, N, mut=()):
    """The twin of k_pre_loss on rows (n, >= 2) and out (n, >= 2), the kernel's own fp32 inputs, n == N == pretrain_batch."""
    assert len(rows) == len(out) == N
    l, du, dv, und = _pre_loss(SR.ArV, rows, out, uv_scale, N, mut)
    exact0 = (l.v == 0) & (l.e == 0)                  # c s == o exactly: the branch is decided, the seed is exactly 0
    und = und & ~exact0
    d = np.stack([du.v, dv.v], axis=1); de = np.stack([du.e, dv.e], axis=1)
    return PreLoss(l.v, l.e, d, de, und, N)


def pre_loss_f32(rows, out, uv_scale, N, fused):
    """An fp32 emulation of k_pre_loss (plain, or every a b + c contracted to an fma): (l (n,), d (n, 2)) as fp64 arrays of fp32 values."""
    l, du, dv, _ = _pre_loss(SR.ArF(fused), rows, out, uv_scale, N)
    return l.done()[0], np.stack([du.done()[0], dv.done()[0]], axis=1)


def loose_share(tw):
    """The bite condition of tests/test_gpu_step_rows.py on the seed class: share of the usable entries with 2 bound > 2^-6 max(|ref|, median |ref|)."""
    ok = ~tw.und
    ref = np.abs(tw.d[ok])
    return float((BOUND_FACTOR * tw.de[ok] > 2.0 ** -6 * np.maximum(ref, np.median(ref))).mean())


# ---- the mask layout of mlp16.hip ---------------------------------------------------------------------------------------------------------------
def mask_bits16(words, n=None, mut=()):
    """(nt, 64, 4) uint32 words of one layer's plane (af_debug_tiles "masks") -> (n, 256) bool, rows of the 2 nt 16-row tiles."""
    w = np.ascontiguousarray(words).astype(np.uint32).reshape(-1, 4, 16, 2)               # (t16, q, j, word)
    e = np.arange(64)
    sh = ((e & 31) if "bit_order" in mut else 31 - (e & 31)).astype(np.uint32)
    bits = ((w[:, :, :, e >> 5] >> sh) & 1).astype(bool)                                  # (t16, q, j, e)
    T, r = e >> 2, e & 3
    out = np.zeros((w.shape[0], 16, 256), bool)
    for q in range(4):
        out[:, :, 16 * T + 4 * (q ^ 1 if "lane_quads" in mut else q) + r] = bits[:, q]
    out = out.reshape(-1, 256)
    return out if n is None else out[:n]
