"""The twin of what a training step does AROUND the chains (csrc/elem.hip k_prep, k_loss_single, k_loss_seg; mlp_common.h chain_dpe_to_uv) and the bound every
entry of what those kernels wrote must lie inside.  Plain numpy, no GPU: tests/test_step_ref_host.py ties the twin to the oracle (oracle/atlas_oracle.py in
fp64 and torch autograd) and shows that fp32 emulations stay inside the bounds while eleven one-line mutations leave them; tests/test_gpu_step_rows.py holds
the kernels' rows (af_debug_tiles "rows", "out", "dout", "dz", "pe") to it.

ROWS (prep_rows).  k_prep computes every coordinate as (float)i / half - 1.f (a flow match: ((float)x + flow) / half - 1.f): divisions, additions of two
values and subtractions only, nothing a compiler can contract, and fp32 division is correctly rounded on the device — the restatement in numpy float32
must match BIT FOR BIT.  Layout of a mapping net's batch: segment s of N rows, s = 0 centre, 1 (x, y+1), 2 (x+1, y) [both over resx / 2], 3 (x, y-d),
4 (x-d, y) and, while the global rigidity term is on (nseg 9), 5 (x, y-D), 6 (x-D, y) with D the net's own distance; behind them, from row (nseg - 2) N,
the VALID flow matches of the batch, sample-major, a sample's forward match (frame f+1) before its backward match (f-1).  The alpha net: segments 0-2 and
the same matches from row 3N.

SEEDS (loss_single / loss_seg).  The loss kernels are restated operation by operation on a small value type, so that ONE text serves three arithmetics:
  V   fp64 value + first-order running error: every fp32 operation adds u |result| (u = 2^-24) to the error propagated from its operands — |a| e_b + |b| e_a
      for a product, (e_a + |a / b| e_b) / (|b| - e_b) for a quotient, e / (2 sqrt(x - e)) for a root — so a subtraction carries its cancellation into the
      bound by itself.  sqrtf and division count as correctly rounded (u |result|).  logf: C_LOG u |result|, C_LOG = 9.155 — numpy-fp32 log against fp64
      on 8 10^7 arguments in [0.001, 0.999] (alpha lies in [0.001, 0.991], 1 - alpha in [0.009, 0.999]): worst 4.5773 u of the result, times a 2x margin
      (the constant is taken the way chain_ref took tanhf's; tests/test_step_ref_host.py re-measures it).  A fused multiply-add rounds once where the
      plain form rounds twice, and the bound counts both roundings: it covers either compilation (the loss kernels are not contract(off)).
  F   numpy-fp32 emulation, plain or with fused multiply-adds (the exact fp64 product added and rounded once) — the stand-in for a kernel on the CPU.
The asserted bound is 2 x the running error (BOUND_FACTOR): the factor covers the second-order terms the first-order propagation drops.
Constants: the kernels hold the regulariser 0.001f, 0.99f, 0.001f, 0.495f and the coefficients in fp32; coeffs(..., exact=False) gives those values (the twin
of the KERNEL), exact=True the doubles the reference computes with (the twin compared with the oracle).
Kinks: sign(d) of the alpha-flow L1 term and 1 / |e| of a flow term are not continuous at 0; where the twin's d, or a flow norm, lies within its own running
error of 0 the entries that depend on it are flagged (the `undecided` arrays) and left out by the caller, which counts them.

UV GRADIENT (dpe_to_uv).  dPE = dZ_0 W_0 (K = 256 on the fp32 pipe in every mode: chain_ref's bound (K + 1) u den) enters as a value with that bound; then
sum over octaves of b (cos dsin - sin dcos), b = fl32(pi) 2^k, k = 2g + h for lane half h, the two halves added, times din_scale, `+=` onto the loss seed."""
import numpy as np

U = 2.0 ** -24
C_LOG = 9.155
BOUND_FACTOR = 2.0
PI32 = float(np.float32(np.pi))
F32 = np.float32
REC_RGB, REC_DX, REC_DY, REC_FF, REC_FB, REC_MF, REC_MB, REC_FG = 0, 3, 6, 9, 11, 13, 14, 15

MUTATIONS = ("y+d", "rank_b", "flow_base", "dtx_dty", "du_xm_ym", "eps", "aflow_sign", "fg_weight", "cnt_bwd", "octave", "assign")


# ---- the two arithmetics ------------------------------------------------------------------------------------------------------------------------
class V:
    """fp64 value and first-order running error bound of its fp32 computation."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def c(x):
        return x if isinstance(x, V) else V(x)

    @staticmethod
    def _r(v, e):
        return V(v, e + U * np.abs(v))

    def __add__(self, o):
        o = V.c(o); return V._r(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.c(o); return V._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.c(o) - self

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.c(o); return V._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.c(o)
        lo = np.maximum(np.abs(o.v) - o.e, 1e-300)
        return V._r(self.v / o.v, self.e / lo + np.abs(self.v) * o.e / (lo * np.maximum(np.abs(o.v), 1e-300)))

    def __rtruediv__(self, o):
        return V.c(o) / self

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def done(self):
        return self.v, self.e


class ArV:
    """The operations of the twin that are not operators."""
    lift = staticmethod(V.c)

    @staticmethod
    def sqrt(x):
        r = np.sqrt(x.v)
        return V(r, x.e / (2.0 * np.sqrt(np.maximum(x.v - x.e, 1e-300))) + U * r)

    @staticmethod
    def log(x):
        r = np.log(x.v)
        return V(r, x.e / np.maximum(x.v - x.e, 1e-300) + C_LOG * U * np.abs(r))

    @staticmethod
    def abs(x):
        return V(np.abs(x.v), x.e)

    @staticmethod
    def sign(x):
        """(sign as an exact value, undecided: the value lies within its own error of 0)."""
        return V(np.sign(x.v)), np.abs(x.v) <= BOUND_FACTOR * x.e

    @staticmethod
    def over_pos(num, den):
        """den > 0 ? num / den : 0 — (value, undecided: den within its own error of 0, the quotient's bound means nothing there)."""
        und = den.v <= 2.0 * BOUND_FACTOR * den.e
        q = num / V(np.where(und, 1.0, den.v), np.where(und, 0.0, den.e))
        return V(np.where(und, 0.0, q.v), np.where(und, 0.0, q.e)), und

    @staticmethod
    def select(mask, x):
        return V(np.where(mask, x.v, 0.0), np.where(mask, x.e, 0.0))


def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


class F:
    """An fp32 value (held in fp64), or — fused arithmetic only — the exact product of two that the next addition absorbs as an fma."""
    __slots__ = ("v", "pending", "fused")

    def __init__(self, v, fused=False, pending=False):
        self.v = np.asarray(v, np.float64); self.fused = fused; self.pending = pending

    def val(self):
        return _r32(self.v) if self.pending else self.v

    def _o(self, o):
        return o if isinstance(o, F) else F(_r32(o), self.fused)

    def __add__(self, o):
        o = self._o(o)
        if self.pending:                   # fma: the exact product takes the other operand in (a product itself: rounded first)
            return F(_r32(self.v + o.val()), self.fused)
        return F(_r32(self.v + o.v), self.fused)          # o.v: a value, or the exact product of the fma
    __radd__ = __add__

    def __sub__(self, o):
        return self + (-self._o(o))

    def __rsub__(self, o):
        return self._o(o) - self

    def __neg__(self):
        return F(-self.v, self.fused, self.pending)

    def __mul__(self, o):
        o = self._o(o)
        p = self.val() * o.val()              # two fp32 factors: exact in fp64
        return F(p, self.fused, True) if self.fused else F(_r32(p), self.fused)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._o(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            return F(_r32(self.val() / o.val()), self.fused)       # fp64 quotient of fp32 operands rounds to the correctly rounded fp32 quotient

    def __rtruediv__(self, o):
        return self._o(o) / self

    def __getitem__(self, i):
        return F(self.v[i], self.fused, self.pending)

    def done(self):
        return self.val(), None


class ArF:
    def __init__(self, fused):
        self.fused = fused

    def lift(self, x):
        return x if isinstance(x, F) else F(_r32(x), self.fused)

    def sqrt(self, x):
        return F(_r32(np.sqrt(x.val())), self.fused)

    def log(self, x):
        return F(np.log(x.val().astype(np.float32)).astype(np.float64), self.fused)

    def abs(self, x):
        return F(np.abs(x.val()), self.fused)

    def sign(self, x):
        return F(np.sign(x.val()), self.fused), np.zeros(np.shape(x.v), bool)

    def over_pos(self, num, den):
        d = den.val()
        q = (num / F(np.where(d > 0, d, 1.0), self.fused)).val()
        return F(np.where(d > 0, q, 0.0), self.fused), np.zeros(np.shape(d), bool)

    def select(self, mask, x):
        return F(np.where(mask, x.val(), 0.0), self.fused)


# ---- configuration ------------------------------------------------------------------------------------------------------------------------------
def glob_on(cfg, it):
    return bool(cfg.include_global_rigidity_loss) and it <= cfg.stop_global_rigidity


def coeffs(cfg, it, two_layer, exact=False):
    """The coefficients of iteration `it` as the loss kernel gets them (host.hip enqueue_*_step): fp32 values unless `exact` (the reference's doubles)."""
    r = (lambda x: float(x)) if exact else (lambda x: float(np.float32(x)))
    glob = glob_on(cfg, it)
    K = dict(N=int(cfg.samples_batch), nseg=9 if glob else 7, L=float(max(cfg.resx, cfg.resy)), uv_scale=r(cfg.uv_mapping_scale), d_local=float(cfg.derivative_amount),
             c_rgb=r(cfg.rgb_coeff), c_grad=r(cfg.gradient_loss_coeff) if cfg.use_gradient_loss else 0.0, c_rig=r(cfg.rigidity_coeff), c_flow=r(cfg.optical_flow_coeff),
             eps=r(0.001), a99=r(0.99), a001=r(0.001), dalpha=r(0.495))
    if two_layer:
        K.update(d_global=(float(cfg.global_rigidity_derivative_amount_fg), float(cfg.global_rigidity_derivative_amount_bg)),
                 c_grig=(r(cfg.global_rigidity_coeff_fg) if glob else 0.0, r(cfg.global_rigidity_coeff_bg) if glob else 0.0),
                 c_boot=0.0 if it > cfg.stop_bootstrapping_iteration else r(cfg.alpha_bootstrapping_factor), c_aflow=r(cfg.alpha_flow_factor), c_sparse=r(cfg.sparsity_coeff))
    else:
        K.update(d_global=(float(cfg.global_rigidity_derivative_amount_fg),), c_grig=(r(cfg.global_rigidity_coeff_fg) if glob else 0.0,))
    return K


def records_from_video(video, inds, two_layer):
    """(n, 16) fp32 pixel records of get_tuples' columns `inds`, the layout of k_pack_table: rgb, d/dx rgb, d/dy rgb, forward flow, backward flow, forward mask,
    backward mask, fg mask."""
    inds = np.asarray(inds, np.int64)
    resx, resy = int(video.resx), int(video.resy)
    f = inds // (resx * resy); rem = inds - f * resx * resy
    y = rem // resx; x = rem - y * resx
    rec = np.zeros((inds.size, 16), np.float32)
    rec[:, 0:3] = video.video_frames.numpy()[y, x, :, f]
    rec[:, 3:6] = video.video_frames_dx.numpy()[y, x, :, f]
    rec[:, 6:9] = video.video_frames_dy.numpy()[y, x, :, f]
    rec[:, 9:11] = video.optical_flows.numpy()[y, x, :, f, 0]
    rec[:, 11:13] = video.optical_flows_reverse.numpy()[y, x, :, f, 0]
    rec[:, 13] = video.optical_flows_mask.numpy()[y, x, f, 0]
    rec[:, 14] = video.optical_flows_reverse_mask.numpy()[y, x, f, 0]
    if two_layer:
        rec[:, 15] = video.mask_frames.numpy()[y, x, f]
    return rec


# ---- k_prep -------------------------------------------------------------------------------------------------------------------------------------
def prep_rows(records, inds, cfg, it, two_layer, mut=()):
    """k_prep in float32, operation by operation.  Returns dict: map1 [, map2, alpha] (live rows, 3) fp32; rank (N, 2) int (-1: no valid match);
    counts (forward, backward); live; nseg; flow_base."""
    rec = np.asarray(records, np.float32)
    inds = np.asarray(inds, np.int64)
    N = inds.size
    assert rec.shape == (N, 16) and N == cfg.samples_batch
    resx, resy, nf = int(cfg.resx), int(cfg.resy), int(cfg.number_of_frames)
    P2 = resx * resy
    f = inds // P2; rem = inds - f * P2
    y = rem // resx; x = rem - y * resx
    hm, hg, hf = F32(max(resx, resy) / 2.0), F32(resx / 2.0), F32(nf / 2.0)
    one = F32(1.0)
    co = lambda i, h: i.astype(np.float32) / h - one                  # noqa: E731   (float)i / half - 1.f
    nseg = 9 if glob_on(cfg, it) else 7
    d = int(cfg.derivative_amount)
    sgn = 1 if "y+d" in mut else -1
    xc, yc, tc = co(x, hm), co(y, hm), co(f, hf)
    segs = [(xc, yc), (co(x, hg), co(y + 1, hg)), (co(x + 1, hg), co(y, hg)), (xc, co(y + sgn * d, hm)), (co(x - d, hm), yc)]
    vf, vb = rec[:, REC_MF] != 0, rec[:, REC_MB] != 0
    per = vf.astype(np.int64) + vb
    rank_f = np.cumsum(per) - per
    rank_b = rank_f + (0 if "rank_b" in mut else vf)
    live = int(per.sum())
    base = ((9 if "flow_base" in mut else nseg) - 2) * N
    fx, fy, ft = co(x.astype(np.float32) + rec[:, REC_FF], hm), co(y.astype(np.float32) + rec[:, REC_FF + 1], hm), co(f + 1, hf)
    bx, by, bt = co(x.astype(np.float32) + rec[:, REC_FB], hm), co(y.astype(np.float32) + rec[:, REC_FB + 1], hm), co(f - 1, hf)

    def flows(rows, at):
        rows[at + rank_f[vf]] = np.stack([fx, fy, ft], 1)[vf]
        rows[at + rank_b[vb]] = np.stack([bx, by, bt], 1)[vb]

    out = dict(rank=np.stack([np.where(vf, rank_f, -1), np.where(vb, rank_b, -1)], 1), counts=(int(vf.sum()), int(vb.sum())), live=live, nseg=nseg, flow_base=(nseg - 2) * N)
    for name, D in (("map1", cfg.global_rigidity_derivative_amount_fg),) + ((("map2", cfg.global_rigidity_derivative_amount_bg),) if two_layer else ()):
        s = list(segs)
        if nseg > 7:
            s += [(xc, co(y - int(D), hm)), (co(x - int(D), hm), yc)]
        rows = np.zeros((max(base, (nseg - 2) * N) + live, 3), np.float32)
        for i, (a, b) in enumerate(s):
            rows[i * N:(i + 1) * N] = np.stack([a, b, tc], 1)
        flows(rows, base)
        out[name] = rows[:(nseg - 2) * N + live]
    if two_layer:
        rows = np.zeros((3 * N + live, 3), np.float32)
        for i, (a, b) in enumerate(segs[:3]):
            rows[i * N:(i + 1) * N] = np.stack([a, b, tc], 1)
        flows(rows, 3 * N)
        out["alpha"] = rows
    return out


def x0_tiles(rows):
    """The T-layout copy k_prep keeps of a net's xyt rows: (nt, 32, 32) with tile[t, c, j] = rows[32 t + j, c]; (value, written mask)."""
    R_ = len(rows); nt = (R_ + 31) // 32
    t = np.zeros((nt * 32, 32), np.float32); w = np.zeros((nt * 32, 32), bool)
    t[:R_, :3] = rows; w[:R_, :3] = True
    return t.reshape(nt, 32, 32).transpose(0, 2, 1), w.reshape(nt, 32, 32).transpose(0, 2, 1)


# ---- the loss kernels ---------------------------------------------------------------------------------------------------------------------------
class _Out:
    """A [rows][4] gradient buffer of the twin: value, running error, undecided; rows never written stay exactly 0."""

    def __init__(self, rows):
        self.v = np.zeros((rows, 4)); self.e = np.zeros((rows, 4)); self.und = np.zeros((rows, 4), bool)

    def put(self, rows, col, x, mask=None, und=None):
        v, e = x.done()
        sel = slice(None) if mask is None else mask
        rows = np.asarray(rows)[sel]
        self.v[rows, col] = v[sel]
        if e is not None:
            self.e[rows, col] = e[sel]
        if und is not None:
            self.und[rows, col] = und[sel]


def _pad32(r):
    return (r + 31) // 32 * 32


def _rigidity(ar, u, v, u_ym, v_ym, u_xm, v_xm, L, s, d, w, eps, mut):
    """elem.hip rigidity(): (loss, du, dv, du_xm, du_ym, dv_xm, dv_ym)."""
    j00 = ((u - u_xm) * L / 2.0) / s / d; j01 = ((u - u_ym) * L / 2.0) / s / d
    j10 = ((v - v_xm) * L / 2.0) / s / d; j11 = ((v - v_ym) * L / 2.0) / s / d
    g00 = j00 * j00 + j10 * j10; g01 = j00 * j01 + j10 * j11; g11 = j01 * j01 + j11 * j11
    A = g00 + eps; D = g11 + eps; B = g01
    det = A * D - B * B
    i00 = D / det; i01 = (-B) / det; i11 = A / det
    ng = ar.sqrt(g00 * g00 + 2.0 * g01 * g01 + g11 * g11)
    ni = ar.sqrt(i00 * i00 + 2.0 * i01 * i01 + i11 * i11)
    b2_00 = i00 * i00 + i01 * i01; b2_01 = i00 * i01 + i01 * i11; b2_11 = i01 * i01 + i11 * i11
    b3_00 = b2_00 * i00 + b2_01 * i01; b3_01 = b2_00 * i01 + b2_01 * i11; b3_11 = b2_01 * i01 + b2_11 * i11
    rg = 1.0 / ng; ri = 1.0 / ni                  # ng, ni >= |(G + eps)^-1| > 0: the kernel's guards never fire
    s00 = g00 * rg - b3_00 * ri; s01 = g01 * rg - b3_01 * ri; s11 = g11 * rg - b3_11 * ri
    k = (L / 2.0) / s / d * w * 2.0
    d00 = k * (j00 * s00 + j01 * s01); d01 = k * (j00 * s01 + j01 * s11)
    d10 = k * (j10 * s00 + j11 * s01); d11 = k * (j10 * s01 + j11 * s11)
    du_xm, du_ym = -d00, -d01
    if "du_xm_ym" in mut:
        du_xm, du_ym = du_ym, du_xm
    return ng + ni, d00 + d01, d10 + d11, du_xm, du_ym, -d10, -d11


def _mapping_part(ar, om, dm, und_all, N, nseg, rank, counts, K, net, wrow, terms, tag, mut, dA=None):
    """Rigidity (local, global) and the flow terms of one mapping net, written into the _Out `dm`; returns dA with the net's flow contribution added."""
    lift = ar.lift
    L, s = K["L"], lift(K["uv_scale"])
    invN = lift(1.0) / lift(float(N))
    n = np.arange(N)
    col = lambda r, c: lift(om[r, c])                                # noqa: E731
    u, v = col(n, 0), col(n, 1)
    eps = lift(K["eps"] * 1.1) if "eps" in mut else lift(K["eps"])
    du = lift(np.zeros(N)); dv = lift(np.zeros(N))
    for name, seg, d, c in (("rigidity", 3, K["d_local"], K["c_rig"]), ("global_rigidity", 5, K["d_global"][net], K["c_grig"][net])):
        if seg == 5 and nseg <= 7:
            terms[name + tag] = lift(np.zeros(N))
            continue
        loss, ru, rv, du_xm, du_ym, dv_xm, dv_ym = _rigidity(ar, u, v, col(seg * N + n, 0), col(seg * N + n, 1), col((seg + 1) * N + n, 0), col((seg + 1) * N + n, 1),
                                                             L, s, d, lift(c) * invN, eps, mut)
        terms[name + tag] = loss
        du = du + ru; dv = dv + rv
        dm.put(seg * N + n, 0, du_ym); dm.put(seg * N + n, 1, dv_ym)
        dm.put((seg + 1) * N + n, 0, du_xm); dm.put((seg + 1) * N + n, 1, dv_xm)
    fscale = L / (2.0 * s)
    base = (nseg - 2) * N
    for dr, dname in ((0, "fwd"), (1, "bwd")):
        valid = rank[:, dr] >= 0
        row = base + np.where(valid, rank[:, dr], 0)
        eu = col(row, 0) - u; ev = col(row, 1) - v
        nrm = ar.sqrt(eu * eu + ev * ev)
        l = nrm * L / (2.0 * s)
        cnt = lift(float(counts[0 if "cnt_bwd" in mut else dr]))
        num = lift(K["c_flow"]) * 0.5 * fscale
        if wrow is not None:
            l_w = l * wrow; num = num * wrow
        else:
            l_w = l
        w, und = ar.over_pos(num, nrm * cnt)
        gu = w * eu; gv = w * ev
        terms["flow_%s%s" % (dname, tag)] = ar.select(valid, l_w)
        du = du - ar.select(valid, gu); dv = dv - ar.select(valid, gv)
        und = und & valid
        dm.put(row, 0, gu, valid, und); dm.put(row, 1, gv, valid, und)
        und_all |= und
        if dA is not None:
            wsign = -1.0 if net else 1.0
            dA = dA + ar.select(valid, wsign * lift(K["c_flow"]) * 0.5 * l / cnt)
    dm.put(n, 0, du, und=und_all); dm.put(n, 1, dv, und=und_all)
    return dA


def _run_single(ar, out_map, out_atlas, records, rank, counts, K, mut):
    N, nseg = K["N"], K["nseg"]
    lift = ar.lift
    rec = np.asarray(records, np.float32)
    live = int((rank >= 0).sum())
    dm = _Out(_pad32((nseg - 2) * N + live)); da = _Out(3 * N)
    terms = {}
    n = np.arange(N)
    invN = lift(1.0) / lift(float(N))
    c_rgb, c_grad = lift(K["c_rgb"]), lift(K["c_grad"])
    l_rgb = lift(np.zeros(N)); l_grad = lift(np.zeros(N))
    for c in range(3):
        rgb = (lift(out_atlas[n, c]) + 1.0) * 0.5; rgby = (lift(out_atlas[N + n, c]) + 1.0) * 0.5; rgbx = (lift(out_atlas[2 * N + n, c]) + 1.0) * 0.5
        e = rgb - lift(rec[:, REC_RGB + c])
        rx = lift(rec[:, REC_DX + c]) - (rgbx - rgb); ry = lift(rec[:, REC_DY + c]) - (rgby - rgb)
        l_rgb = l_rgb + e * e
        l_grad = l_grad + (rx * rx + ry * ry)
        dtc = 0.5 * (c_rgb * 2.0 * e + c_grad * 2.0 * (rx + ry)) * invN
        dtx = 0.5 * ((-c_grad) * 2.0 * rx) * invN
        dty = 0.5 * ((-c_grad) * 2.0 * ry) * invN
        if "dtx_dty" in mut:
            dtx, dty = dty, dtx
        da.put(n, c, dtc); da.put(N + n, c, dty); da.put(2 * N + n, c, dtx)
    terms["rgb"], terms["gradient"] = l_rgb, l_grad
    und = np.zeros(N, bool)
    _mapping_part(ar, out_map, dm, und, N, nseg, rank, counts, K, 0, None, terms, "", mut)
    return dict(dout_map=dm, dout_atlas=da, terms=terms, undecided_samples=und)


def _alpha_of(t, K):
    a = 0.5 * (t + 1.0)
    a = a * K["a99"]
    return a + K["a001"]


def _run_seg(ar, out_m1, out_m2, out_alpha, out_atlas, records, rank, counts, K, mut):
    N, nseg = K["N"], K["nseg"]
    lift = ar.lift
    rec = np.asarray(records, np.float32)
    live = int((rank >= 0).sum())
    d1, d2 = _Out(_pad32((nseg - 2) * N + live)), _Out(_pad32((nseg - 2) * N + live))
    da, dal = _Out(6 * N), _Out(_pad32(3 * N + live))
    terms = {}
    n = np.arange(N)
    invN = lift(1.0) / lift(float(N))
    KA = dict(a99=lift(K["a99"]), a001=lift(K["a001"]))
    al = _alpha_of(lift(out_alpha[n, 0]), KA); aly = _alpha_of(lift(out_alpha[N + n, 0]), KA); alx = _alpha_of(lift(out_alpha[2 * N + n, 0]), KA)
    c_rgb, c_grad, c_sparse = lift(K["c_rgb"]), lift(K["c_grad"]), lift(K["c_sparse"])
    z = lambda: lift(np.zeros(N))                                    # noqa: E731
    dA, dAy, dAx, l_rgb, l_grad, l_sp, sq1 = z(), z(), z(), z(), z(), z(), z()
    at = lambda seg, c: lift(out_atlas[seg * N + n, c])             # noqa: E731
    for c in range(3):
        r1 = (at(0, c) + 1.0) * 0.5; r2 = (at(3, c) + 1.0) * 0.5
        r1y = (at(1, c) + 1.0) * 0.5; r2y = (at(4, c) + 1.0) * 0.5
        r1x = (at(2, c) + 1.0) * 0.5; r2x = (at(5, c) + 1.0) * 0.5
        rgb = r1 * al + r2 * (1.0 - al)
        rgby = r1y * aly + r2y * (1.0 - aly)
        rgbx = r1x * alx + r2x * (1.0 - alx)
        e = rgb - lift(rec[:, REC_RGB + c])
        rx = lift(rec[:, REC_DX + c]) - (rgbx - rgb); ry = lift(rec[:, REC_DY + c]) - (rgby - rgb)
        nf = r1 * (1.0 - al)
        l_rgb = l_rgb + e * e
        l_grad = l_grad + (rx * rx + ry * ry)
        l_sp = l_sp + nf * nf
        sq1 = sq1 + r1 * r1
        g = (c_rgb * 2.0 * e + c_grad * 2.0 * (rx + ry)) * invN
        gx = (-c_grad) * 2.0 * rx * invN; gy = (-c_grad) * 2.0 * ry * invN
        d1c = 0.5 * (al * g + c_sparse * 2.0 * r1 * (1.0 - al) * (1.0 - al) * invN)
        d2c = 0.5 * (1.0 - al) * g
        d1x = 0.5 * alx * gx; d2x = 0.5 * (1.0 - alx) * gx
        d1y = 0.5 * aly * gy; d2y = 0.5 * (1.0 - aly) * gy
        if "dtx_dty" in mut:
            d1x, d1y = d1y, d1x
        dA = dA + (r1 - r2) * g
        dAx = dAx + (r1x - r2x) * gx
        dAy = dAy + (r1y - r2y) * gy
        da.put(n, c, d1c); da.put(N + n, c, d1y); da.put(2 * N + n, c, d1x)
        da.put(3 * N + n, c, d2c); da.put(4 * N + n, c, d2y); da.put(5 * N + n, c, d2x)
    dA = dA - c_sparse * 2.0 * (1.0 - al) * sq1 * invN
    terms["rgb"], terms["gradient"], terms["sparsity"] = l_rgb, l_grad, l_sp
    m = lift(rec[:, REC_FG])
    terms["alpha_bootstrapping"] = (-m) * ar.log(al) - (1.0 - m) * ar.log(1.0 - al)
    dA = dA + lift(K["c_boot"]) * ((-m) / al + (1.0 - m) / (1.0 - al)) * invN
    cntf, cntb = lift(float(counts[0])), lift(float(counts[1]))
    vf, vb = rank[:, 0] >= 0, rank[:, 1] >= 0
    und_a = np.zeros(N, bool)
    row_f = 3 * N + np.where(vf, rank[:, 0], 0); row_b = 3 * N + np.where(vb, rank[:, 1], 0)
    c_aflow = lift(K["c_aflow"])
    # forward: d = al - alpha(match)
    d = al - _alpha_of(lift(out_alpha[row_f, 0]), KA)
    sg, und = ar.sign(d)
    g = c_aflow * 0.5 * sg / cntf
    terms["flow_alpha_fwd"] = ar.select(vf, ar.abs(d))
    dA = dA + ar.select(vf, g); dAf = -g
    und_f = und & vf; und_a |= und_f
    # backward: d = alpha(match) - al
    d = _alpha_of(lift(out_alpha[row_b, 0]), KA) - al
    if "aflow_sign" in mut:
        d = -d
    sg, und = ar.sign(d)
    g = c_aflow * 0.5 * sg / (cntf if "cnt_bwd" in mut else cntb)
    terms["flow_alpha_bwd"] = ar.select(vb, ar.abs(d))
    dAb = g; dA = dA - ar.select(vb, g)
    und_b = und & vb; und_a |= und_b
    und_m = [np.zeros(N, bool), np.zeros(N, bool)]
    for net, (om, dm) in enumerate(((out_m1, d1), (out_m2, d2))):
        wrow = (1.0 - al) if (net or "fg_weight" in mut) else al
        dA = _mapping_part(ar, om, dm, und_m[net], N, nseg, rank, counts, K, net, wrow, terms, str(net + 1), mut, dA)
    und_a |= und_m[0] | und_m[1]
    dalpha = lift(K["dalpha"])
    dal.put(n, 0, dalpha * dA, und=und_a); dal.put(N + n, 0, dalpha * dAy); dal.put(2 * N + n, 0, dalpha * dAx)
    dal.put(row_f, 0, dalpha * dAf, vf, und_f); dal.put(row_b, 0, dalpha * dAb, vb, und_b)
    return dict(dout_m1=d1, dout_m2=d2, dout_atlas=da, dout_alpha=dal, terms=terms, undecided_samples=und_a)


def loss_single_ref(out_map, out_atlas, records, rank, counts, K, mut=()):
    """k_loss_single on the kernel's own output rows: dict(dout_map, dout_atlas: _Out with value / running error / undecided per entry; terms: {name: V (N,)};
    undecided_samples).  The asserted bound is BOUND_FACTOR x the running error."""
    return _run_single(ArV, np.asarray(out_map, np.float32), np.asarray(out_atlas, np.float32), records, np.asarray(rank), counts, K, frozenset(mut))


def loss_seg_ref(out_m1, out_m2, out_alpha, out_atlas, records, rank, counts, K, mut=()):
    """k_loss_seg likewise: dout_m1, dout_m2, dout_atlas, dout_alpha, terms."""
    f = lambda a: np.asarray(a, np.float32)                          # noqa: E731
    return _run_seg(ArV, f(out_m1), f(out_m2), f(out_alpha), f(out_atlas), records, np.asarray(rank), counts, K, frozenset(mut))


def loss_single_emu(out_map, out_atlas, records, rank, counts, K, fused=False, mut=()):
    """The fp32 emulation of k_loss_single (plain, or with every a b + c fused): the CPU stand-in for the kernel."""
    return _run_single(ArF(fused), np.asarray(out_map, np.float32), np.asarray(out_atlas, np.float32), records, np.asarray(rank), counts, K, frozenset(mut))


def loss_seg_emu(out_m1, out_m2, out_alpha, out_atlas, records, rank, counts, K, fused=False, mut=()):
    f = lambda a: np.asarray(a, np.float32)                          # noqa: E731
    return _run_seg(ArF(fused), f(out_m1), f(out_m2), f(out_alpha), f(out_atlas), records, np.asarray(rank), counts, K, frozenset(mut))


SINGLE_RECORD = ("rgb", "gradient", "rigidity", "global_rigidity", "flow")
SEG_RECORD = ("rgb", "gradient", "rigidity1", "rigidity2", "global_rigidity1", "global_rigidity2", "flow1", "flow2", "flow_alpha", "alpha_bootstrapping", "sparsity")


def record_terms(terms, counts, N, two_layer):
    """The loss record's terms (af_train_steps: sums / N; a flow term 0.5 (fwd / #fwd + bwd / #bwd)) from the twin's per-sample terms: {name: (fp64 value,
    bound)}, bound = summed running error + N u sum |term| in the same units.  The kernels add N fp32 terms in a tree (lanes, waves, blocks: < 16 roundings on
    any one term's way, host division included); N u is what a sequential sum would need and covers any order."""
    out = {}

    def mean(t, den):
        v, e = t.done()
        return v.sum() / den, (e.sum() + N * U * np.abs(v).sum()) / den

    for name in (SEG_RECORD if two_layer else SINGLE_RECORD):
        if name.startswith("flow"):
            key = "flow_alpha_%s" if name == "flow_alpha" else "flow_%s" + name[4:]
            (vf, ef), (vb, eb) = mean(terms[key % "fwd"], counts[0]), mean(terms[key % "bwd"], counts[1])
            out[name] = (0.5 * (vf + vb), 0.5 * (ef + eb))
        else:
            out[name] = mean(terms[name], N)
    return out


# ---- chain_dpe_to_uv ----------------------------------------------------------------------------------------------------------------------------
def dpe_product(dz0, W0, emulate=False):
    """dPE = dZ_0 W_0 over the 40 PE slots the kernel reads (a net with fewer octaves: zero weights behind its own).  dz0 (rows, hid) the kernel's plane 0,
    W0 (hid, enc).  Returns (value, chain_ref's bound (256 + 1) u sum |dz w|); emulate: a float32 product instead (bound None)."""
    dz0 = np.asarray(dz0, np.float64); W0 = np.asarray(W0, np.float64)
    W = np.zeros((W0.shape[0], 40)); W[:, :W0.shape[1]] = W0
    if emulate:
        return (dz0.astype(np.float32) @ W.astype(np.float32)).astype(np.float64), None
    return dz0 @ W, (256 + 1.0) * U * (np.abs(dz0) @ np.abs(W))


def _pe40(pe):
    """The 40 PE slots chain_dpe_to_uv reads (the kernel's tile holds all ten octaves; rows of a narrower encoding are padded: their dPE is exactly 0)."""
    pe = np.asarray(pe, np.float64)[:, :40]
    out = np.zeros((len(pe), 40)); out[:, :pe.shape[1]] = pe
    return out


def _run_dpe(ar, dpe, pe, seed_uv, din_scale, mut):
    """mlp_common.h chain_dpe_to_uv: dpe, pe (rows, 40) in the reference's feature order 4 k + (sin u, sin v, cos u, cos v); seed_uv: the two lifted seed
    columns the `+=` lands on.  Returns the two lifted columns of the mapping net's output gradient."""
    res = []
    for i in (0, 1):
        halves = []
        for h in (0, 1):
            dx = ar.lift(np.zeros(len(pe)))
            for g in range(5):
                k = 2 * g + h
                b = float(np.ldexp(PI32, 2 * g if ("octave" in mut and h) else k))
                s_, c_ = ar.lift(pe[:, 4 * k + i]), ar.lift(pe[:, 4 * k + 2 + i])
                dx = dx + b * (c_ * dpe[:, 4 * k + i] - s_ * dpe[:, 4 * k + 2 + i])
            halves.append(dx)
        dx = halves[0] + halves[1]
        res.append(din_scale * dx if "assign" in mut else seed_uv[i] + din_scale * dx)
    return res


def dpe_to_uv_ref(dz0, W0, pe, seed, seed_err, din_scale=0.5, mut=()):
    """Rows of the mapping net's output gradient after the atlas chain's `+=`: (value (rows, 2), running error (rows, 2)) from the atlas net's dz plane 0, its
    layer-0 weights, its PE tile rows (rows, >= 40) and the loss seed (value, running error) of those rows."""
    v, b = dpe_product(dz0, W0)
    cols = _run_dpe(ArV, V(v, b), _pe40(pe), [V(seed[:, i], seed_err[:, i]) for i in (0, 1)], din_scale, frozenset(mut))
    return np.stack([c.v for c in cols], 1), np.stack([c.e for c in cols], 1)


def dpe_to_uv_emu(dz0, W0, pe, seed, din_scale=0.5, fused=False, mut=()):
    v, _ = dpe_product(dz0, W0, emulate=True)
    ar = ArF(fused)
    cols = _run_dpe(ar, F(v, fused), _pe40(pe), [ar.lift(seed[:, i]) for i in (0, 1)], din_scale, frozenset(mut))
    return np.stack([c.val() for c in cols], 1)
