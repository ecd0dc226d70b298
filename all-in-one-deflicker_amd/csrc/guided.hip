// guided.hip — residual guided transfer: a proxy-size correction carried to the full-size frame as a smooth gain / offset field, the device
// side of guided.py.  Per channel, independently: the fast guided filter (He & Sun) of the residual d = P - I with guide I.
//   k_guided_coeffs (proxy size): the window of a pixel is the (2r + 1)^2 square clipped to the frame, n its pixel count.  Exact integer
//     sums S_I, S_d, S_II, S_Id over the window (r <= 32: each below 4225 * 255^2 = 274 730 625, int32); num = n S_Id - S_I S_d and
//     den = n S_II - S_I^2 in int64; a = float(num) / (float(den) + eps * float(n * n)), b = (float(S_d) - a * float(S_I)) / float(n).
//   k_guided_smooth (proxy size): the box mean of a and of b over the same clipped window, in fp32 and in one fixed order: the row sums
//     left to right from 0.f, the sum of the row sums top to bottom from 0.f, one divide by float(n).
//   k_guided_apply (full size): abar and bbar sampled bilinearly at the full-size pixel centres, s = (X + 0.5) * (w / W) - 0.5 in fp64 clamped
//     to [0, w - 1] (the geometry of the any-size render, elem.hip coord_at), x0 = (int)s, x1 = min(x0 + 1, w - 1), ax = (float)(s - x0) (y
//     alike); v = top + ay * (bot - top) with top = v00 + ax * (v01 - v00), bot = v10 + ax * (v11 - v10) (exact on a constant field);
//     out = clamp(rint(F + (abar * F + bbar)), 0, 255), rint to even.  One kernel body for both sample depths: the policies Sample8 and
//     Sample16 below fix the packing, the clamps and the correction term of each.
// Every conversion, product, sum and quotient is one correctly rounded operation in the order written (contraction off), so the host may
// demand equality with a numpy restatement.  The two proxy-size kernels run separable box sums over an LDS tile of 32 x 16 outputs with a
// halo of r, one channel (coeffs) or one channel of one plane (smooth) per workgroup: at r = 32 the packed input tile (80 x 96 int32) and
// the three row-sum planes (80 x 32 int32 each) take 61 440 B, so the dynamic LDS never passes 64 KiB and two workgroups fit a CU; at the
// default r = 8 it is 18 KiB.  The integer sums add zeros outside the frame (order-free), the fp32 sums skip what is outside.  The apply
// kernel is memory-bound (3 B in, 3 B out per pixel, the coefficient planes in cache): 4 pixels per thread as one 12-byte load and one
// 12-byte store when W is a multiple of 4 and the pointers are 4-byte aligned, else bytes.  64-bit element offsets; no atomics.
// The colour guide (include/atlasfit.h af_guided_coeffs_colour): every output channel fitted on all three guide channels.
//   k_guided_moments (proxy size): the 21 exact window sums, six groups of three row-sum planes per tile, to int32 planes.
//   k_guided_solve (proxy size): per pixel the 3 x 3 system in fp64 by LDL^T in one written order, A (h, w, 9) and b (h, w, 3) in fp32.
//   k_guided_smooth<9>: the box means of the 12 planes; k_guided_apply<P, VEC, true>: t = A_k0 f_0 + A_k1 f_1 + A_k2 f_2 + b_k step by step.
#include "af_dev.h"
#include "elem.h"

#pragma clang fp contract(off)

namespace {

constexpr int TW = 32, TH = 16;      // outputs of one workgroup of 256 threads: 2 per thread

struct Tile {      // the geometry of one workgroup's tile with its halo
  int x0, y0, cols, rows;      // the frame position of tile entry (0, 0): x0 = first output column - r
};
__device__ __forceinline__ Tile tile_of(int r) {
  Tile t;
  t.x0 = blockIdx.x * TW - r; t.y0 = blockIdx.y * TH - r;
  t.cols = TW + 2 * r; t.rows = TH + 2 * r;
  return t;
}
__device__ __forceinline__ int window_side(int p, int r, int size) {      // pixels of [p - r, p + r] inside [0, size)
  const int lo = p - r < 0 ? 0 : p - r, hi = p + r > size - 1 ? size - 1 : p + r;
  return hi - lo + 1;
}

__global__ __launch_bounds__(256) void k_guided_coeffs(GuidedCoeffArgs g) {
  extern __shared__ int lds[];
  const Tile t = tile_of(g.r);
  const int ch = blockIdx.z, tid = threadIdx.x, win = 2 * g.r + 1;
  int* tile = lds;                                  // [rows][cols] I + (d << 16): I in 0..255, d in -255..255; 0 outside the frame
  int* hp = tile + t.rows * t.cols;                 // [rows][TW] row sums of the packed pairs (65 * 255 < 2^15: the halves cannot meet)
  int* hii = hp + t.rows * TW;                      // [rows][TW] row sums of I I
  int* hid = hii + t.rows * TW;                     // [rows][TW] row sums of I d
  for (int e = tid; e < t.rows * t.cols; e += 256) {
    const int ty = e / t.cols, tx = e - ty * t.cols, y = t.y0 + ty, x = t.x0 + tx;
    int v = 0;
    if (x >= 0 && x < g.w && y >= 0 && y < g.h) {
      const long long o = ((long long)y * g.w + x) * 3 + ch;
      const int i = g.I[o], d = (int)g.P[o] - i;
      v = i + d * 65536;
    }
    tile[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < t.rows * TW; e += 256) {
    const int ty = e / TW, tx = e - ty * TW;
    const int* row = tile + ty * t.cols + tx;
    int sp = 0, sii = 0, sid = 0;
    for (int k = 0; k < win; ++k) {
      const int v = row[k], i = v & 0xffff, d = v >> 16;
      sp += v; sii += i * i; sid += i * d;
    }
    hp[e] = sp; hii[e] = sii; hid[e] = sid;
  }
  __syncthreads();
  for (int e = tid; e < TW * TH; e += 256) {
    const int ty = e / TW, tx = e - ty * TW, y = blockIdx.y * TH + ty, x = blockIdx.x * TW + tx;
    if (x >= g.w || y >= g.h) continue;
    int si = 0, sd = 0, sii = 0, sid = 0;
    for (int k = 0; k < win; ++k) {
      const int o = (ty + k) * TW + tx, v = hp[o];
      si += v & 0xffff; sd += v >> 16; sii += hii[o]; sid += hid[o];
    }
    const int n = window_side(x, g.r, g.w) * window_side(y, g.r, g.h);
    const long long num = (long long)n * sid - (long long)si * sd, den = (long long)n * sii - (long long)si * si;
    const float a = (float)num / ((float)den + g.eps * (float)(n * n));
    const float b = ((float)sd - a * (float)si) / (float)n;
    const long long o = ((long long)y * g.w + x) * 3 + ch;
    g.a[o] = a;
    g.b[o] = b;
  }
}

// The colour guide's window sums.  Twenty-one sums laid out like the three row-sum planes above would take 215 KB at
// r = 32, so the work is split over blockIdx.z: each of 6 groups loads the same tile, packed as I_0 + (I_1 << 8) + (I_2 << 16) + (P_j << 24)
// with j = z % 3 (0 outside the frame, where d_j = P_j - I_j is 0 too), and forms three row-sum planes, the LDS of k_guided_coeffs:
//   z = 0..2   the packed pair (S_z, S_dz), and the two products 2z and 2z + 1 of the list 00 01 02 11 12 22
//   z = 3..5   S_0,dk, S_1,dk and S_2,dk of k = z - 3
// and writes its sums to the int32 planes of GuidedMomentArgs.S.  Integer sums: order-free.
constexpr int pair_u(int p) { return p < 3 ? 0 : p < 5 ? 1 : 2; }      // the channels of product p of 00 01 02 11 12 22
constexpr int pair_v(int p) { return p < 3 ? p : p < 5 ? p - 2 : 2; }

template <int Z> __device__ __forceinline__ void moments_group(const GuidedMomentArgs& g, int* lds) {
  constexpr int J = Z % 3;
  const Tile t = tile_of(g.r);
  const int tid = threadIdx.x, win = 2 * g.r + 1;
  unsigned int* tile = (unsigned int*)lds;          // [rows][cols]
  int* h0 = lds + t.rows * t.cols;                  // [rows][TW] each
  int* h1 = h0 + t.rows * TW;
  int* h2 = h1 + t.rows * TW;
  for (int e = tid; e < t.rows * t.cols; e += 256) {
    const int ty = e / t.cols, tx = e - ty * t.cols, y = t.y0 + ty, x = t.x0 + tx;
    unsigned int v = 0;
    if (x >= 0 && x < g.w && y >= 0 && y < g.h) {
      const long long o = ((long long)y * g.w + x) * 3;
      v = (unsigned int)g.I[o] | (unsigned int)g.I[o + 1] << 8 | (unsigned int)g.I[o + 2] << 16 | (unsigned int)g.P[o + J] << 24;
    }
    tile[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < t.rows * TW; e += 256) {
    const int ty = e / TW, tx = e - ty * TW;
    const unsigned int* row = tile + ty * t.cols + tx;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int k = 0; k < win; ++k) {
      const unsigned int v = row[k];
      const int i[3] = {(int)(v & 255u), (int)(v >> 8 & 255u), (int)(v >> 16 & 255u)};
      const int d = (int)(v >> 24) - i[J];
      if (Z < 3) {
        s0 += i[J] + d * 65536;                     // 65 * 255 < 2^15: the halves cannot meet
        s1 += i[pair_u(2 * J)] * i[pair_v(2 * J)];
        s2 += i[pair_u(2 * J + 1)] * i[pair_v(2 * J + 1)];
      } else {
        s0 += i[0] * d; s1 += i[1] * d; s2 += i[2] * d;
      }
    }
    h0[e] = s0; h1[e] = s1; h2[e] = s2;
  }
  __syncthreads();
  const long long hw = (long long)g.h * g.w;
  for (int e = tid; e < TW * TH; e += 256) {
    const int ty = e / TW, tx = e - ty * TW, y = blockIdx.y * TH + ty, x = blockIdx.x * TW + tx;
    if (x >= g.w || y >= g.h) continue;
    int s0 = 0, s0d = 0, s1 = 0, s2 = 0;
    for (int k = 0; k < win; ++k) {
      const int o = (ty + k) * TW + tx, v = h0[o];
      if (Z < 3) { s0 += v & 0xffff; s0d += v >> 16; } else { s0 += v; }
      s1 += h1[o]; s2 += h2[o];
    }
    int* out = g.S + ((long long)y * g.w + x);
    if (Z < 3) {
      out[J * hw] = s0; out[(3 + J) * hw] = s0d; out[(6 + 2 * J) * hw] = s1; out[(7 + 2 * J) * hw] = s2;
    } else {
      out[(12 + 3 * J) * hw] = s0; out[(13 + 3 * J) * hw] = s1; out[(14 + 3 * J) * hw] = s2;
    }
  }
}

__global__ __launch_bounds__(256) void k_guided_moments(GuidedMomentArgs g) {
  extern __shared__ int lds[];
  switch (blockIdx.z) {      // uniform over the workgroup
    case 0: moments_group<0>(g, lds); break;
    case 1: moments_group<1>(g, lds); break;
    case 2: moments_group<2>(g, lds); break;
    case 3: moments_group<3>(g, lds); break;
    case 4: moments_group<4>(g, lds); break;
    default: moments_group<5>(g, lds); break;
  }
}

// The colour guide's solve, one proxy pixel per thread: include/atlasfit.h af_guided_coeffs_colour writes the sequence out; every fp64
// operation below is one correctly rounded operation in that order (contraction off).
__global__ __launch_bounds__(256) void k_guided_solve(GuidedSolveArgs g) {
  const long long hw = (long long)g.h * g.w, p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int y = (int)(p / g.w), x = (int)(p - (long long)y * g.w);
  const int n = window_side(x, g.r, g.w) * window_side(y, g.r, g.h);
  long long S[21];
#pragma unroll
  for (int q = 0; q < 21; ++q) S[q] = g.S[q * hw + p];
  const double nd = (double)n, e = (double)g.eps * (double)(n * n);
  double m[6];      // Sigma + e I as 00 01 02 11 12 22
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    m[q] = (double)(n * S[6 + q] - S[pair_u(q)] * S[pair_v(q)]);
    if (pair_u(q) == pair_v(q)) m[q] = m[q] + e;
  }
  const double d0 = m[0], l10 = m[1] / d0, l20 = m[2] / d0;
  const double d1 = m[3] - l10 * m[1];
  const double t21 = m[4] - l20 * m[1], l21 = t21 / d1;
  const double d2 = (m[5] - l20 * m[2]) - l21 * t21;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double z0 = (double)(n * S[12 + 3 * k] - S[0] * S[3 + k]);
    const double z1 = (double)(n * S[13 + 3 * k] - S[1] * S[3 + k]) - l10 * z0;
    const double z2 = ((double)(n * S[14 + 3 * k] - S[2] * S[3 + k]) - l20 * z0) - l21 * z1;
    const double x2 = z2 / d2;
    const double x1 = z1 / d1 - l21 * x2;
    const double x0 = (z0 / d0 - l10 * x1) - l20 * x2;
    const double b = ((double)S[3 + k] - ((x0 * (double)S[0] + x1 * (double)S[1]) + x2 * (double)S[2])) / nd;
    g.A[p * 9 + 3 * k] = (float)x0; g.A[p * 9 + 3 * k + 1] = (float)x1; g.A[p * 9 + 3 * k + 2] = (float)x2;
    g.b[p * 3 + k] = (float)b;
  }
}

// The box means of NA + 3 planes: the channels of a (h, w, NA), then those of b (h, w, 3); NA is 3, or 9 for the colour guide.
template <int NA>
__global__ __launch_bounds__(256) void k_guided_smooth(GuidedSmoothArgs g) {
  extern __shared__ int lds[];
  const Tile t = tile_of(g.r);
  const bool of_a = blockIdx.z < NA;
  const int ch = of_a ? blockIdx.z : blockIdx.z - NA, nch = of_a ? NA : 3, tid = threadIdx.x;
  const float* src = of_a ? g.a : g.b;
  float* dst = of_a ? g.am : g.bm;
  float* tile = (float*)lds;                        // [rows][cols]; what lies outside the frame is never read
  float* hs = tile + t.rows * t.cols;               // [rows][TW] row sums over the clipped window, left to right
  for (int e = tid; e < t.rows * t.cols; e += 256) {
    const int ty = e / t.cols, tx = e - ty * t.cols, y = t.y0 + ty, x = t.x0 + tx;
    tile[e] = x >= 0 && x < g.w && y >= 0 && y < g.h ? src[((long long)y * g.w + x) * nch + ch] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < t.rows * TW; e += 256) {
    const int ty = e / TW, tx = e - ty * TW, x = blockIdx.x * TW + tx;
    const int lo = x - g.r < 0 ? 0 : x - g.r, hi = x + g.r > g.w - 1 ? g.w - 1 : x + g.r;      // past the frame's edge: a sum nobody reads
    const float* row = tile + ty * t.cols - t.x0;
    float s = 0.f;
    for (int k = lo; k <= hi; ++k) s += row[k];
    hs[e] = s;
  }
  __syncthreads();
  for (int e = tid; e < TW * TH; e += 256) {
    const int ty = e / TW, tx = e - ty * TW, y = blockIdx.y * TH + ty, x = blockIdx.x * TW + tx;
    if (x >= g.w || y >= g.h) continue;
    const int lo = y - g.r < 0 ? 0 : y - g.r, hi = y + g.r > g.h - 1 ? g.h - 1 : y + g.r;
    float s = 0.f;
    for (int k = lo; k <= hi; ++k) s += hs[(k - t.y0) * TW + tx];
    const int n = window_side(x, g.r, g.w) * (hi - lo + 1);
    dst[((long long)y * g.w + x) * nch + ch] = s / (float)n;
  }
}

struct AxisTap { int i0, i1; float f; };
__device__ __forceinline__ AxisTap axis_tap(int d, int src, double scale) {      // scale = (double)src / (double)dst, from the host
  double s = ((double)d + 0.5) * scale - 0.5;
  s = s < 0.0 ? 0.0 : s;
  s = s > (double)(src - 1) ? (double)(src - 1) : s;
  AxisTap t;
  t.i0 = (int)s;
  t.i1 = t.i0 + 1 < src ? t.i0 + 1 : src - 1;
  t.f = (float)(s - (double)t.i0);
  return t;
}
__device__ __forceinline__ float bil(const float* v, long long o00, long long o01, long long o10, long long o11, float ax, float ay) {
  const float v00 = v[o00], v01 = v[o01], v10 = v[o10], v11 = v[o11];
  const float top = v00 + ax * (v01 - v00), bot = v10 + ax * (v11 - v10);
  return top + ay * (bot - top);
}

// The one apply kernel over a sample policy P, 4 pixels (12 samples) per thread held as packed 32-bit words.  P supplies:
//   sample, args     the stored type and the argument block
//   BYTES, ALIGN     bytes per sample (12 * BYTES / 4 words per 4 pixels) and the alignment the vector path asks of the frame and the output:
//                    8-bit, one 12-byte load and store at 4; deep, three 8-byte ones at 8 (W a multiple of 4 makes a row a multiple of either)
//   ld(s, g)         the load clamp: a stored sample above M reads as M
//   maxf(g)          the upper clamp (float)M
//   corrected(f, abar, bbar, g)     the value before rint, each policy's own expression: its order of operations is part of the bytes
//   offset(bbar, g)  the colour guide's last term: bbar, or bbar * s at depth
struct Sample8 {
  typedef unsigned char sample;
  typedef GuidedApplyArgs args;
  enum { BYTES = 1, ALIGN = 4 };
  static __device__ __forceinline__ unsigned int ld(unsigned int s, const args&) { return s; }
  static __device__ __forceinline__ constexpr float maxf(const args&) { return 255.f; }
  static __device__ __forceinline__ float corrected(float f, float ab, float bb, const args&) { return f + (ab * f + bb); }
  static __device__ __forceinline__ float offset(float bb, const args&) { return bb; }
};
// A frame of D-bit samples held in uint16, M = 2^D - 1, with the planes of the 8-bit pair: f = (float)min(F, M), p = abar * f, q = bbar * s with
// s = (float)(M / 255.0) from the host, t = p + q, out = clamp(rint(f + t), 0, M).  At D = 8 s is 1 and q is bbar: the bytes of Sample8.
struct Sample16 {
  typedef unsigned short sample;
  typedef GuidedApply16Args args;
  enum { BYTES = 2, ALIGN = 8 };
  static __device__ __forceinline__ unsigned int ld(unsigned int s, const args& g) { const unsigned int m = (unsigned int)g.maxv; return s > m ? m : s; }
  static __device__ __forceinline__ float maxf(const args& g) { return (float)g.maxv; }
  static __device__ __forceinline__ float corrected(float f, float ab, float bb, const args& g) {
    const float p = ab * f, q = bb * g.s, t = p + q;
    return f + t;
  }
  static __device__ __forceinline__ float offset(float bb, const args& g) { return bb * g.s; }
};

template <class P> struct __attribute__((aligned(P::ALIGN))) Px4 { unsigned int w[3 * P::BYTES]; };      // 4 RGB pixels

// COLOUR: g.a is the nine-channel plane A (entry 3k + c) and, per output channel k, t = A_k0 f_0; t = t + A_k1 f_1;
// t = t + A_k2 f_2; t = t + P::offset(b_k); out_k = clamp(rint(f_k + t)), one fp32 operation per step.  With A = diag(a) the added terms
// are exact zeros and the bytes are the per-channel ones.
template <class P, bool VEC, bool COLOUR>
__global__ __launch_bounds__(256) void k_guided_apply(typename P::args g) {
  constexpr int WORDS = 3 * P::BYTES, PER = 4 / P::BYTES, SB = 8 * P::BYTES;      // words of 4 pixels, samples per word, bits per sample
  constexpr unsigned int MASK = (1u << SB) - 1u;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
  if (x4 >= g.W || y >= g.H) return;
  const AxisTap ty = axis_tap(y, g.h, g.scale_y);
  const long long base = ((long long)y * g.W + x4) * 3;
  const float maxf = P::maxf(g);
  Px4<P> in, out{};
  if (VEC) {
    in = *(const Px4<P>*)(g.F + base);
  } else {
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
      unsigned int v = 0;
#pragma unroll
      for (int k = 0; k < PER; ++k)
        if (x4 + (j * PER + k) / 3 < g.W) v |= (unsigned int)g.F[base + j * PER + k] << (SB * k);
      in.w[j] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x = x4 + i < g.W ? x4 + i : g.W - 1;      // past the row's end: computed on the last pixel, never stored
    const AxisTap tx = axis_tap(x, g.w, g.scale_x);
    const long long r0 = (long long)ty.i0 * g.w, r1 = (long long)ty.i1 * g.w;
    if constexpr (COLOUR) {
      const long long p00 = r0 + tx.i0, p01 = r0 + tx.i1, p10 = r1 + tx.i0, p11 = r1 + tx.i1;
      const float f0 = (float)P::ld((in.w[(i * 3) / PER] >> (SB * ((i * 3) % PER))) & MASK, g);
      const float f1 = (float)P::ld((in.w[(i * 3 + 1) / PER] >> (SB * ((i * 3 + 1) % PER))) & MASK, g);
      const float f2 = (float)P::ld((in.w[(i * 3 + 2) / PER] >> (SB * ((i * 3 + 2) % PER))) & MASK, g);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int j = i * 3 + k, q = 3 * k;
        float t = bil(g.a, p00 * 9 + q, p01 * 9 + q, p10 * 9 + q, p11 * 9 + q, tx.f, ty.f) * f0;
        t = t + bil(g.a, p00 * 9 + q + 1, p01 * 9 + q + 1, p10 * 9 + q + 1, p11 * 9 + q + 1, tx.f, ty.f) * f1;
        t = t + bil(g.a, p00 * 9 + q + 2, p01 * 9 + q + 2, p10 * 9 + q + 2, p11 * 9 + q + 2, tx.f, ty.f) * f2;
        t = t + P::offset(bil(g.b, p00 * 3 + k, p01 * 3 + k, p10 * 3 + k, p11 * 3 + k, tx.f, ty.f), g);
        float v = rintf((k == 0 ? f0 : k == 1 ? f1 : f2) + t);
        v = v > 0.f ? (v < maxf ? v : maxf) : 0.f;      // a NaN becomes 0
        out.w[j / PER] |= (unsigned int)v << (SB * (j % PER));
      }
    } else {
      const long long o00 = (r0 + tx.i0) * 3, o01 = (r0 + tx.i1) * 3, o10 = (r1 + tx.i0) * 3, o11 = (r1 + tx.i1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int j = i * 3 + c;
        const float f = (float)P::ld((in.w[j / PER] >> (SB * (j % PER))) & MASK, g);
        const float ab = bil(g.a, o00 + c, o01 + c, o10 + c, o11 + c, tx.f, ty.f);
        const float bb = bil(g.b, o00 + c, o01 + c, o10 + c, o11 + c, tx.f, ty.f);
        float v = rintf(P::corrected(f, ab, bb, g));
        v = v > 0.f ? (v < maxf ? v : maxf) : 0.f;      // a NaN becomes 0
        out.w[j / PER] |= (unsigned int)v << (SB * (j % PER));
      }
    }
  }
  if (VEC) {
    *(Px4<P>*)(g.out + base) = out;
  } else {
#pragma unroll
    for (int j = 0; j < WORDS; ++j)
#pragma unroll
      for (int k = 0; k < PER; ++k)
        if (x4 + (j * PER + k) / 3 < g.W) g.out[base + j * PER + k] = (typename P::sample)(out.w[j] >> (SB * k));
  }
}

// Grid (ceil(W / 256), ceil(H / 4)) of 64 x 4 threads, 4 pixels of a row per thread.
template <class P, bool COLOUR> int apply_launch(const typename P::args* a, hipStream_t s) {
  const dim3 grid((unsigned)((a->W + 255) / 256), (unsigned)((a->H + 3) / 4));
  const bool vec = a->W % 4 == 0 && ((uintptr_t)a->F | (uintptr_t)a->out) % P::ALIGN == 0;
  if (vec) hipLaunchKernelGGL((k_guided_apply<P, true, COLOUR>), grid, dim3(64, 4), 0, s, *a);
  else hipLaunchKernelGGL((k_guided_apply<P, false, COLOUR>), grid, dim3(64, 4), 0, s, *a);
  return (int)hipGetLastError();
}

dim3 tile_grid(int h, int w, int planes) { return dim3((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH), (unsigned)planes); }

}  // namespace

extern "C" {
// Grids: (ceil(w / 32), ceil(h / 16), 3 channels [x 2 planes]) of 256 threads; h, w <= 16384 keeps them inside the limits.  The dynamic LDS
// is at most 61 440 B (r = 32), below the 64 KiB a launch may ask for without an attribute.
int af_launch_guided_coeffs(const GuidedCoeffArgs* a, hipStream_t s) {
  const size_t rows = TH + 2 * a->r, cols = TW + 2 * a->r;
  hipLaunchKernelGGL(k_guided_coeffs, tile_grid(a->h, a->w, 3), dim3(256), (rows * cols + 3 * rows * TW) * 4, s, *a);
  return (int)hipGetLastError();
}
int af_launch_guided_smooth(const GuidedSmoothArgs* a, hipStream_t s) {
  const size_t rows = TH + 2 * a->r, cols = TW + 2 * a->r;
  hipLaunchKernelGGL(k_guided_smooth<3>, tile_grid(a->h, a->w, 6), dim3(256), (rows * cols + rows * TW) * 4, s, *a);
  return (int)hipGetLastError();
}
int af_launch_guided_apply(const GuidedApplyArgs* a, hipStream_t s) { return apply_launch<Sample8, false>(a, s); }
int af_launch_guided_apply16(const GuidedApply16Args* a, hipStream_t s) { return apply_launch<Sample16, false>(a, s); }
// The colour guide: the moments over 6 groups with the LDS of k_guided_coeffs, the solve one pixel per thread (h w <= 2^28: at most 2^20
// workgroups), the box means of 12 planes.
int af_launch_guided_moments(const GuidedMomentArgs* a, hipStream_t s) {
  const size_t rows = TH + 2 * a->r, cols = TW + 2 * a->r;
  hipLaunchKernelGGL(k_guided_moments, tile_grid(a->h, a->w, 6), dim3(256), (rows * cols + 3 * rows * TW) * 4, s, *a);
  return (int)hipGetLastError();
}
int af_launch_guided_solve(const GuidedSolveArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_guided_solve, dim3((unsigned)(((long long)a->h * a->w + 255) / 256)), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
int af_launch_guided_smooth_colour(const GuidedSmoothArgs* a, hipStream_t s) {
  const size_t rows = TH + 2 * a->r, cols = TW + 2 * a->r;
  hipLaunchKernelGGL(k_guided_smooth<9>, tile_grid(a->h, a->w, 12), dim3(256), (rows * cols + rows * TW) * 4, s, *a);
  return (int)hipGetLastError();
}
int af_launch_guided_apply_colour(const GuidedApplyArgs* a, hipStream_t s) { return apply_launch<Sample8, true>(a, s); }
int af_launch_guided_apply_colour16(const GuidedApply16Args* a, hipStream_t s) { return apply_launch<Sample16, true>(a, s); }
}
