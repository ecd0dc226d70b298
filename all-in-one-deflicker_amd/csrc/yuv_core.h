// yuv_core.h — the one body of the YCbCr <-> RGB kernels of a YUV4MPEG2 frame payload, for every sample depth.
// yuv.hip and yuv16.hip each define a depth policy P, include this header and export their two af_launch_* entries with one line each.
// The payload is the Y plane h x w, then Cb, then Cr, each ch x cw; the image is (h, w, 3) samples RGB, HWC contiguous.  Integer arithmetic
// only: the result is exact and independent of any order, so the host may demand equality with numpy.  A sample holds D bits, M = 2^D - 1,
// the coefficients have Q = D + 6 fraction bits, y0 is 16 2^(D-8) or 0, the chroma centre C = 2^(D-1).
//   reading: chroma at a luma position is the bilinear interpolation there, edge clamped; the weights of an axis are quarters (centred
//     siting: 3/4 own sample, 1/4 the neighbour on the pixel's side; left-cosited: even x 1, odd x 1/2 + 1/2), so the interpolated
//     chroma is an integer c16 in units of 1/16.  acc = cy 16 (Y - y0) + cu (cb16 - 16 C) + cv (cr16 - 16 C),
//     out = clamp((acc + 2^(Q+3)) >> (Q+4), 0, M): one rounding per sample.
//   writing: Y = clamp(((ky . rgb + 2^(Q-1)) >> Q) + y0, 0, M); chroma is ku . rgb / kv . rgb UNROUNDED per pixel (Q fraction bits), summed
//     over the taps of the sample (centred axis: its 2 pixels; left-cosited axis: [1, 2, 1] around luma column 2j; indices clamped, so an
//     odd edge replicates the last column / row), rounded once by Q + log2 of the taps' sum, plus C, clamped.
// One thread per 2 x 2 luma block: its chroma fetch (a 3 x 3 neighbourhood at most) is shared by its four pixels, and on the way back
// its pixels are the taps of its chroma sample(s).  Sample loads and stores; no LDS, no atomics; 64-bit element offsets.
// A depth policy P supplies:
//   sample, acc, args       the stored type, the type of every product and sum of the matrix, the argument block (YuvArgs / Yuv16Args)
//   q(a), c16(a)            Q and 16 C: compile-time constants or fields of the block
//   ld(p, a), sat(v, a)     a sample as an int (clamped to M where the type can hold more), an acc clamped to 0..M as a sample
#pragma once
#include "af_dev.h"
#include "elem.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The weights (quarters) of the three candidate samples of one axis for the two pixels d = 0, 1 of a block, and their indices.
// FULL: the plane is not subsampled, the candidates are the block's own two samples.  Subsampled: samples b - 1, b, b + 1.
template <int MODE> __device__ __forceinline__ int axis_weight(int d, int k) {
  if (MODE == YUV_AXIS_FULL) return (d == 0 ? (k == 1) : (k == 2)) ? 4 : 0;
  if (MODE == YUV_AXIS_CENTRED) return k == 1 ? 3 : ((d == 0 ? k == 0 : k == 2) ? 1 : 0);
  return d == 0 ? (k == 1 ? 4 : 0) : (k == 0 ? 0 : 2);      // left-cosited
}
template <int MODE> __device__ __forceinline__ int axis_index(int b, int k, int n) {      // n: samples of the plane along this axis
  return MODE == YUV_AXIS_FULL ? clampi(2 * b + k - 1, 0, n - 1) : clampi(b + k - 1, 0, n - 1);
}

// c16 of the four pixels of block (bx, by) from one chroma plane.
template <class P, int HM, int VM>
__device__ __forceinline__ void chroma16(const typename P::sample* plane, const typename P::args& a, int bx, int by, int (&out)[2][2]) {
  int c[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const typename P::sample* row = plane + (size_t)axis_index<VM>(by, r, a.ch) * (size_t)a.cw;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const bool used = (axis_weight<VM>(0, r) | axis_weight<VM>(1, r)) && (axis_weight<HM>(0, q) | axis_weight<HM>(1, q));
      c[r][q] = used ? P::ld(row + axis_index<HM>(bx, q, a.cw), a) : 0;
    }
  }
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      int s = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) s += axis_weight<VM>(dy, r) * axis_weight<HM>(dx, q) * c[r][q];
      out[dy][dx] = s;
    }
}

template <class P, int HM, int VM, bool MONO> __global__ __launch_bounds__(256) void k_yuv_to_rgb(typename P::args a) {
  typedef typename P::acc A;
  const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
  if (2 * bx >= a.w || 2 * by >= a.h) return;
  const int c16 = P::c16(a), sh = P::q(a) + 4;
  int cb[2][2] = {{c16, c16}, {c16, c16}}, cr[2][2] = {{c16, c16}, {c16, c16}};
  if (!MONO) {
    const typename P::sample* pb = a.src + (size_t)a.h * (size_t)a.w;
    chroma16<P, HM, VM>(pb, a, bx, by, cb);
    chroma16<P, HM, VM>(pb + (size_t)a.ch * (size_t)a.cw, a, bx, by, cr);
  }
  const A half = (A)1 << (sh - 1);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int y = 2 * by + dy;
    if (y >= a.h) continue;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int x = 2 * bx + dx;
      if (x >= a.w) continue;
      const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
      const A l = (A)(a.cy * 16) * (A)(P::ld(a.src + p, a) - a.y0) + half;      // cy 16 stays below 2^27 at every depth
      const A u = cb[dy][dx] - c16, v = cr[dy][dx] - c16;
      typename P::sample* o = a.dst + p * 3;
      o[0] = P::sat((l + (A)a.crv * v) >> sh, a);
      o[1] = P::sat((l + (A)a.cgu * u + (A)a.cgv * v) >> sh, a);
      o[2] = P::sat((l + (A)a.cbu * u) >> sh, a);
    }
  }
}

// The taps of one axis over the block's three candidate pixels 2b - 1, 2b, 2b + 1 (clamped), for chroma sample s of the block: FULL has
// two samples (pixel 2b + s alone), a subsampled axis one.
template <int MODE> __device__ __forceinline__ int tap(int s, int k) {
  if (MODE == YUV_AXIS_FULL) return k == s + 1 ? 1 : 0;
  if (MODE == YUV_AXIS_CENTRED) return k == 0 ? 0 : 1;
  return k == 1 ? 2 : 1;                                      // left-cosited: [1, 2, 1] around 2b
}
template <int MODE> __device__ __forceinline__ constexpr int tap_log2() { return MODE == YUV_AXIS_FULL ? 0 : (MODE == YUV_AXIS_CENTRED ? 1 : 2); }

template <class P, int HM, int VM, bool MONO> __global__ __launch_bounds__(256) void k_rgb_to_yuv(typename P::args a) {
  typedef typename P::acc A;
  const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
  if (2 * bx >= a.w || 2 * by >= a.h) return;
  A cu[3][3], cv[3][3];                                       // unrounded chroma of the candidate pixels: rows 2by - 1 .. 2by + 1, columns 2bx - 1 .. 2bx + 1
  const int Q = P::q(a);
  const A yhalf = (A)1 << (Q - 1);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int y = clampi(2 * by + r - 1, 0, a.h - 1);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int x = clampi(2 * bx + q - 1, 0, a.w - 1);
      const bool luma = r > 0 && q > 0;                       // one of the block's own four pixels
      const bool chroma = !MONO && (tap<VM>(0, r) | tap<VM>(1, r)) && (tap<HM>(0, q) | tap<HM>(1, q));
      cu[r][q] = cv[r][q] = 0;
      if (!luma && !chroma) continue;
      const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
      const typename P::sample* s = a.src + p * 3;
      const A R = P::ld(s, a), G = P::ld(s + 1, a), B = P::ld(s + 2, a);
      if (luma && 2 * by + r - 1 < a.h && 2 * bx + q - 1 < a.w) a.dst[p] = P::sat(((a.ky[0] * R + a.ky[1] * G + a.ky[2] * B + yhalf) >> Q) + a.y0, a);
      if (chroma) {
        cu[r][q] = a.ku[0] * R + a.ku[1] * G + a.ku[2] * B;
        cv[r][q] = a.kv[0] * R + a.kv[1] * G + a.kv[2] * B;
      }
    }
  }
  if (MONO) return;
  const int sh = Q + tap_log2<HM>() + tap_log2<VM>();
  const A chalf = (A)1 << (sh - 1), centre = P::c16(a) >> 4;
  typename P::sample* pb = a.dst + (size_t)a.h * (size_t)a.w;
  typename P::sample* pr = pb + (size_t)a.ch * (size_t)a.cw;
#pragma unroll
  for (int sy = 0; sy < (VM == YUV_AXIS_FULL ? 2 : 1); ++sy) {
    const int j = VM == YUV_AXIS_FULL ? 2 * by + sy : by;
    if (j >= a.ch) continue;
#pragma unroll
    for (int sx = 0; sx < (HM == YUV_AXIS_FULL ? 2 : 1); ++sx) {
      const int i = HM == YUV_AXIS_FULL ? 2 * bx + sx : bx;
      if (i >= a.cw) continue;
      A su = 0, sv = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          su += tap<VM>(sy, r) * tap<HM>(sx, q) * cu[r][q];
          sv += tap<VM>(sy, r) * tap<HM>(sx, q) * cv[r][q];
        }
      const size_t c = (size_t)j * (size_t)a.cw + (size_t)i;
      pb[c] = P::sat(((su + chalf) >> sh) + centre, a);
      pr[c] = P::sat(((sv + chalf) >> sh) + centre, a);
    }
  }
}

// Grid (ceil(ceil(w / 2) / 64), ceil(ceil(h / 2) / 4)) of 64 x 4 threads: h, w <= 16384 keeps both far inside the grid limits.
template <class P, bool TO_RGB, int HM, int VM, bool MONO> int yuv_launch(const typename P::args* a, hipStream_t s) {
  const dim3 grid((unsigned)(((a->w + 1) / 2 + 63) / 64), (unsigned)(((a->h + 1) / 2 + 3) / 4)), block(64, 4);
  if (TO_RGB) hipLaunchKernelGGL((k_yuv_to_rgb<P, HM, VM, MONO>), grid, block, 0, s, *a);
  else hipLaunchKernelGGL((k_rgb_to_yuv<P, HM, VM, MONO>), grid, block, 0, s, *a);
  return (int)hipGetLastError();
}

template <class P, bool TO_RGB> int yuv_dispatch(const typename P::args* a, hipStream_t s) {
  if (a->mono) return yuv_launch<P, TO_RGB, YUV_AXIS_FULL, YUV_AXIS_FULL, true>(a, s);
  if (a->hmode == YUV_AXIS_FULL && a->vmode == YUV_AXIS_FULL) return yuv_launch<P, TO_RGB, YUV_AXIS_FULL, YUV_AXIS_FULL, false>(a, s);
  if (a->hmode == YUV_AXIS_COSITED && a->vmode == YUV_AXIS_FULL) return yuv_launch<P, TO_RGB, YUV_AXIS_COSITED, YUV_AXIS_FULL, false>(a, s);
  if (a->hmode == YUV_AXIS_CENTRED && a->vmode == YUV_AXIS_CENTRED) return yuv_launch<P, TO_RGB, YUV_AXIS_CENTRED, YUV_AXIS_CENTRED, false>(a, s);
  if (a->hmode == YUV_AXIS_COSITED && a->vmode == YUV_AXIS_CENTRED) return yuv_launch<P, TO_RGB, YUV_AXIS_COSITED, YUV_AXIS_CENTRED, false>(a, s);
  return (int)hipErrorInvalidValue;
}

}  // namespace
