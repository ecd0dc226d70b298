// yuv16.hip — YCbCr <-> RGB of one YUV4MPEG2 frame payload of more than 8 bits per sample, and the reduction of such samples to bytes
// (y4m.py, guided.py).  A sample is a uint16 holding D bits, M = 2^D - 1; a stored sample above M reads as M.
// The conversions are yuv.hip's arithmetic restated at depth D: the same planes, sitings, weights, taps and clamped indices, coefficients of
// Q = D + 6 fraction bits (14 at D = 8), y0 = 16 2^(D-8) or 0, the chroma centre C = 2^(D-1).
//   reading: acc = cy 16 (Y - y0) + cu (cb16 - 16 C) + cv (cr16 - 16 C), out = clamp((acc + 2^(Q+3)) >> (Q+4), 0, M).
//   writing: Y = clamp(((ky . rgb + 2^(Q-1)) >> Q) + y0, 0, M); chroma unrounded per pixel, summed over the taps, rounded once by
//     Q + log2 of the taps' sum, plus C, clamped.
// The interpolated chroma (at most 16 * 65535) and the coefficients (below 2.2 * 2^22) are ints; every product and sum of the matrix is
// int64 (a luma product reaches 2^43 at D = 16).  Integer arithmetic only: exact and independent of any order.  One thread per 2 x 2 luma
// block as in yuv.hip; 16-bit loads and stores; no LDS, no atomics; 64-bit element offsets.
//   k_depth_reduce: v8 = (510 min(v, M) + M) / (2 M), integer division (510 * 65535 + 65535 < 2^26).  A thread owns 8 consecutive samples:
//     one 16-byte load and one 8-byte store where the pointers allow it and the group is whole, else element by element.
#include "af_dev.h"
#include "elem.h"

namespace {

typedef long long i64;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned short sat(i64 v, int maxv) { return (unsigned short)(v < 0 ? 0 : (v > (i64)maxv ? (i64)maxv : v)); }
__device__ __forceinline__ int ld(const unsigned short* p, int maxv) { const int v = *p; return v > maxv ? maxv : v; }

// The weights (quarters) and indices of the three candidate samples of one axis: yuv.hip's, unchanged.
template <int MODE> __device__ __forceinline__ int axis_weight(int d, int k) {
  if (MODE == YUV_AXIS_FULL) return (d == 0 ? (k == 1) : (k == 2)) ? 4 : 0;
  if (MODE == YUV_AXIS_CENTRED) return k == 1 ? 3 : ((d == 0 ? k == 0 : k == 2) ? 1 : 0);
  return d == 0 ? (k == 1 ? 4 : 0) : (k == 0 ? 0 : 2);      // left-cosited
}
template <int MODE> __device__ __forceinline__ int axis_index(int b, int k, int n) {
  return MODE == YUV_AXIS_FULL ? clampi(2 * b + k - 1, 0, n - 1) : clampi(b + k - 1, 0, n - 1);
}

// c16 of the four pixels of block (bx, by) from one chroma plane.
template <int HM, int VM> __device__ __forceinline__ void chroma16(const unsigned short* plane, int ch, int cw, int bx, int by, int maxv, int (&out)[2][2]) {
  int c[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const unsigned short* row = plane + (size_t)axis_index<VM>(by, r, ch) * (size_t)cw;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const bool used = (axis_weight<VM>(0, r) | axis_weight<VM>(1, r)) && (axis_weight<HM>(0, q) | axis_weight<HM>(1, q));
      c[r][q] = used ? ld(row + axis_index<HM>(bx, q, cw), maxv) : 0;
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

template <int HM, int VM, bool MONO> __global__ __launch_bounds__(256) void k_yuv_to_rgb16(Yuv16Args a) {
  const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
  if (2 * bx >= a.w || 2 * by >= a.h) return;
  int cb[2][2] = {{a.c16, a.c16}, {a.c16, a.c16}}, cr[2][2] = {{a.c16, a.c16}, {a.c16, a.c16}};
  if (!MONO) {
    const unsigned short* pb = a.src + (size_t)a.h * (size_t)a.w;
    chroma16<HM, VM>(pb, a.ch, a.cw, bx, by, a.maxv, cb);
    chroma16<HM, VM>(pb + (size_t)a.ch * (size_t)a.cw, a.ch, a.cw, bx, by, a.maxv, cr);
  }
  const int sh = a.q + 4;
  const i64 half = (i64)1 << (a.q + 3);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int y = 2 * by + dy;
    if (y >= a.h) continue;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int x = 2 * bx + dx;
      if (x >= a.w) continue;
      const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
      const i64 l = (i64)a.cy * (i64)(16 * (ld(a.src + p, a.maxv) - a.y0)) + half;
      const i64 u = cb[dy][dx] - a.c16, v = cr[dy][dx] - a.c16;
      unsigned short* o = a.dst + p * 3;
      o[0] = sat((l + (i64)a.crv * v) >> sh, a.maxv);
      o[1] = sat((l + (i64)a.cgu * u + (i64)a.cgv * v) >> sh, a.maxv);
      o[2] = sat((l + (i64)a.cbu * u) >> sh, a.maxv);
    }
  }
}

// The taps of one axis over the block's three candidate pixels 2b - 1, 2b, 2b + 1 (clamped): yuv.hip's, unchanged.
template <int MODE> __device__ __forceinline__ int tap(int s, int k) {
  if (MODE == YUV_AXIS_FULL) return k == s + 1 ? 1 : 0;
  if (MODE == YUV_AXIS_CENTRED) return k == 0 ? 0 : 1;
  return k == 1 ? 2 : 1;                                      // left-cosited: [1, 2, 1] around 2b
}
template <int MODE> __device__ __forceinline__ constexpr int tap_log2() { return MODE == YUV_AXIS_FULL ? 0 : (MODE == YUV_AXIS_CENTRED ? 1 : 2); }

template <int HM, int VM, bool MONO> __global__ __launch_bounds__(256) void k_rgb_to_yuv16(Yuv16Args a) {
  const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
  if (2 * bx >= a.w || 2 * by >= a.h) return;
  i64 cu[3][3], cv[3][3];                                     // unrounded chroma of the candidate pixels
  const i64 yhalf = (i64)1 << (a.q - 1);
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
      const unsigned short* s = a.src + p * 3;
      const i64 R = ld(s, a.maxv), G = ld(s + 1, a.maxv), B = ld(s + 2, a.maxv);
      if (luma && 2 * by + r - 1 < a.h && 2 * bx + q - 1 < a.w) a.dst[p] = sat(((a.ky[0] * R + a.ky[1] * G + a.ky[2] * B + yhalf) >> a.q) + a.y0, a.maxv);
      if (chroma) {
        cu[r][q] = a.ku[0] * R + a.ku[1] * G + a.ku[2] * B;
        cv[r][q] = a.kv[0] * R + a.kv[1] * G + a.kv[2] * B;
      }
    }
  }
  if (MONO) return;
  const int sh = a.q + tap_log2<HM>() + tap_log2<VM>();
  const i64 chalf = (i64)1 << (sh - 1), centre = a.c16 >> 4;
  unsigned short* pb = a.dst + (size_t)a.h * (size_t)a.w;
  unsigned short* pr = pb + (size_t)a.ch * (size_t)a.cw;
#pragma unroll
  for (int sy = 0; sy < (VM == YUV_AXIS_FULL ? 2 : 1); ++sy) {
    const int j = VM == YUV_AXIS_FULL ? 2 * by + sy : by;
    if (j >= a.ch) continue;
#pragma unroll
    for (int sx = 0; sx < (HM == YUV_AXIS_FULL ? 2 : 1); ++sx) {
      const int i = HM == YUV_AXIS_FULL ? 2 * bx + sx : bx;
      if (i >= a.cw) continue;
      i64 su = 0, sv = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          su += tap<VM>(sy, r) * tap<HM>(sx, q) * cu[r][q];
          sv += tap<VM>(sy, r) * tap<HM>(sx, q) * cv[r][q];
        }
      const size_t c = (size_t)j * (size_t)a.cw + (size_t)i;
      pb[c] = sat(((su + chalf) >> sh) + centre, a.maxv);
      pr[c] = sat(((sv + chalf) >> sh) + centre, a.maxv);
    }
  }
}

template <bool TO_RGB, int HM, int VM, bool MONO> int launch(const Yuv16Args* a, hipStream_t s) {
  const dim3 grid((unsigned)(((a->w + 1) / 2 + 63) / 64), (unsigned)(((a->h + 1) / 2 + 3) / 4)), block(64, 4);
  if (TO_RGB) hipLaunchKernelGGL((k_yuv_to_rgb16<HM, VM, MONO>), grid, block, 0, s, *a);
  else hipLaunchKernelGGL((k_rgb_to_yuv16<HM, VM, MONO>), grid, block, 0, s, *a);
  return (int)hipGetLastError();
}

template <bool TO_RGB> int dispatch(const Yuv16Args* a, hipStream_t s) {
  if (a->mono) return launch<TO_RGB, YUV_AXIS_FULL, YUV_AXIS_FULL, true>(a, s);
  if (a->hmode == YUV_AXIS_FULL && a->vmode == YUV_AXIS_FULL) return launch<TO_RGB, YUV_AXIS_FULL, YUV_AXIS_FULL, false>(a, s);
  if (a->hmode == YUV_AXIS_COSITED && a->vmode == YUV_AXIS_FULL) return launch<TO_RGB, YUV_AXIS_COSITED, YUV_AXIS_FULL, false>(a, s);
  if (a->hmode == YUV_AXIS_CENTRED && a->vmode == YUV_AXIS_CENTRED) return launch<TO_RGB, YUV_AXIS_CENTRED, YUV_AXIS_CENTRED, false>(a, s);
  if (a->hmode == YUV_AXIS_COSITED && a->vmode == YUV_AXIS_CENTRED) return launch<TO_RGB, YUV_AXIS_COSITED, YUV_AXIS_CENTRED, false>(a, s);
  return (int)hipErrorInvalidValue;
}

template <bool VEC> __global__ __launch_bounds__(256) void k_depth_reduce(DepthReduceArgs a) {
  const i64 base = ((i64)blockIdx.x * 256 + threadIdx.x) * 8;
  if (base >= a.count) return;
  const unsigned m = (unsigned)a.maxv, den = 2u * m;
  if (VEC && base + 8 <= a.count) {
    const uint4 in = *(const uint4*)(a.src + base);
    const unsigned w[4] = {in.x, in.y, in.z, in.w};
    unsigned o[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      unsigned v = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
      v = v > m ? m : v;
      o[k >> 2] |= ((510u * v + m) / den) << (8 * (k & 3));
    }
    *(uint2*)(a.dst + base) = make_uint2(o[0], o[1]);
    return;
  }
  for (int k = 0; k < 8 && base + k < a.count; ++k) {
    unsigned v = a.src[base + k];
    v = v > m ? m : v;
    a.dst[base + k] = (unsigned char)((510u * v + m) / den);
  }
}

}  // namespace

extern "C" {
// Grid (ceil(ceil(w / 2) / 64), ceil(ceil(h / 2) / 4)) of 64 x 4 threads, as in yuv.hip.
int af_launch_yuv_to_rgb16(const Yuv16Args* a, hipStream_t s) { return dispatch<true>(a, s); }
int af_launch_rgb_to_yuv16(const Yuv16Args* a, hipStream_t s) { return dispatch<false>(a, s); }
// Grid ceil(count / 2048) of 256 threads: count <= 2^32 keeps it at 2^21 workgroups.
int af_launch_depth_reduce(const DepthReduceArgs* a, hipStream_t s) {
  const dim3 grid((unsigned)((a->count + 2047) / 2048));
  const bool vec = (uintptr_t)a->src % 16 == 0 && (uintptr_t)a->dst % 8 == 0;
  if (vec) hipLaunchKernelGGL(k_depth_reduce<true>, grid, dim3(256), 0, s, *a);
  else hipLaunchKernelGGL(k_depth_reduce<false>, grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
}
