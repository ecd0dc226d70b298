// yuv.hip — YCbCr <-> RGB of one YUV4MPEG2 frame payload with chroma resampling (y4m.py).
// The payload is the Y plane h x w, then Cb, then Cr, each ch x cw; the image is (h, w, 3) uint8 RGB, HWC contiguous.  Integer
// arithmetic only: the result is exact and independent of any order, so the host may demand equality with numpy.
//   reading: chroma at a luma position is the bilinear interpolation there, edge clamped; the weights of an axis are quarters (centred
//     siting: 3/4 own sample, 1/4 the neighbour on the pixel's side; left-cosited: even x 1, odd x 1/2 + 1/2), so the interpolated
//     chroma is an integer c16 in units of 1/16.  acc = cy 16 (Y - y0) + cu (cb16 - 2048) + cv (cr16 - 2048) with coefficients of 14
//     fraction bits, out = clamp((acc + 2^17) >> 18): one rounding per byte.
//   writing: Y = clamp(((ky . rgb + 2^13) >> 14) + y0); chroma is ku . rgb / kv . rgb UNROUNDED per pixel (14 fraction bits), summed over the
//     taps of the sample (centred axis: its 2 pixels; left-cosited axis: [1, 2, 1] around luma column 2j; indices clamped, so an odd
//     edge replicates the last column / row), rounded once, plus 128, clamped.
// One thread per 2 x 2 luma block: its chroma fetch (a 3 x 3 neighbourhood at most) is shared by its four pixels, and on the way back
// its pixels are the taps of its chroma sample(s).  Byte loads and stores; no LDS, no atomics; 64-bit pixel offsets.
#include "af_dev.h"
#include "elem.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned char u8(int v) { return (unsigned char)clampi(v, 0, 255); }

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
template <int HM, int VM> __device__ __forceinline__ void chroma16(const unsigned char* plane, int ch, int cw, int bx, int by, int (&out)[2][2]) {
  int c[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const unsigned char* row = plane + (size_t)axis_index<VM>(by, r, ch) * (size_t)cw;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const bool used = (axis_weight<VM>(0, r) | axis_weight<VM>(1, r)) && (axis_weight<HM>(0, q) | axis_weight<HM>(1, q));
      c[r][q] = used ? (int)row[axis_index<HM>(bx, q, cw)] : 0;
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

template <int HM, int VM, bool MONO> __global__ __launch_bounds__(256) void k_yuv_to_rgb(YuvArgs a) {
  const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
  if (2 * bx >= a.w || 2 * by >= a.h) return;
  int cb[2][2] = {{2048, 2048}, {2048, 2048}}, cr[2][2] = {{2048, 2048}, {2048, 2048}};
  if (!MONO) {
    const unsigned char* pb = a.src + (size_t)a.h * (size_t)a.w;
    chroma16<HM, VM>(pb, a.ch, a.cw, bx, by, cb);
    chroma16<HM, VM>(pb + (size_t)a.ch * (size_t)a.cw, a.ch, a.cw, bx, by, cr);
  }
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int y = 2 * by + dy;
    if (y >= a.h) continue;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int x = 2 * bx + dx;
      if (x >= a.w) continue;
      const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
      const int l = a.cy * 16 * ((int)a.src[p] - a.y0) + (1 << 17);
      const int u = cb[dy][dx] - 2048, v = cr[dy][dx] - 2048;
      unsigned char* o = a.dst + p * 3;
      o[0] = u8((l + a.crv * v) >> 18);
      o[1] = u8((l + a.cgu * u + a.cgv * v) >> 18);
      o[2] = u8((l + a.cbu * u) >> 18);
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

template <int HM, int VM, bool MONO> __global__ __launch_bounds__(256) void k_rgb_to_yuv(YuvArgs a) {
  const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
  if (2 * bx >= a.w || 2 * by >= a.h) return;
  int cu[3][3], cv[3][3];                                     // unrounded chroma of the candidate pixels: rows 2by - 1 .. 2by + 1, columns 2bx - 1 .. 2bx + 1
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
      const unsigned char* s = a.src + p * 3;
      const int R = s[0], G = s[1], B = s[2];
      if (luma && 2 * by + r - 1 < a.h && 2 * bx + q - 1 < a.w) a.dst[p] = u8(((a.ky[0] * R + a.ky[1] * G + a.ky[2] * B + (1 << 13)) >> 14) + a.y0);
      if (chroma) {
        cu[r][q] = a.ku[0] * R + a.ku[1] * G + a.ku[2] * B;
        cv[r][q] = a.kv[0] * R + a.kv[1] * G + a.kv[2] * B;
      }
    }
  }
  if (MONO) return;
  constexpr int SH = 14 + tap_log2<HM>() + tap_log2<VM>();
  unsigned char* pb = a.dst + (size_t)a.h * (size_t)a.w;
  unsigned char* pr = pb + (size_t)a.ch * (size_t)a.cw;
#pragma unroll
  for (int sy = 0; sy < (VM == YUV_AXIS_FULL ? 2 : 1); ++sy) {
    const int j = VM == YUV_AXIS_FULL ? 2 * by + sy : by;
    if (j >= a.ch) continue;
#pragma unroll
    for (int sx = 0; sx < (HM == YUV_AXIS_FULL ? 2 : 1); ++sx) {
      const int i = HM == YUV_AXIS_FULL ? 2 * bx + sx : bx;
      if (i >= a.cw) continue;
      int su = 0, sv = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          su += tap<VM>(sy, r) * tap<HM>(sx, q) * cu[r][q];
          sv += tap<VM>(sy, r) * tap<HM>(sx, q) * cv[r][q];
        }
      const size_t c = (size_t)j * (size_t)a.cw + (size_t)i;
      pb[c] = u8(((su + (1 << (SH - 1))) >> SH) + 128);
      pr[c] = u8(((sv + (1 << (SH - 1))) >> SH) + 128);
    }
  }
}

template <bool TO_RGB, int HM, int VM, bool MONO> int launch(const YuvArgs* a, hipStream_t s) {
  const dim3 grid((unsigned)(((a->w + 1) / 2 + 63) / 64), (unsigned)(((a->h + 1) / 2 + 3) / 4)), block(64, 4);
  if (TO_RGB) hipLaunchKernelGGL((k_yuv_to_rgb<HM, VM, MONO>), grid, block, 0, s, *a);
  else hipLaunchKernelGGL((k_rgb_to_yuv<HM, VM, MONO>), grid, block, 0, s, *a);
  return (int)hipGetLastError();
}

template <bool TO_RGB> int dispatch(const YuvArgs* a, hipStream_t s) {
  if (a->mono) return launch<TO_RGB, YUV_AXIS_FULL, YUV_AXIS_FULL, true>(a, s);
  if (a->hmode == YUV_AXIS_FULL && a->vmode == YUV_AXIS_FULL) return launch<TO_RGB, YUV_AXIS_FULL, YUV_AXIS_FULL, false>(a, s);
  if (a->hmode == YUV_AXIS_COSITED && a->vmode == YUV_AXIS_FULL) return launch<TO_RGB, YUV_AXIS_COSITED, YUV_AXIS_FULL, false>(a, s);
  if (a->hmode == YUV_AXIS_CENTRED && a->vmode == YUV_AXIS_CENTRED) return launch<TO_RGB, YUV_AXIS_CENTRED, YUV_AXIS_CENTRED, false>(a, s);
  if (a->hmode == YUV_AXIS_COSITED && a->vmode == YUV_AXIS_CENTRED) return launch<TO_RGB, YUV_AXIS_COSITED, YUV_AXIS_CENTRED, false>(a, s);
  return (int)hipErrorInvalidValue;
}

}  // namespace

extern "C" {
// Grid (ceil(ceil(w / 2) / 64), ceil(ceil(h / 2) / 4)) of 64 x 4 threads: h, w <= 16384 keeps both far inside the grid limits.
int af_launch_yuv_to_rgb(const YuvArgs* a, hipStream_t s) { return dispatch<true>(a, s); }
int af_launch_rgb_to_yuv(const YuvArgs* a, hipStream_t s) { return dispatch<false>(a, s); }
}
