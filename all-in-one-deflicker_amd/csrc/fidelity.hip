// fidelity.hip — PSNR and SSIM between two uint8 RGB sequences of one size, the device side of fidelity.py.  Every
// channel on its own; a frame is read as h rows of 3 w bytes, byte column xb = 3 x + c, so a window of win x win pixels of one channel
// is win rows of win bytes three apart.
//   SSE: the integer sum of (a - b)^2 over a frame and channel: exact, independent of any order.
//   SSIM (skimage.metrics.structural_similarity at its uint8 defaults: uniform window, sample covariance, K1 0.01, K2 0.03, range 255)
//     at every window that lies wholly inside the frame.  With N = win^2 the exact integer sums Sx, Sy, Sxx + Syy, Sxy of the window
//     (int32 in the passes, the products in int64), c1 = (0.01 * 255)^2 N^2 and c2 = (0.03 * 255)^2 N (N - 1) from the host in fp64:
//       A1 = (double)(2 Sx Sy) + c1            B1 = (double)(Sx^2 + Sy^2) + c1
//       A2 = (double)(2 (N Sxy - Sx Sy)) + c2  B2 = (double)((N Sxx - Sx^2) + (N Syy - Sy^2)) + c2       S = (A1 A2) / (B1 B2)
//     each fp64 operation one correctly rounded operation in the order written (contraction off); the integer in B2 is formed as
//     N (Sxx + Syy) - Sx^2 - Sy^2, the same integer.  Every integer is below 2^53, so its conversion is exact.
// k_fidelity_ssim (a template on the window size): one workgroup per (tile of 96 byte columns x 16 rows of windows, frame).  The tile plus its halo (3 (win - 1) byte
// columns, win - 1 rows) of both frames is staged in LDS as one 16-bit pair a | b << 8 per byte, read from HBM once per tile as dwords
// (bytes when a pointer is not 4-byte aligned or w is no multiple of 4: a row then starts anywhere); the row pass leaves three int32
// planes (Sx | Sy << 16, Sxx + Syy, Sxy of win bytes three apart), the column pass adds win of them.  At win = 15 the dynamic LDS is
// 42 960 B (tile 30 x 140 x 2, planes 3 x 30 x 96 x 4), at the default 7 it is 30 360 B: five workgroups fit a CU.  Consecutive lanes
// read consecutive 16-bit pairs (two lanes per bank, the same dword: a broadcast) and consecutive dwords: no bank conflicts.  The
// workgroup owns the bytes of its tile for the SSE (the last tile of an axis also the halo beyond it: every byte of a frame has one
// owner), so an SSIM call reads the frames once for both.  Per workgroup and channel one fp64 partial of S and one 64-bit partial of the
// SSE: shuffles inside a wave, four values through LDS, added as (0 + 1) + (2 + 3); the host adds the partials in block order.  No
// atomics: two calls agree bitwise.
// k_fidelity_sse: the SSE alone, a stream of 12-byte groups (four pixels) per thread, 24 576 bytes of a frame per workgroup.
// 64-bit offsets throughout: 16384^2 x 3 bytes x n passes 2^32.
#include "af_dev.h"
#include "elem.h"
#include "fidelity.h"

#pragma clang fp contract(off)

namespace {

constexpr int TBX = 3 * AF_FID_TILE_X, TY = AF_FID_TILE_Y;

// the three per-channel partials of a workgroup, in one fixed order
template <class T>
__device__ __forceinline__ void block_sum3(T v0, T v1, T v2, T (*red)[3], T* out) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { v0 += __shfl_xor(v0, o); v1 += __shfl_xor(v1, o); v2 += __shfl_xor(v2, o); }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = v0; red[wave][1] = v1; red[wave][2] = v2; }
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// WIN is a template argument: the tile's geometry is constant and the tap loops unroll (seven window sizes, two load paths).
template <bool VEC, int WIN>
__global__ __launch_bounds__(256) void k_fidelity_ssim(FidelityArgs g, int f0) {
  extern __shared__ __attribute__((aligned(16))) int lds[];      // the tile is written as 8-byte pairs
  __shared__ unsigned long long red_sse[4][3];
  __shared__ double red_ssim[4][3];
  constexpr int win = WIN;
  const int tid = threadIdx.x;
  constexpr int rows = TY + win - 1, cols = TBX + 3 * (win - 1), pitch = (cols + 3) & ~3;      // 16-bit pairs per tile row
  unsigned short* tile = (unsigned short*)lds;       // [rows][pitch] a | b << 8; 0 outside the frame
  unsigned int* hp = (unsigned int*)lds + rows * pitch / 2;      // [rows][TBX] Sx | Sy << 16 of a row (15 * 255 < 2^16)
  int* hq = (int*)hp + rows * TBX;                   // [rows][TBX] Sxx + Syy
  int* hxy = hq + rows * TBX;                        // [rows][TBX] Sxy
  const int W3 = 3 * g.w, OH = g.h - win + 1, OWB = 3 * (g.w - win + 1);
  const int x0 = blockIdx.x * TBX, y0 = blockIdx.y * TY, f = f0 + (int)blockIdx.z;
  const size_t fbase = (size_t)f * (size_t)g.h * (size_t)W3;
  const unsigned char* A = g.a + fbase;
  const unsigned char* B = g.b + fbase;
  // the bytes this workgroup owns for the SSE: its tile, and in the last tile of an axis everything up to the frame's edge
  const int own_x = blockIdx.x == gridDim.x - 1 ? W3 : x0 + TBX, own_y = blockIdx.y == gridDim.y - 1 ? g.h : y0 + TY;
  unsigned int s0 = 0, s1 = 0, s2 = 0;               // at most 17 bytes per thread and channel: below 2^32
  if (VEC) {
    constexpr int p4 = pitch / 4;
    for (int e = tid; e < rows * p4; e += 256) {
      const int ty = e / p4, q = e - ty * p4, y = y0 + ty, x = x0 + 4 * q;
      unsigned int av = 0, bv = 0;
      if (y < g.h && x < W3) {                       // W3 is a multiple of 4 here: the dword ends inside the row
        const size_t o = (size_t)y * (size_t)W3 + (size_t)x;
        av = *(const unsigned int*)(A + o);
        bv = *(const unsigned int*)(B + o);
      }
      uint2 pk;
      pk.x = (av & 0xffu) | ((bv & 0xffu) << 8) | ((av & 0xff00u) << 8) | ((bv & 0xff00u) << 16);
      pk.y = ((av >> 16) & 0xffu) | (((bv >> 16) & 0xffu) << 8) | ((av >> 24) << 16) | ((bv >> 24) << 24);
      ((uint2*)tile)[ty * p4 + q] = pk;
      if (y < own_y) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int d = (int)((av >> (8 * k)) & 255u) - (int)((bv >> (8 * k)) & 255u), c = (4 * q + k) % 3;      // x0 is a multiple of 3
          const unsigned int d2 = x + k < own_x ? (unsigned int)(d * d) : 0u;
          s0 += c == 0 ? d2 : 0u; s1 += c == 1 ? d2 : 0u; s2 += c == 2 ? d2 : 0u;
        }
      }
    }
  } else {
    for (int e = tid; e < rows * pitch; e += 256) {
      const int ty = e / pitch, tx = e - ty * pitch, y = y0 + ty, x = x0 + tx;
      unsigned int av = 0, bv = 0;
      if (y < g.h && x < W3) {
        const size_t o = (size_t)y * (size_t)W3 + (size_t)x;
        av = A[o]; bv = B[o];
      }
      tile[e] = (unsigned short)(av | (bv << 8));
      if (y < own_y && x < own_x) {
        const int d = (int)av - (int)bv, c = tx % 3;
        const unsigned int d2 = (unsigned int)(d * d);
        s0 += c == 0 ? d2 : 0u; s1 += c == 1 ? d2 : 0u; s2 += c == 2 ? d2 : 0u;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < rows * TBX; e += 256) {
    const int ty = e / TBX, tx = e - ty * TBX;
    const unsigned short* row = tile + ty * pitch + tx;
    unsigned int sp = 0; int sq = 0, sxy = 0;
#pragma unroll
    for (int k = 0; k < win; ++k) {
      const int v = row[3 * k], a = v & 0xff, b = v >> 8;
      sp += (unsigned int)a + ((unsigned int)b << 16); sq += a * a + b * b; sxy += a * b;
    }
    hp[e] = sp; hq[e] = sq; hxy[e] = sxy;
  }
  __syncthreads();
  const long long N = (long long)win * win;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  for (int e = tid; e < TBX * TY; e += 256) {
    const int ty = e / TBX, tx = e - ty * TBX, y = y0 + ty, xb = x0 + tx;
    if (y >= OH || xb >= OWB) continue;
    unsigned int sp = 0; int sq = 0, sxy = 0;        // 225 * 255 < 2^16; 225 * 2 * 255^2 and 225 * 255^2 fit int32
#pragma unroll
    for (int k = 0; k < win; ++k) {
      const int o = (ty + k) * TBX + tx;
      sp += hp[o]; sq += hq[o]; sxy += hxy[o];
    }
    const long long sx = sp & 0xffffu, sy = sp >> 16;
    const double A1 = (double)(2 * sx * sy) + g.c1;
    const double B1 = (double)(sx * sx + sy * sy) + g.c1;
    const double A2 = (double)(2 * (N * sxy - sx * sy)) + g.c2;
    const double B2 = (double)(N * sq - sx * sx - sy * sy) + g.c2;
    const double S = (A1 * A2) / (B1 * B2);
    if (g.map) g.map[((size_t)f * (size_t)OH + (size_t)y) * (size_t)OWB + (size_t)xb] = S;
    const int c = tx % 3;
    m0 += c == 0 ? S : 0.0; m1 += c == 1 ? S : 0.0; m2 += c == 2 ? S : 0.0;
  }
  const size_t blk = ((size_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  block_sum3<double>(m0, m1, m2, red_ssim, g.ssim_part + blk * 3);
  if (g.sse_part) block_sum3<unsigned long long>(s0, s1, s2, red_sse, g.sse_part + blk * 3);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_fidelity_sse(FidelityArgs g, int f0) {
  __shared__ unsigned long long red[4][3];
  const int f = f0 + (int)blockIdx.y;
  const size_t total = (size_t)g.h * (size_t)g.w * 3;
  const unsigned char* A = g.a + (size_t)f * total;
  const unsigned char* B = g.b + (size_t)f * total;
  unsigned int s[3] = {0, 0, 0};                     // 8 rounds of 4 bytes per channel: below 2^32
#pragma unroll
  for (int it = 0; it < AF_FID_SSE_BYTES / (256 * 12); ++it) {
    const size_t o = (size_t)blockIdx.x * AF_FID_SSE_BYTES + (size_t)(it * 256 + (int)threadIdx.x) * 12;      // a multiple of 3: byte j is channel j % 3
    if (o >= total) continue;
    if (VEC) {                                       // total is a multiple of 12 here: the group ends inside the frame
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned int av = *(const unsigned int*)(A + o + 4 * j), bv = *(const unsigned int*)(B + o + 4 * j);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int d = (int)((av >> (8 * k)) & 255u) - (int)((bv >> (8 * k)) & 255u);
          s[(4 * j + k) % 3] += (unsigned int)(d * d);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if (o + j < total) {
          const int d = (int)A[o + j] - (int)B[o + j];
          s[j % 3] += (unsigned int)(d * d);
        }
      }
    }
  }
  const size_t blk = (size_t)f * gridDim.x + blockIdx.x;
  block_sum3<unsigned long long>(s[0], s[1], s[2], red, g.sse_part + blk * 3);
}

}  // namespace

extern "C" {
// Grid (ceil(3 (w - win + 1) / 96), ceil((h - win + 1) / 16), frames) of 256 threads: at 16384 x 16384 it is 512 x 1024; a launch takes at
// most 65535 frames (gridDim.z), so a longer sequence goes in several.  Dynamic LDS at most 42 960 B.  The partials are
// [n][grid.y * grid.x][3].
int af_launch_fidelity_ssim(const FidelityArgs* a, hipStream_t s) {
  const int win = a->win, rows = TY + win - 1, pitch = (TBX + 3 * (win - 1) + 3) & ~3;
  const size_t lds_bytes = (size_t)rows * pitch * 2 + 3 * (size_t)rows * TBX * 4;
  const unsigned gx = (unsigned)((3 * (a->w - win + 1) + TBX - 1) / TBX), gy = (unsigned)((a->h - win + 1 + TY - 1) / TY);
  const bool vec = a->w % 4 == 0 && ((uintptr_t)a->a | (uintptr_t)a->b) % 4 == 0;
  for (int f0 = 0; f0 < a->n; f0 += 65535) {
    const int nf = a->n - f0 < 65535 ? a->n - f0 : 65535;
    const dim3 grid(gx, gy, (unsigned)nf);
    switch (win) {
#define AF_FID_CASE(W)                                                                                             \
      case W:                                                                                                      \
        if (vec) hipLaunchKernelGGL((k_fidelity_ssim<true, W>), grid, dim3(256), lds_bytes, s, *a, f0);            \
        else hipLaunchKernelGGL((k_fidelity_ssim<false, W>), grid, dim3(256), lds_bytes, s, *a, f0);               \
        break;
      AF_FID_CASE(3) AF_FID_CASE(5) AF_FID_CASE(7) AF_FID_CASE(9) AF_FID_CASE(11) AF_FID_CASE(13) AF_FID_CASE(15)
#undef AF_FID_CASE
      default: return (int)hipErrorInvalidValue;      // af_fidelity refuses every other window before it gets here
    }
    const int e = (int)hipGetLastError();
    if (e) return e;
  }
  return 0;
}
// Grid (ceil(3 h w / 24576), frames): at 16384 x 16384 it is 32768 wide.  The partials are [n][grid.x][3].
int af_launch_fidelity_sse(const FidelityArgs* a, hipStream_t s) {
  const size_t total = (size_t)a->h * (size_t)a->w * 3;
  const unsigned gx = (unsigned)((total + AF_FID_SSE_BYTES - 1) / AF_FID_SSE_BYTES);
  const bool vec = total % 12 == 0 && ((uintptr_t)a->a | (uintptr_t)a->b) % 4 == 0;
  for (int f0 = 0; f0 < a->n; f0 += 65535) {
    const int nf = a->n - f0 < 65535 ? a->n - f0 : 65535;
    if (vec) hipLaunchKernelGGL(k_fidelity_sse<true>, dim3(gx, (unsigned)nf), dim3(256), 0, s, *a, f0);
    else hipLaunchKernelGGL(k_fidelity_sse<false>, dim3(gx, (unsigned)nf), dim3(256), 0, s, *a, f0);
    const int e = (int)hipGetLastError();
    if (e) return e;
  }
  return 0;
}
}
