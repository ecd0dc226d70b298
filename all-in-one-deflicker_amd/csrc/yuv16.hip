// yuv16.hip — YCbCr <-> RGB of one YUV4MPEG2 frame payload of more than 8 bits per sample, and the reduction of such samples to bytes
// (y4m.py, guided.py).  The conversions are the kernels of yuv_core.h at the depth policy below: a sample is a uint16
// holding D bits, a stored sample above M = 2^D - 1 reads as M (every load is clamped); Q = D + 6 (14 at D = 8), M and 16 C = 2^(D+3) come
// from the argument block.  The interpolated chroma (at most 16 * 65535) and the coefficients (below 2.2 * 2^22) are ints; every product
// and sum of the matrix is int64 (a luma product reaches 2^43 at D = 16).
//   k_depth_reduce: v8 = (510 min(v, M) + M) / (2 M), integer division (510 * 65535 + 65535 < 2^26).  A thread owns 8 consecutive samples:
//     one 16-byte load and one 8-byte store where the pointers allow it and the group is whole, else element by element.
#include "yuv_core.h"

namespace {

typedef long long i64;

struct DepthN {
  typedef unsigned short sample;
  typedef i64 acc;
  typedef Yuv16Args args;
  static __device__ __forceinline__ int q(const args& a) { return a.q; }
  static __device__ __forceinline__ int c16(const args& a) { return a.c16; }
  static __device__ __forceinline__ int ld(const sample* p, const args& a) { const int v = *p; return v > a.maxv ? a.maxv : v; }
  static __device__ __forceinline__ sample sat(i64 v, const args& a) { return (sample)(v < 0 ? 0 : (v > (i64)a.maxv ? (i64)a.maxv : v)); }
};

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
int af_launch_yuv_to_rgb16(const Yuv16Args* a, hipStream_t s) { return yuv_dispatch<DepthN, true>(a, s); }
int af_launch_rgb_to_yuv16(const Yuv16Args* a, hipStream_t s) { return yuv_dispatch<DepthN, false>(a, s); }
// Grid ceil(count / 2048) of 256 threads: count <= 2^32 keeps it at 2^21 workgroups.
int af_launch_depth_reduce(const DepthReduceArgs* a, hipStream_t s) {
  const dim3 grid((unsigned)((a->count + 2047) / 2048));
  const bool vec = (uintptr_t)a->src % 16 == 0 && (uintptr_t)a->dst % 8 == 0;
  if (vec) hipLaunchKernelGGL(k_depth_reduce<true>, grid, dim3(256), 0, s, *a);
  else hipLaunchKernelGGL(k_depth_reduce<false>, grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
}
