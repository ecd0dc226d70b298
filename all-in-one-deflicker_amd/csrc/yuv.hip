// yuv.hip — YCbCr <-> RGB of one YUV4MPEG2 frame payload of 8 bits per sample (y4m.py): the kernels of yuv_core.h at the
// depth policy below.  Everything the depth decides is a compile-time constant here: byte samples, int products and sums, Q = 14 (the
// reading shift is 18, the writing shift 14 + log2 of the taps' sum), 16 C = 2048, M = 255; a byte cannot exceed M, so a load is not clamped.
#include "yuv_core.h"

namespace {

struct Depth8 {
  typedef unsigned char sample;
  typedef int acc;
  typedef YuvArgs args;
  static __device__ __forceinline__ constexpr int q(const args&) { return 14; }
  static __device__ __forceinline__ constexpr int c16(const args&) { return 2048; }
  static __device__ __forceinline__ int ld(const sample* p, const args&) { return *p; }
  static __device__ __forceinline__ sample sat(int v, const args&) { return (sample)clampi(v, 0, 255); }
};

}  // namespace

extern "C" {
int af_launch_yuv_to_rgb(const YuvArgs* a, hipStream_t s) { return yuv_dispatch<Depth8, true>(a, s); }
int af_launch_rgb_to_yuv(const YuvArgs* a, hipStream_t s) { return yuv_dispatch<Depth8, false>(a, s); }
}
