// maskprop.hip — propagation of fg masks along the flows, the device side of masks.py.
//   k_mask_step: one step from a source frame s to a neighbouring target frame t.  Target pixel (x, y) looks up q = (x, y) + f_ts[y, x] in
//     the source.  q inside the frame (0 <= qx <= w - 1 && 0 <= qy <= h - 1, written so that a NaN is not inside) and the round trip
//     f_ts[y, x] + bil(f_st)(q) shorter than thresh (the squared norm against thresh^2, one fp32 from the host): m_t = bil(m_s)(q),
//     c_t = bil(c_s)(q).  Otherwise (disoccluded, out of frame, NaN): m_t = m_s[y, x], c_t = 0 — the value is held and carries no
//     confidence.  bil: x0 = (int)qx, x1 = min(x0 + 1, w - 1), ax = qx - x0 (y alike); top = v00 (1 - ax) + v01 ax, bot alike,
//     bil = top (1 - ay) + bot ay.
//   k_mask_blend: frame t strictly between keys a < t < b from the forward result (m_f, c_f) and the backward result (m_b, c_b):
//     wf = (b - t) c_f, wb = (t - a) c_b, s = wf + wb, out = s > 0 ? (wf m_f + wb m_b) / s : ((b - t) m_f + (t - a) m_b) / (b - a),
//     clamped to [0, 1] by comparisons (a NaN stays one).
// Every product, sum and quotient is one correctly rounded fp32 operation in the order written (contraction off: no fused multiply-add),
// so the host may demand equality with a numpy restatement.  One thread per pixel; no LDS, no atomics; 64-bit element offsets (h, w up
// to 16384 makes a flow 2 GiB).
#include "af_dev.h"
#include "elem.h"

#pragma clang fp contract(off)

namespace {

struct Tap {      // the four source pixels of a bilinear look-up and its two weights
  long long o00, o01, o10, o11;
  float ax, ay;
};

__device__ __forceinline__ float bil(const float* v, const Tap& t, int stride, int c) {
  const float bx = 1.f - t.ax, by = 1.f - t.ay;
  const float top = v[t.o00 * stride + c] * bx + v[t.o01 * stride + c] * t.ax;
  const float bot = v[t.o10 * stride + c] * bx + v[t.o11 * stride + c] * t.ax;
  return top * by + bot * t.ay;
}

__global__ __launch_bounds__(256) void k_mask_step(MaskStepArgs a) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.w || y >= a.h) return;
  const long long p = (long long)y * a.w + x;
  const float fx = a.f_ts[p * 2], fy = a.f_ts[p * 2 + 1];
  const float qx = (float)x + fx, qy = (float)y + fy;
  float m = a.m_s[p], c = 0.f;
  if (qx >= 0.f && qx <= (float)(a.w - 1) && qy >= 0.f && qy <= (float)(a.h - 1)) {      // false for a NaN
    const int x0 = (int)qx, y0 = (int)qy;
    const int x1 = x0 + 1 < a.w ? x0 + 1 : a.w - 1, y1 = y0 + 1 < a.h ? y0 + 1 : a.h - 1;
    Tap t;
    t.o00 = (long long)y0 * a.w + x0; t.o01 = (long long)y0 * a.w + x1;
    t.o10 = (long long)y1 * a.w + x0; t.o11 = (long long)y1 * a.w + x1;
    t.ax = qx - (float)x0; t.ay = qy - (float)y0;
    const float dx = fx + bil(a.f_st, t, 2, 0), dy = fy + bil(a.f_st, t, 2, 1);
    if (dx * dx + dy * dy < a.thresh2) {
      m = bil(a.m_s, t, 1, 0);
      c = bil(a.c_s, t, 1, 0);
    }
  }
  a.m_t[p] = m;
  a.c_t[p] = c;
}

__global__ __launch_bounds__(256) void k_mask_blend(MaskBlendArgs a) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.w || y >= a.h) return;
  const long long p = (long long)y * a.w + x;
  const float mf = a.m_f[p], mb = a.m_b[p];
  const float wf = a.to_b * a.c_f[p], wb = a.from_a * a.c_b[p];
  const float s = wf + wb;
  float v = s > 0.f ? (wf * mf + wb * mb) / s : (a.to_b * mf + a.from_a * mb) / a.span;
  v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
  a.out[p] = v;
}

dim3 pixel_grid(int h, int w) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)); }

}  // namespace

extern "C" {
// Grid (ceil(w / 64), ceil(h / 4)) of 64 x 4 threads: h, w <= 16384 keeps both far inside the grid limits.
int af_launch_mask_step(const MaskStepArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_mask_step, pixel_grid(a->h, a->w), dim3(64, 4), 0, s, *a);
  return (int)hipGetLastError();
}
int af_launch_mask_blend(const MaskBlendArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_mask_blend, pixel_grid(a->h, a->w), dim3(64, 4), 0, s, *a);
  return (int)hipGetLastError();
}
}
