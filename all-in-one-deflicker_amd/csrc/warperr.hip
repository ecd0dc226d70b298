// warperr.hip — the warping error E_warp of Lai et al. (ECCV 2018) over consecutive frame pairs, from the building blocks the
// reference ships in src/models/utils.py: flow_warping (:504-529), detect_occlusion (:532-572), compute_flow_gradients /
// compute_flow_magnitude (:478-502).  Pair t: warped = flow_warping(I_{t+1}, fw_t); occ = detect_occlusion(A = bw_{t+1}, B = fw_t);
// E_t = sum noc * (warped - I_t)^2 / (3 * sum noc).  One fused kernel per pixel: the sample position is computed once and its four
// bilinear corners serve both I_{t+1} and A; B's right and lower neighbours give the motion-boundary mask.  fp32 like the reference
// (no FMA contraction), the gradient terms in fp64 like compute_flow_gradients' np.zeros buffers; fp64 block partials, summed on
// the host in a fixed order (host_util.hip af_warp_error_pair, host_render.hip af_warp_error).
#include <math.h>
#include "af_dev.h"
#include "elem.h"

namespace {

// grid_sample's unnormalize of the CPU kernel (ATen GridSamplerKernel.cpp ComputeLocationBase): align_corners (in + 1) * ((size - 1) / 2),
// otherwise (in + 1) * (size / 2) - 0.5, both in fp32.
__device__ __forceinline__ float unnormalize(float in, int size, int align) {
#pragma clang fp contract(off)
  return align ? (in + 1.f) * ((float)(size - 1) / 2.f) : (in + 1.f) * ((float)size / 2.f) - 0.5f;
}

// Source accessor, a template on the pixel strides: element k of pixel p of pair `pair` of img1 is img1[pair * img_pair_stride + p * IS + k],
// likewise img2 (IS floats per pixel) and the flows B = flow12, A = flow21 (FS floats per pixel).  IS = FS = 16: the pixel record table
// (REC_RGB, REC_FF of frame t; REC_RGB, REC_FB of frame t+1); IS = 3: HWC images; FS = 2: HWC flows.
template <int IS, int FS>
__global__ __launch_bounds__(256) void k_warp_error(WarpErrArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[2][4];
  const int W = a.w, H = a.h, npix = W * H;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int pair = blockIdx.y;
  double sse = 0.0, cnt = 0.0;
  if (r < npix) {
    const size_t ib = (size_t)pair * a.img_pair_stride, fb = (size_t)pair * a.flow_pair_stride;
    const float* i1 = a.img1 + ib;
    const float* i2 = a.img2 + ib;
    const float* fB = a.flow12 + fb;
    const float* fA = a.flow21 + fb;
    const int y = r / W, x = r - y * W;
    const float bx = fB[(size_t)r * FS], by = fB[(size_t)r * FS + 1];
    // flow_warping: vgrid = grid + flo; 2 * v / max(W - 1, 1) - 1 (fp32); then grid_sample's unnormalize
    const float nx = 2.f * ((float)x + bx) / (float)max(W - 1, 1) - 1.f;
    const float ny = 2.f * ((float)y + by) / (float)max(H - 1, 1) - 1.f;
    const float sx = unnormalize(nx, W, a.align_corners), sy = unnormalize(ny, H, a.align_corners);
    const float xw = floorf(sx), yn = floorf(sy);
    const float we = sx - xw, wn = sy - yn;          // ATen compute_interp_params: w = x - x_w, e = 1 - w, n = y - y_n, s = 1 - n
    const float e = 1.f - we, s = 1.f - wn;
    const float c_nw = s * e, c_ne = s * we, c_sw = wn * e, c_se = wn * we;
    // zero padding: a corner outside [0, W-1] x [0, H-1] reads 0 (tested in fp32 before any integer conversion: flows may be huge)
    const bool vx0 = xw >= 0.f && xw <= (float)(W - 1), vx1 = xw >= -1.f && xw <= (float)(W - 2);
    const bool vy0 = yn >= 0.f && yn <= (float)(H - 1), vy1 = yn >= -1.f && yn <= (float)(H - 2);
    const int ix = (vx0 || vx1) ? (int)xw : 0, iy = (vy0 || vy1) ? (int)yn : 0;
    const bool v_nw = vx0 && vy0, v_ne = vx1 && vy0, v_sw = vx0 && vy1, v_se = vx1 && vy1;
    const size_t p_nw = (size_t)iy * W + ix;
    auto tap = [&](const float* b, int stride, int k) {
      const float q_nw = v_nw ? b[p_nw * stride + k] : 0.f;
      const float q_ne = v_ne ? b[(p_nw + 1) * stride + k] : 0.f;
      const float q_sw = v_sw ? b[(p_nw + W) * stride + k] : 0.f;
      const float q_se = v_se ? b[(p_nw + W + 1) * stride + k] : 0.f;
      return ((q_nw * c_nw + q_ne * c_ne) + q_sw * c_sw) + q_se * c_se;
    };
    float wv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) wv[c] = tap(i2, IS, c);
    const float awx = tap(fA, FS, 0), awy = tap(fA, FS, 1);
    // mask1 (fp32): |A_w + B|^2 > 0.01 (|A_w|^2 + |B|^2) + 0.5
    const float s0 = awx + bx, s1 = awy + by;
    const float fb_mag = s0 * s0 + s1 * s1, aw_mag = awx * awx + awy * awy, b_mag = bx * bx + by * by;
    const bool m1 = fb_mag > 0.01f * (aw_mag + b_mag) + 0.5f;
    // mask2: differences of B taken in fp32, stored, squared and summed in fp64 (0 in the last column / row); the bound in fp32
    const double dxu = x + 1 < W ? (double)(bx - fB[(size_t)(r + 1) * FS]) : 0.0;
    const double dyu = x + 1 < W ? (double)(by - fB[(size_t)(r + 1) * FS + 1]) : 0.0;
    const double dxv = y + 1 < H ? (double)(bx - fB[(size_t)(r + W) * FS]) : 0.0;
    const double dyv = y + 1 < H ? (double)(by - fB[(size_t)(r + W) * FS + 1]) : 0.0;
    const double fx_mag = dxu * dxu + dxv * dxv, fy_mag = dyu * dyu + dyv * dyv;
    const bool m2 = (fx_mag + fy_mag) > (double)(0.01f * b_mag + 0.002f);
    const bool noc = !(m1 || m2);
    if (a.noc) a.noc[(size_t)pair * npix + r] = noc ? 1.f : 0.f;
    if (a.warped) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.warped[((size_t)pair * npix + r) * 3 + c] = wv[c];
    }
    if (noc) {
      const double d0 = (double)(wv[0] - i1[(size_t)r * IS]), d1 = (double)(wv[1] - i1[(size_t)r * IS + 1]), d2 = (double)(wv[2] - i1[(size_t)r * IS + 2]);
      sse = (d0 * d0 + d1 * d1) + d2 * d2;
      cnt = 1.0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sse += __shfl_xor(sse, o); cnt += __shfl_xor(cnt, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sse; red[1][threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* p = a.part + ((size_t)pair * gridDim.x + blockIdx.x) * 2;
    p[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    p[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

}  // namespace

extern "C" {
// kind 0: record table (img and flow records of 16 floats), 1: HWC images with record-table flows, 2: HWC images and HWC flows.
// Grid (ceil(h*w / 256), npairs); part receives [npairs][nblk][2] = {sum noc * sum_c diff^2, sum noc}.
int af_launch_warp_error(const WarpErrArgs* a, int kind, int npairs, hipStream_t s) {
  const dim3 grid((unsigned)((a->w * a->h + 255) / 256), (unsigned)npairs);
  if (kind == 0)      hipLaunchKernelGGL((k_warp_error<AF_REC_F, AF_REC_F>), grid, dim3(256), 0, s, *a);
  else if (kind == 1) hipLaunchKernelGGL((k_warp_error<3, AF_REC_F>), grid, dim3(256), 0, s, *a);
  else                hipLaunchKernelGGL((k_warp_error<3, 2>), grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
}
