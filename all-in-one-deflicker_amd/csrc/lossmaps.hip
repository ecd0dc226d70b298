// lossmaps.hip — per-pixel loss maps of one whole frame (src/models/stage_1/evaluate.py:338-384 fg/bg, :650-705 single):
// rigidity (loss_utils.py:227-280, return_all), optical flow (:283-296, :360-383), alpha flow (:412-424), rgb error and residual.
// The MLP work runs through the existing forward chains (host_render.hip af_render_loss_maps); these two kernels build the chains' input
// rows and finish the maps.  All fp32 like elem.hip (no fast-math).
#include <math.h>
#include "af_dev.h"
#include "elem.h"


AF_DEV float alpha_map(float t) { float a = 0.5f * (t + 1.f); a = a * 0.99f; return a + 0.001f; }   // evaluate.py:331-335 (== elem.hip alpha_of)

AF_DEV void put_xyt(float* coords, size_t r, float x, float y, float t) { f32x4 v = {x, y, t, 0.f}; *(f32x4*)(coords + r * 4) = v; }

// Input rows of every pixel of one frame, one segment of rows_pad rows per role (pixel p -> row seg*rows_pad + p); pad rows are zero.
// seg_ym / seg_xm / seg_t < 0: that segment is not built.  Centre rows as k_frame_coords_at at the lattice size (t = the Python-float frame time rounded
// to fp32, evaluate.py:313); the neighbour and flow-target rows compute t in fp32 from the integer frame, as the reference's
// int64 jif tensors divided by a Python float do (loss_utils.py:230-233, :373-381).
__global__ __launch_bounds__(256) void k_lossmap_rows(LossMapArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.rows_pad) return;
  const int npix = a.resx * a.resy;
  if (r >= npix) {
    put_xyt(a.coords, (size_t)a.seg_c * a.rows_pad + r, 0.f, 0.f, 0.f);
    if (a.seg_ym >= 0) { put_xyt(a.coords, (size_t)a.seg_ym * a.rows_pad + r, 0.f, 0.f, 0.f); put_xyt(a.coords, (size_t)a.seg_xm * a.rows_pad + r, 0.f, 0.f, 0.f); }
    if (a.seg_t >= 0) put_xyt(a.coords, (size_t)a.seg_t * a.rows_pad + r, 0.f, 0.f, 0.f);
    return;
  }
  const int y = r / a.resx, x = r - y * a.resx;
  const float hm = a.half_main, hf = a.half_frames;
  const float xc = (float)x / hm - 1.f, yc = (float)y / hm - 1.f;
  put_xyt(a.coords, (size_t)a.seg_c * a.rows_pad + r, xc, yc, a.t_centre);
  const float tf = (float)a.frame / hf - 1.f;
  if (a.seg_ym >= 0) {
    put_xyt(a.coords, (size_t)a.seg_ym * a.rows_pad + r, xc, (float)(y - a.d) / hm - 1.f, tf);
    put_xyt(a.coords, (size_t)a.seg_xm * a.rows_pad + r, (float)(x - a.d) / hm - 1.f, yc, tf);
  }
  if (a.seg_t >= 0) {      // forward flow target from the record table (get_corresponding_flow_matches_all: flow of index 0, frame f + 1)
    const float* rec = a.table + (a.rec0 + r) * AF_REC_F;
    put_xyt(a.coords, (size_t)a.seg_t * a.rows_pad + r, ((float)x + rec[REC_FF]) / hm - 1.f, ((float)y + rec[REC_FF + 1]) / hm - 1.f,
            (float)(a.frame + 1) / hf - 1.f);
  }
}

// get_rigidity_loss(..., return_all=True) of one pixel (loss_utils.py:239-275), in the reference's operation order.
AF_DEV float rigidity_map(float u, float v, float u_ym, float v_ym, float u_xm, float v_xm, float L, float s, float d) {
  const float j00 = ((u - u_xm) * L / 2.f) / s / d, j01 = ((u - u_ym) * L / 2.f) / s / d;
  const float j10 = ((v - v_xm) * L / 2.f) / s / d, j11 = ((v - v_ym) * L / 2.f) / s / d;
  const float g00 = j00 * j00 + j10 * j10, g01 = j00 * j01 + j10 * j11, g11 = j01 * j01 + j11 * j11;   // JtJ (symmetric: g10 = g01)
  const float A = g00 + 0.001f, D = g11 + 0.001f, B = g01;
  const float det = A * D - B * B;
  const float i00 = D / det, i01 = -B / det, i11 = A / det;
  // (M ** 2).sum(1).sum(1): column sums first
  const float ng = sqrtf((g00 * g00 + g01 * g01) + (g01 * g01 + g11 * g11));
  const float ni = sqrtf((i00 * i00 + i01 * i01) + (i01 * i01 + i11 * i11));
  return ng + ni;
}

// Finish of one frame's maps.  Chain outputs are [rows][4]: the mapping nets' segment s at row s*rows_pad of out_m1 / out_m2; the
// alpha net's centre rows, then rows_pad rows later its flow-target rows; the atlas's fg rows, then rows_pad rows later the bg rows.
__global__ __launch_bounds__(256) void k_lossmap_finish(LossMapArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int npix = a.resx * a.resy;
  if (r >= npix) return;
  const size_t P = (size_t)a.rows_pad;
  const float* rec = a.table + (a.rec0 + r) * AF_REC_F;
  const bool valid = rec[REC_MF] > 0.f;                       // forward_flows_for_loss_mask > 0 (loss_utils.py:382)
  const float al = a.out_alpha ? alpha_map(a.out_alpha[(size_t)r * 4]) : 1.f;   // single path: alpha = 1
  const float fscale_num = a.L, fscale_den = 2.f * a.uv_scale;
#pragma unroll
  for (int net = 0; net < 2; ++net) {
    const float* om = net ? a.out_m2 : a.out_m1;
    float* rig = net ? a.rigidity2 : a.rigidity1;
    float* flo = net ? a.flow2 : a.flow1;
    if (!rig && !flo) continue;
    const f32x4 uvc = *(const f32x4*)(om + ((size_t)a.seg_c * P + r) * 4);
    if (rig) {
      const f32x4 pym = *(const f32x4*)(om + ((size_t)a.seg_ym * P + r) * 4);
      const f32x4 pxm = *(const f32x4*)(om + ((size_t)a.seg_xm * P + r) * 4);
      rig[r] = rigidity_map(uvc[0], uvc[1], pym[0], pym[1], pxm[0], pxm[1], a.L, a.uv_scale, (float)a.d);
    }
    if (flo) {
      float l = 0.f;          // the last frame has no forward match (evaluate.py:374-376, :692): 0
      if (a.flow_map) {
        const f32x4 m = *(const f32x4*)(om + ((size_t)a.seg_t * P + r) * 4);
        const float eu = m[0] - uvc[0], ev = m[1] - uvc[1];
        float e = sqrtf(eu * eu + ev * ev);
        if (!valid) e = 0.f;
        e = e * (net ? 1.f - al : al);                         // :292 errors * alpha (fg) / (1 - alpha) (bg)
        l = e * fscale_num / fscale_den;                        // :294 errors * resx / (2 * uv_mapping_scale)
      }
      flo[r] = l;
    }
  }
  if (a.flow_alpha) {       // loss_utils.py:412-424: |alpha - alpha(target)|, 0 where the mask is 0 (also on the last frame)
    const float at = alpha_map(a.out_alpha[(P + r) * 4]);
    a.flow_alpha[r] = valid ? fabsf(al - at) : 0.f;
  }
  if (a.rgb_err || a.residual) {      // the reconstruction of af_render_frame (k_frame_finish_at)
    const f32x4 t1 = *(const f32x4*)(a.out_atlas + (size_t)r * 4);
    float res[3];
    if (a.out_alpha) {
      const f32x4 t2 = *(const f32x4*)(a.out_atlas + (P + r) * 4);
#pragma unroll
      for (int c = 0; c < 3; ++c) res[c] = rec[REC_RGB + c] - (((t1[c] + 1.f) * 0.5f) * al + ((t2[c] + 1.f) * 0.5f) * (1.f - al));
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) res[c] = rec[REC_RGB + c] - (t1[c] + 1.f) * 0.5f;
    }
    if (a.residual) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.residual[(size_t)r * 3 + c] = res[c];
    }
    if (a.rgb_err) {          // evaluate.py:379-381: (frame - rgb).norm(dim=1) ** 2
      const float n = sqrtf((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]);
      a.rgb_err[r] = n * n;
    }
  }
}

extern "C" {
int af_launch_lossmap_rows(const LossMapArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_lossmap_rows, dim3((a->rows_pad + 255) / 256), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
int af_launch_lossmap_finish(const LossMapArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_lossmap_finish, dim3((a->resx * a->resy + 255) / 256), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
}
