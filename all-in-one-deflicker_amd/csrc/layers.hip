// layers.hip — forward-only outputs of a trained handle beyond the composited frame: per-layer uv / alpha / colour, the
// mapping-area reduction, atlas textures and texture-edit propagation (src/models/stage_1/evaluate.py:24-200,300-438).
// The MLP work runs through the existing forward chains (host_render.hip); these kernels sit around them.  All fp32 like elem.hip
// (no fast-math), except the bilinear texture sampling, which is fp64 as in the reference's numpy (int64 - float32 -> float64).
#include <math.h>
#include "af_dev.h"
#include "elem.h"


AF_DEV float alpha_of_raw(float t) { float a = 0.5f * (t + 1.f); a = a * 0.99f; return a + 0.001f; }   // evaluate.py:331-335 (== elem.hip alpha_of)

// Layer finish (evaluate.py:302-337 without the blend): raw uv of both mappings, alpha, each layer's colour (t+1)/2.
// out_atlas holds the fg rows, then `row2` rows later the bg rows; uv2s / out_alpha / row2 unused on a single-atlas handle
// (alpha = 1).  Every output may be NULL.  All pointers are those of the rows at hand: a whole lattice frame (af_render_layers) or one
// band of an oh x ow grid (af_render_layers_at; the host adds the band's offset in 64 bits).  alpha_u8: the truncated byte of alpha,
// (uint8)(int)((double)alpha * 255), as k_frame_finish_at makes it of a colour.
__global__ __launch_bounds__(256) void k_layer_finish(const float* uv1s, const float* uv2s, const float* out_atlas, size_t row2,
                                                      const float* out_alpha, int npix, float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2,
                                                      unsigned char* alpha_u8) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= npix) return;
  if (uv1) { uv1[(size_t)r * 2] = uv1s[(size_t)r * 4]; uv1[(size_t)r * 2 + 1] = uv1s[(size_t)r * 4 + 1]; }
  if (uv2) { uv2[(size_t)r * 2] = uv2s[(size_t)r * 4]; uv2[(size_t)r * 2 + 1] = uv2s[(size_t)r * 4 + 1]; }
  if (alpha) alpha[r] = out_alpha ? alpha_of_raw(out_alpha[(size_t)r * 4]) : 1.f;
  if (alpha_u8) alpha_u8[r] = (unsigned char)(int)((double)(out_alpha ? alpha_of_raw(out_alpha[(size_t)r * 4]) : 1.f) * 255.0);
  if (rgb1) {
    const f32x4 t = *(const f32x4*)(out_atlas + (size_t)r * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb1[(size_t)r * 3 + c] = (t[c] + 1.f) * 0.5f;
  }
  if (rgb2) {
    const f32x4 t = *(const f32x4*)(out_atlas + (row2 + r) * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb2[(size_t)r * 3 + c] = (t[c] + 1.f) * 0.5f;
  }
}

// get_mapping_area (evaluate.py:142-190), one frame: predicate and min/max of uv*0.5 + shift, reduced per block.
// fg (which 0): mask_fg > 0.5 and a > 0.95; bg (which 1): -a > -0.5 on every pixel.  a = the RAW alpha-net output.
// part[block] = {min x, min y, max x, max y}; a block without a selected pixel leaves {+inf, +inf, -inf, -inf}.
__global__ __launch_bounds__(256) void k_area_reduce(const float* uv, const float* out_alpha, const float* table, size_t rec0, int npix,
                                                     int which, float4* part) {
  __shared__ float red[4][4];
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  if (r < npix) {
    const float a = out_alpha[(size_t)r * 4];
    const bool sel = which == 0 ? (table[(rec0 + r) * AF_REC_F + REC_FG] > 0.5f && a > 0.95f) : (-a > -0.5f);
    if (sel) {
      const float shift = which == 0 ? 0.5f : -0.5f;
      const float x = uv[(size_t)r * 4] * 0.5f + shift, y = uv[(size_t)r * 4 + 1] * 0.5f + shift;    // x*0.5 is exact: fused or not, the same value
      mnx = x; mny = y; mxx = x; mxy = y;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mnx = fminf(mnx, __shfl_xor(mnx, o)); mny = fminf(mny, __shfl_xor(mny, o));
    mxx = fmaxf(mxx, __shfl_xor(mxx, o)); mxy = fmaxf(mxy, __shfl_xor(mxy, o));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w][0] = mnx; red[w][1] = mny; red[w][2] = mxx; red[w][3] = mxy; }
  __syncthreads();
  if (threadIdx.x == 0)
    part[blockIdx.x] = make_float4(fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0])), fminf(fminf(red[0][1], red[1][1]), fminf(red[2][1], red[3][1])),
                                   fmaxf(fmaxf(red[0][2], red[1][2]), fmaxf(red[2][2], red[3][2])), fmaxf(fmaxf(red[0][3], red[1][3]), fmaxf(red[2][3], red[3][3])));
}

// torch.linspace(s, e, n)[i] in fp32 as torch's CPU kernel computes it: step = (e - s) / (n - 1), then s + step*i below n/2 and
// e - step*(n-1-i) from n/2 on, each one fused multiply-add (checked against torch.linspace in tests/test_atlas_outputs_host.py).
AF_DEV float linspace_f32(float s, float e, int n, int i) {
  if (n == 1) return s;
  const float step = (e - s) / (float)(n - 1);
  return i < n / 2 ? fmaf(step, (float)i, s) : fmaf(-step, (float)(n - 1 - i), e);
}

// get_high_res_texture (evaluate.py:87-104): input rows (x, y) of texture rows [row0, row0 + nrows) of a res x res grid, row = y,
// column = x; rows of the last tile past nrows*res are zero.
__global__ void k_tex_coords(float* coords, int res, int row0, int nrows, float sx, float ex, float sy, float ey, int rows_pad) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows_pad) return;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (r < nrows * res) { const int ty = r / res, tx = r - ty * res; v[0] = linspace_f32(sx, ex, res, tx); v[1] = linspace_f32(sy, ey, res, row0 + ty); }
  *(f32x4*)(coords + (size_t)r * 4) = v;
}

__global__ void k_tex_finish(const float* out_atlas, int rows, float* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const f32x4 t = *(const f32x4*)(out_atlas + (size_t)r * 4);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(size_t)r * 3 + c] = 0.5f * (t[c] + 1.f);
}

// get_colors + bilinear_interpolate_numpy (evaluate.py:24-84) for one layer at one pixel.  px, py: texel coordinates
// (uv*0.5 +- 0.5 - min) * pixel_size in fp32.  Returns false when the pixel is not "relevant" (:67-78; NaN is never relevant).
// The four taps are the numpy gist's, including its clipping of x1 / y1 BEFORE the weights (a coordinate exactly at res-1 gets weight 0).
AF_DEV bool sample_texture(const float* tex, int res, float px, float py, double rgb[3], int tap[4]) {
  const float fx = floorf(px), cx = ceilf(px), fy = floorf(py), cy = ceilf(py);
  if (!(cy >= 0.f && fy >= 0.f && cx >= 0.f && fx >= 0.f && cy < (float)res && fy < (float)res && cx < (float)res && fx < (float)res)) return false;
  const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, res - 1), y1 = min(y0 + 1, res - 1);
  tap[0] = (int)fy; tap[1] = (int)cy; tap[2] = (int)fx; tap[3] = (int)cx;      // floor / ceil rows and columns of the usage masks
  if (!tex) return true;
  const double x = px, y = py;
  const double wa = ((double)x1 - x) * ((double)y1 - y), wb = ((double)x1 - x) * (y - (double)y0);
  const double wc = (x - (double)x0) * ((double)y1 - y), wd = (x - (double)x0) * (y - (double)y0);
  const float* Ia = tex + ((size_t)y0 * res + x0) * 3; const float* Ib = tex + ((size_t)y1 * res + x0) * 3;
  const float* Ic = tex + ((size_t)y0 * res + x1) * 3; const float* Id = tex + ((size_t)y1 * res + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[c] = (((double)Ia[c] * wa + (double)Ib[c] * wb) + (double)Ic[c] * wc) + (double)Id[c] * wd;
  return true;
}

// Texture-edit propagation and texel usage (evaluate.py:373-438), one frame.  Layer L (0 fg, 1 bg) takes part when active[L]
// is set; its texture may be NULL (usage masks only).  edit1 = rgb1*alpha, edit2 = rgb2, edit = the sum of
// rgb1*alpha and rgb2*(1-alpha) over the relevant layers, 0 where no layer is relevant.  Usage masks over ALL frames:
// use_fg = max of alpha over the four floor/ceil texels (atomicMax on the uint bits: alpha >= 0.001 > 0 and the caller zeroes
// the mask, so the unsigned order is the float order), use_bg = 1 on any use.
// The rows are a lattice frame's (af_render_edit) or one band's of an oh x ow grid (af_edit_frame: band-local pointers, textures and usage
// masks resident in the session's own memory; the masks' updates commute, so they do not depend on the banding).  edit_u8: the truncated
// byte of edit, (uint8)(int)((double)edit * 255).
__global__ __launch_bounds__(256) void k_edit(EditArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.npix) return;
  const float al = alpha_of_raw(a.out_alpha[(size_t)r * 4]);
  double acc[3] = {0.0, 0.0, 0.0};
  for (int L = 0; L < 2; ++L) {
    if (!a.active[L]) continue;
    const float* uv = L == 0 ? a.uv1 : a.uv2;
    const float shift = L == 0 ? 0.5f : -0.5f;
    const float px = (uv[(size_t)r * 4] * 0.5f + shift - a.minx[L]) * a.pixel_size[L];
    const float py = (uv[(size_t)r * 4 + 1] * 0.5f + shift - a.miny[L]) * a.pixel_size[L];
    double rgb[3]; int tap[4];
    const bool rel = sample_texture(a.tex[L], a.res, px, py, rgb, tap);
    float* eo = a.edit_layer[L];
    if (rel) {
      const double w = L == 0 ? (double)al : (double)(1.f - al);     // evaluate.py:421-429: (1 - alpha) in fp32, products in fp64
      if (a.tex[L]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += rgb[c] * w;
        if (eo) {
#pragma unroll
          for (int c = 0; c < 3; ++c) eo[(size_t)r * 3 + c] = (float)(L == 0 ? rgb[c] * w : rgb[c]);
        }
      }
      float* use = a.use[L];
      if (use) {
        const int ys[4] = {tap[1], tap[0], tap[0], tap[1]}, xs[4] = {tap[3], tap[2], tap[3], tap[2]};   // (ceil, ceil), (floor, floor), (floor, ceil), (ceil, floor)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float* p = use + (size_t)ys[k] * a.res + xs[k];
          if (L == 0) atomicMax((unsigned int*)p, __float_as_uint(al));
          else *p = 1.f;
        }
      }
    } else if (eo) {
#pragma unroll
      for (int c = 0; c < 3; ++c) eo[(size_t)r * 3 + c] = 0.f;
    }
  }
  if (a.edit) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.edit[(size_t)r * 3 + c] = (float)acc[c];
  }
  if (a.edit_u8) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.edit_u8[(size_t)r * 3 + c] = (unsigned char)(int)((double)(float)acc[c] * 255.0);
  }
}

extern "C" {
int af_launch_layer_finish(const float* uv1s, const float* uv2s, const float* out_atlas, size_t row2, const float* out_alpha, int npix,
                           float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2, unsigned char* alpha_u8, hipStream_t s) {
  hipLaunchKernelGGL(k_layer_finish, dim3((npix + 255) / 256), dim3(256), 0, s, uv1s, uv2s, out_atlas, row2, out_alpha, npix, uv1, uv2, alpha, rgb1, rgb2, alpha_u8);
  return (int)hipGetLastError();
}
int af_launch_area_reduce(const float* uv, const float* out_alpha, const float* table, size_t rec0, int npix, int which, float* part, hipStream_t s) {
  hipLaunchKernelGGL(k_area_reduce, dim3((npix + 255) / 256), dim3(256), 0, s, uv, out_alpha, table, rec0, npix, which, (float4*)part);
  return (int)hipGetLastError();
}
int af_launch_tex_coords(float* coords, int res, int row0, int nrows, float sx, float ex, float sy, float ey, int rows_pad, hipStream_t s) {
  hipLaunchKernelGGL(k_tex_coords, dim3((rows_pad + 255) / 256), dim3(256), 0, s, coords, res, row0, nrows, sx, ex, sy, ey, rows_pad);
  return (int)hipGetLastError();
}
int af_launch_tex_finish(const float* out_atlas, int rows, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_tex_finish, dim3((rows + 255) / 256), dim3(256), 0, s, out_atlas, rows, out);
  return (int)hipGetLastError();
}
int af_launch_edit(const EditArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_edit, dim3((a->npix + 255) / 256), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}
}
