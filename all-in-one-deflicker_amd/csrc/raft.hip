// raft.hip — the optical-flow precompute (reference: src/preprocess_optical_flow.py -> src/models/stage_1/raft_wrapper.py ->
// src/models/stage_1/core/{raft,extractor,update,corr}.py): a forward-only RAFT ("basic", small=False) in fp32, iters update steps,
// test mode, at the padded size.
//
// Activations are NHWC fp32.  Every convolution is k_rconv: the implicit-GEMM core of conv_gemm.h (shared with filter.hip's k_conv;
// v_mfma_f32_32x32x2_f32 with exact fp32 products, chunks of 16 summed with Kahan's compensation) instantiated with a stack of B images
// along M (pair-directions of one batch run in one launch; a pixel's sum does not depend on its place in a tile, so batching changes no
// bit) and without reflection padding.  k_rconv's epilogue is what RAFT adds: an output scale, sigmoid, the tanh | ReLU split of the
// context encoder, and the two fused GRU epilogues (z | r in one launch with r * h written into the slice the q-conv reads;
// h = (1 - z) h + z q).  Kernels are rectangular (kh, kw).  Concatenations are free: producers write channel slices of one buffer.  The
// all-pairs correlation is the same kernel as a 1x1 convolution whose weights are the second frame's transposed features.
//
// Precision mode AF_RAFT_FP16 (af_raft_set_precision; what the reference runs on a GPU: both encoders and the update block under fp16
// autocast): every convolution of fnet, cnet and the update block runs as k_rconv_h on conv_tile_h (conv_gemm_h.h), the norms round at
// their store.  The buffers stay NHWC fp32 and hold fp16-representable values: every producer rounds once where autocast would hold an
// fp16 tensor.  The correlation volume, pooling, lookup, coords1 += delta, flow = coords1 - coords0 and the upsampling stay fp32.
#include <math.h>
#include <string.h>

#include "conv_gemm_h.h"

namespace {

constexpr int HD = 128;                   // hidden and context channels
constexpr int HXC = 384;                  // cat(h, inp, motion)
constexpr int CORRC = 324;                // 4 levels x 81 taps

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 3, ACT_SIGMOID = 4, ACT_TANH_RELU = 5 };
enum { EPI_PLAIN = 0, EPI_GRU_ZR = 1, EPI_GRU_Q = 2 };

struct RConvArgs {
  ConvGeom g;
  int act, epi;
  float oscale;                           // v = (sum + bias) * oscale before the activation
  const float* h; long long ldh;          // GRU epilogues: the hidden state (M, 128) at pixel stride ldh
  float* z;                               // GRU epilogues: the update gate (M, 128), written by ZR and read by Q
  float* y; long long ldy;                // output at pixel stride ldy
  float* y2; long long ldy2;              // optional second copy
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// conv_tile with the batch index, without reflection padding; the epilogue: scale, GRU gates or activation, store
// (the arguments are captured by copy: captured by reference, k_rconv<128> spills into 89 AGPRs instead of 72)
template <int BN>
__global__ __launch_bounds__(256) void k_rconv(RConvArgs a) {
  conv_tile<BN, true, false>(a.g, [=](int m, int co, float v) {
#pragma clang fp contract(off)
    v = v * a.oscale;
    if (a.epi == EPI_GRU_ZR) {          // channels [0, 128): z; [128, 256): r, stored as r * h
      v = sigmoidf_(v);
      if (co < HD) a.z[(size_t)m * HD + co] = v;
      else a.y[(size_t)m * a.ldy + (co - HD)] = v * a.h[(size_t)m * a.ldh + (co - HD)];
      return;
    }
    if (a.epi == EPI_GRU_Q) {           // h = (1 - z) h + z tanh(q); y may alias h (each element is read and written by this lane only)
      const float q = tanhf(v), zz = a.z[(size_t)m * HD + co], hh = a.h[(size_t)m * a.ldh + co];
      a.y[(size_t)m * a.ldy + co] = (1.f - zz) * hh + zz * q;
      return;
    }
    if (a.act == ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (a.act == ACT_TANH) v = tanhf(v);
    else if (a.act == ACT_SIGMOID) v = sigmoidf_(v);
    else if (a.act == ACT_TANH_RELU) v = co < HD ? tanhf(v) : (v > 0.f ? v : 0.f);
    a.y[(size_t)m * a.ldy + co] = v;
    if (a.y2) a.y2[(size_t)m * a.ldy2 + co] = v;
  });
}

// The fp16 mode's convolution: conv_tile_h hands y = fp16(sum + bias16); the scale and the activation are applied in fp32 and the
// result is rounded to fp16 once more.  GRU: z, r = fp16(sigmoid(y)), r * h rounded once, q = fp16(tanh(y)), h = fp16((1 - z) h + z q).
template <int BN>
__global__ __launch_bounds__(256) void k_rconv_h(RConvArgs a) {
  conv_tile_h<BN, true, false>(a.g, [=](int m, int co, float v) {
#pragma clang fp contract(off)
    v = v * a.oscale;
    if (a.epi == EPI_GRU_ZR) {
      v = round_h(sigmoidf_(v));
      if (co < HD) a.z[(size_t)m * HD + co] = v;
      else a.y[(size_t)m * a.ldy + (co - HD)] = round_h(v * a.h[(size_t)m * a.ldh + (co - HD)]);
      return;
    }
    if (a.epi == EPI_GRU_Q) {
      const float q = round_h(tanhf(v)), zz = a.z[(size_t)m * HD + co], hh = a.h[(size_t)m * a.ldh + co];
      a.y[(size_t)m * a.ldy + co] = round_h((1.f - zz) * hh + zz * q);
      return;
    }
    if (a.act == ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (a.act == ACT_TANH) v = tanhf(v);
    else if (a.act == ACT_SIGMOID) v = sigmoidf_(v);
    else if (a.act == ACT_TANH_RELU) v = co < HD ? tanhf(v) : (v > 0.f ? v : 0.f);
    v = round_h(v);
    a.y[(size_t)m * a.ldy + co] = v;
    if (a.y2) a.y2[(size_t)m * a.ldy2 + co] = v;
  });
}

// 2 (img / 255) - 1 and InputPadder mode 'sintel' (replicate; `top` rows above, `left` columns on the left): (h, w, 3) -> (Hp, Wp, 3)
__global__ void k_prep(const float* src, int h, int w, float* dst, int Hp, int Wp, int top, int left) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Hp * Wp * 3) return;
  const int c = (int)(i % 3); const long long p = i / 3;
  const int y = (int)(p / Wp), x = (int)(p - (long long)y * Wp);
  const int sy = min(max(y - top, 0), h - 1), sx = min(max(x - left, 0), w - 1);
  dst[i] = 2.f * (src[((size_t)sy * w + sx) * 3 + c] / 255.f) - 1.f;
}

// InstanceNorm statistics, deterministic: chunk `blockIdx.x` of IN_CHUNK pixels -> part[chunk][C][2] = (sum, sum of squares) in fp64.
constexpr int IN_CHUNK = 1024;
__global__ __launch_bounds__(256) void k_in_partial(const float* x, long long P, int C, double* part) {
  __shared__ double s0[256], s1[256];
  const int lanes = 256 / C;                  // C in {64, 96, 128}: 4, 2, 2 pixel lanes
  const int c = threadIdx.x % C, pl = threadIdx.x / C;
  const long long p0 = (long long)blockIdx.x * IN_CHUNK, p1 = p0 + IN_CHUNK < P ? p0 + IN_CHUNK : P;
  double a = 0.0, b = 0.0;
  if (pl < lanes)
    for (long long p = p0 + pl; p < p1; p += lanes) { const double v = (double)x[p * C + c]; a += v; b += v * v; }
  s0[threadIdx.x] = a; s1[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x < C) {
    for (int l = 1; l < lanes; ++l) { a += s0[threadIdx.x + l * C]; b += s1[threadIdx.x + l * C]; }
    part[((size_t)blockIdx.x * C + c) * 2] = a; part[((size_t)blockIdx.x * C + c) * 2 + 1] = b;
  }
}

// ... -> y = x * alpha[c] + beta[c] with alpha = 1 / sqrt(var + eps) (biased variance), beta = -mean * alpha
__global__ void k_in_final(const double* part, int nchunk, long long P, int C, float* alpha, float* beta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nchunk; ++k) { a += part[((size_t)k * C + c) * 2]; b += part[((size_t)k * C + c) * 2 + 1]; }
  const double mean = a / (double)P, var = fmax(b / (double)P - mean * mean, 0.0), rs = 1.0 / sqrt(var + 1e-5);
  alpha[c] = (float)rs; beta[c] = (float)(-mean * rs);
}

// The normalise pass of both norms: v = x * alpha[c] + beta[c]; relu: v = max(v, 0); res: v = max(res + v, 0) (the block's output);
// half: the fp32 result is rounded to fp16 once at the store (the fp16 mode).
__global__ void k_affine(const float* x, const float* alpha, const float* beta, int relu, const float* res, float* y, long long P, int C, int half) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * C) return;
  const int c = (int)(i % C);
  float v = x[i] * alpha[c] + beta[c];
  if (relu) v = v > 0.f ? v : 0.f;
  if (res) { v = res[i] + v; v = v > 0.f ? v : 0.f; }
  y[i] = half ? round_h(v) : v;
}

// fmap (P, C) -> wt [C][Npad] (columns beyond P stay zero): the correlation's "weights"
__global__ void k_transpose(const float* f, int P, int C, float* wt, int Npad) {
  __shared__ float t[32][33];
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 256 threads: 8 rows per pass
  for (int r = ty; r < 32; r += 8) t[r][tx] = (p0 + r < P) ? f[(size_t)(p0 + r) * C + c0 + tx] : 0.f;
  __syncthreads();
  for (int r = ty; r < 32; r += 8) if (p0 + tx < P) wt[(size_t)(c0 + r) * Npad + p0 + tx] = t[tx][r];
}

// F.avg_pool2d(2, 2) over the second image's axes: src (rows, hs, ws) -> dst (rows, hs / 2, ws / 2)
__global__ void k_pool(const float* src, long long rows, int hs, int ws, float* dst) {
#pragma clang fp contract(off)
  const int hd = hs / 2, wd = ws / 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * hd * wd) return;
  const long long r = i / (hd * wd); const int q = (int)(i - r * hd * wd), y = q / wd, x = q - y * wd;
  const float* b = src + (size_t)r * hs * ws + (size_t)(2 * y) * ws + 2 * x;
  dst[i] = (((b[0] + b[1]) + b[ws]) + b[ws + 1]) * 0.25f;
}

struct Pyr { const float* lvl[4]; int h[4], w[4]; long long bstride[4]; };     // level l of batch element e at lvl[l] + e * bstride[l]

// CorrBlock.__call__: out (B * P, 324); channel 81 l + 9 a + b = level l sampled bilinearly (align_corners, zeros outside) at
// (x / 2^l + a - 4, y / 2^l + b - 4), through bilinear_sampler's normalise and grid_sample's unnormalise in fp32.
__global__ void k_lookup(Pyr py, const float* coords, int B, int P, float* out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * P * CORRC) return;
  const int ch = (int)(i % CORRC); const long long bp = i / CORRC;
  const int e = (int)(bp / P), p = (int)(bp - (long long)e * P);
  const int l = ch / 81, t = ch - 81 * l, ta = t / 9, tb = t - 9 * ta;
  const int H = py.h[l], W = py.w[l];
  const float s = 1.f / (float)(1 << l);
  const float px = coords[bp * 2] * s + (float)(ta - 4), pyy = coords[bp * 2 + 1] * s + (float)(tb - 4);
  const float gx = 2.f * px / (float)(W - 1) - 1.f, gy = 2.f * pyy / (float)(H - 1) - 1.f;
  const float ix = (gx + 1.f) * ((float)(W - 1) / 2.f), iy = (gy + 1.f) * ((float)(H - 1) / 2.f);      // ATen's CPU kernel: (g + 1) * ((size - 1) / 2)
  float v = 0.f;
  if (ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H) {       // else all four taps are outside (NaN lands here too)
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wx0 = 1.f - wx1, wy1 = iy - fy, wy0 = 1.f - wy1;
    const float* b = py.lvl[l] + (size_t)e * py.bstride[l] + (size_t)p * H * W;
    const bool xa = x0 >= 0, xb = x0 + 1 < W, ya = y0 >= 0, yb = y0 + 1 < H;
    const float nw = (xa && ya) ? b[(size_t)y0 * W + x0] : 0.f, ne = (xb && ya) ? b[(size_t)y0 * W + x0 + 1] : 0.f;
    const float sw = (xa && yb) ? b[(size_t)(y0 + 1) * W + x0] : 0.f, se = (xb && yb) ? b[(size_t)(y0 + 1) * W + x0 + 1] : 0.f;
    v = ((nw * (wx0 * wy0) + ne * (wx1 * wy0)) + sw * (wx0 * wy1)) + se * (wx1 * wy1);
  }
  out[i] = v;
}

// coords0 of one image: (x, y) per 1/8-grid position
__global__ void k_coords0(float* c, int B, int h, int w) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * h * w) return;
  const int p = (int)(i % (h * w));
  c[i * 2] = (float)(p % w); c[i * 2 + 1] = (float)(p / w);
}

// flow = coords1 - coords0 into the 2-channel flow buffer and the last two channels of both GRU inputs
__global__ void k_flow(const float* c1, const float* c0, long long n2, float* flow, float* hx, float* rhx) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n2) return;
  const float v = c1[i] - c0[i];
  const long long m = i >> 1; const int k = (int)(i & 1);
  flow[i] = v;
  if (hx) { hx[m * HXC + (HXC - 2) + k] = v; rhx[m * HXC + (HXC - 2) + k] = v; }
}

__global__ void k_axpy1(float* c1, const float* d, long long n) {      // coords1 += delta
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) c1[i] = c1[i] + d[i];
}

// strided channel-slice copy: dst[m * ldd + c] = src[m * lds + c], c < C
__global__ void k_slice(const float* src, long long lds, float* dst, long long ldd, long long M, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * C) return;
  const long long m = i / C; const int c = (int)(i - m * C);
  dst[m * ldd + c] = src[m * lds + c];
}

// RAFT.upsample_flow: softmax over the 9 taps of mask channel 64 k + 8 i + j, 8 * flow unfolded 3x3 (zero padding): (B, 8h, 8w, 2)
__global__ void k_upsample(const float* flow, const float* mask, int B, int h, int w, float* up) {
#pragma clang fp contract(off)
  const int Hp = 8 * h, Wp = 8 * w;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * Hp * Wp) return;
  const int e = (int)(i / ((long long)Hp * Wp)); const int q = (int)(i - (long long)e * Hp * Wp);
  const int Y = q / Wp, X = q - Y * Wp, y8 = Y >> 3, ii = Y & 7, x8 = X >> 3, jj = X & 7;
  const float* mk = mask + ((size_t)e * h * w + (size_t)y8 * w + x8) * 576 + ii * 8 + jj;
  float mv[9], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) { mv[k] = mk[64 * k]; mx = fmaxf(mx, mv[k]); }
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) { mv[k] = expf(mv[k] - mx); den += mv[k]; }
  float ux = 0.f, uy = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = y8 + k / 3 - 1, xx = x8 + k % 3 - 1;
    float fx = 0.f, fy = 0.f;
    if (yy >= 0 && yy < h && xx >= 0 && xx < w) { const float* f = flow + ((size_t)e * h * w + (size_t)yy * w + xx) * 2; fx = 8.f * f[0]; fy = 8.f * f[1]; }
    const float m = mv[k] / den;
    ux += m * fx; uy += m * fy;
  }
  up[i * 2] = ux; up[i * 2 + 1] = uy;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

struct BNorm { int c = 0; float *alpha = nullptr, *beta = nullptr; };

struct Epi { int act = ACT_NONE, epi = EPI_PLAIN; float oscale = 1.f; const float* h = nullptr; long long ldh = 0; float* z = nullptr; float* y2 = nullptr; long long ldy2 = 0; };

hipError_t launch_rconv(const ConvLayer& L, const float* x, long long ldx, int B, int H, int W, float* y, long long ldy, const Epi& ep, hipStream_t s,
                        int prec = AF_RAFT_FP32) {
  if (prec == AF_RAFT_FP16) {
    if (!L.wt16) return hipErrorInvalidValue;       // a layer without an fp16 image: never the fp32 kernel in its place
    const RConvArgs a{conv_geom_h(L, x, ldx, B, H, W), ep.act, ep.epi, ep.oscale, ep.h, ep.ldh, ep.z, y, ldy, ep.y2, ep.ldy2};
    return launch_conv_family(k_rconv_h<32>, k_rconv_h<64>, k_rconv_h<128>, a, s);
  }
  const RConvArgs a{conv_geom(L, x, ldx, B, H, W), ep.act, ep.epi, ep.oscale, ep.h, ep.ldh, ep.z, y, ldy, ep.y2, ep.ldy2};
  return launch_conv_family(k_rconv<32>, k_rconv<64>, k_rconv<128>, a, s);
}

// The reference's state_dict order (num_batches_tracked excluded).  An encoder: [norm1] conv1, 6 blocks (conv1, conv2, [norm1, norm2,
// norm3 when strided], [downsample.0, downsample.1 = norm3 again when strided]), conv2.  Bracketed BatchNorm entries (weight, bias,
// running_mean, running_var) exist in cnet only.
const int kBlockC[6] = {64, 64, 96, 96, 128, 128};
const int kBlockS[6] = {1, 1, 2, 1, 2, 1};

struct Encoder { ConvLayer conv1, c1[6], c2[6], down[6], conv2; BNorm n0, n1[6], n2[6], n3[6]; };
struct Update { ConvLayer convc1, convc2, convf1, convf2, conv, zr[2], q[2], fh1, fh2, mk0, mk2; };

struct Cursor {
  const float* p; size_t left; bool ok = true;
  const float* take(size_t n) { if (n > left) { ok = false; return nullptr; } const float* r = p; if (p) p += n; left -= n; return r; }
};

// Walks the flat parameter vector.  With cur.p == nullptr it only counts (left starts at SIZE_MAX).
hipError_t walk_conv(Cursor& cur, ConvLayer* L, int cout, int cin, int kh, int kw, int stride) {
  const float* w = cur.take((size_t)cout * cin * kh * kw); const float* b = cur.take(cout);
  if (!cur.p || !cur.ok || !L) return hipSuccess;
  const hipError_t e = upload_layer(*L, cin, cin, kh, kw, stride, 0, {w}, {b}, cout);
  return e != hipSuccess ? e : upload_layer_h(*L, cin, {w}, {b}, cout);       // both images stay resident
}

hipError_t walk_bn(Cursor& cur, BNorm* N, int c) {
  const float *w = cur.take(c), *b = cur.take(c), *rm = cur.take(c), *rv = cur.take(c);
  if (!cur.p || !cur.ok || !N) return hipSuccess;
  // eval BatchNorm folded into y = x * alpha + beta (ATen's CPU kernel forms the same two terms): alpha = w / sqrt(var + eps), beta = b - mean * alpha
  std::vector<float> al(c), be(c);
  for (int i = 0; i < c; ++i) { const double a = (double)w[i] / sqrt((double)rv[i] + 1e-5); al[i] = (float)a; be[i] = (float)((double)b[i] - (double)rm[i] * a); }
  N->c = c;
  (void)hipFree(N->alpha); (void)hipFree(N->beta); N->alpha = N->beta = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&N->alpha, c * 4)) != hipSuccess || (e = hipMalloc(&N->beta, c * 4)) != hipSuccess) return e;
  if ((e = hipMemcpy(N->alpha, al.data(), c * 4, hipMemcpyHostToDevice)) != hipSuccess) return e;
  return hipMemcpy(N->beta, be.data(), c * 4, hipMemcpyHostToDevice);
}

#define WCHK(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
hipError_t walk_encoder(Cursor& cur, Encoder* E, bool bn, int outc) {
  hipError_t e;
  if (bn) WCHK(walk_bn(cur, E ? &E->n0 : nullptr, 64));
  WCHK(walk_conv(cur, E ? &E->conv1 : nullptr, 64, 3, 7, 7, 2));
  int cin = 64;
  for (int i = 0; i < 6; ++i) {
    const int c = kBlockC[i], s = kBlockS[i];
    WCHK(walk_conv(cur, E ? &E->c1[i] : nullptr, c, cin, 3, 3, s));
    WCHK(walk_conv(cur, E ? &E->c2[i] : nullptr, c, c, 3, 3, 1));
    if (bn) { WCHK(walk_bn(cur, E ? &E->n1[i] : nullptr, c)); WCHK(walk_bn(cur, E ? &E->n2[i] : nullptr, c)); if (s != 1) WCHK(walk_bn(cur, E ? &E->n3[i] : nullptr, c)); }
    if (s != 1) { WCHK(walk_conv(cur, E ? &E->down[i] : nullptr, c, cin, 1, 1, s)); if (bn) WCHK(walk_bn(cur, nullptr, c)); }
    cin = c;
  }
  return walk_conv(cur, E ? &E->conv2 : nullptr, outc, 128, 1, 1, 1);
}

hipError_t walk_update(Cursor& cur, Update* U) {
  hipError_t e;
  WCHK(walk_conv(cur, U ? &U->convc1 : nullptr, 256, CORRC, 1, 1, 1));
  WCHK(walk_conv(cur, U ? &U->convc2 : nullptr, 192, 256, 3, 3, 1));
  WCHK(walk_conv(cur, U ? &U->convf1 : nullptr, 128, 2, 7, 7, 1));
  WCHK(walk_conv(cur, U ? &U->convf2 : nullptr, 64, 128, 3, 3, 1));
  WCHK(walk_conv(cur, U ? &U->conv : nullptr, 126, 256, 3, 3, 1));
  for (int g = 0; g < 2; ++g) {       // convz, convr, convq of the 1x5 pass, then of the 5x1 pass; z and r become one layer of 256 outputs
    const int kh = g == 0 ? 1 : 5, kw = g == 0 ? 5 : 1;
    const size_t nw = (size_t)HD * HXC * 5;
    const float *wz = cur.take(nw), *bz = cur.take(HD), *wr = cur.take(nw), *br = cur.take(HD), *wq = cur.take(nw), *bq = cur.take(HD);
    if (cur.p && cur.ok && U) {
      WCHK(upload_layer(U->zr[g], HXC, HXC, kh, kw, 1, 0, {wz, wr}, {bz, br}, HD));
      WCHK(upload_layer_h(U->zr[g], HXC, {wz, wr}, {bz, br}, HD));
      WCHK(upload_layer(U->q[g], HXC, HXC, kh, kw, 1, 0, {wq}, {bq}, HD));
      WCHK(upload_layer_h(U->q[g], HXC, {wq}, {bq}, HD));
    }
  }
  WCHK(walk_conv(cur, U ? &U->fh1 : nullptr, 256, HD, 3, 3, 1));
  WCHK(walk_conv(cur, U ? &U->fh2 : nullptr, 2, 256, 3, 3, 1));
  WCHK(walk_conv(cur, U ? &U->mk0 : nullptr, 256, HD, 3, 3, 1));
  return walk_conv(cur, U ? &U->mk2 : nullptr, 576, 256, 1, 1, 1);
}
#undef WCHK

size_t raft_param_count() {
  Cursor c{nullptr, (size_t)-1};
  (void)walk_encoder(c, nullptr, false, 256); (void)walk_encoder(c, nullptr, true, 256); (void)walk_update(c, nullptr);
  return (size_t)-1 - c.left;
}

void free_bn(BNorm& N) { (void)hipFree(N.alpha); (void)hipFree(N.beta); N.alpha = N.beta = nullptr; }

}  // namespace

struct af_raft : DevPool {
  int device = 0, h = 0, w = 0, Hp = 0, Wp = 0, top = 0, left = 0, cap = 0, slots = 0;
  int h8 = 0, w8 = 0, P = 0, Npad = 0;
  hipStream_t stream = nullptr;
  Encoder enc[2]; Update up;
  bool loaded = false;
  int prec = AF_RAFT_FP32;
  std::vector<char> slot_valid;
  int last_a = -1, last_b = -1, last_iters = 0;     // batch element 0 of the last flow / step call
  float *img_in = nullptr, *img = nullptr, *sx = nullptr, *sa = nullptr, *sb = nullptr, *sd = nullptr, *in_alpha = nullptr, *in_beta = nullptr;
  double* in_part = nullptr;
  float *fmap = nullptr, *fmapT = nullptr, *ctx = nullptr;              // per slot: (P, 256), [256][Npad], (P, 256) = tanh | relu
  float *vol[4] = {nullptr, nullptr, nullptr, nullptr};                 // per batch element: (P, h_l, w_l)
  int lh[4], lw[4];
  float *hx = nullptr, *rhx = nullptr, *corr = nullptr, *c1 = nullptr, *corflo = nullptr, *f1 = nullptr, *z = nullptr, *fh = nullptr, *delta = nullptr;
  float *coords0 = nullptr, *coords1 = nullptr, *flow = nullptr, *mask = nullptr, *upf = nullptr;

  ~af_raft() {
    for (auto& E : enc) {
      free_layer(E.conv1); free_layer(E.conv2); free_bn(E.n0);
      for (int i = 0; i < 6; ++i) { free_layer(E.c1[i]); free_layer(E.c2[i]); free_layer(E.down[i]); free_bn(E.n1[i]); free_bn(E.n2[i]); free_bn(E.n3[i]); }
    }
    for (ConvLayer* L : {&up.convc1, &up.convc2, &up.convf1, &up.convf2, &up.conv, &up.zr[0], &up.zr[1], &up.q[0], &up.q[1], &up.fh1, &up.fh2, &up.mk0, &up.mk2}) free_layer(*L);
    (void)hipFree(in_part);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

#define RCHK(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)

// One norm of an encoder on x (P, C) in place or into y: instance statistics (fnet) or the folded eval BatchNorm (cnet).
hipError_t run_norm(af_raft* r, const BNorm* bn, float* x, long long P, int C, int relu, const float* res, float* y) {
  hipStream_t s = r->stream;
  const float *al = r->in_alpha, *be = r->in_beta;
  if (bn) { al = bn->alpha; be = bn->beta; }
  else {
    const int nchunk = (int)((P + IN_CHUNK - 1) / IN_CHUNK);
    hipLaunchKernelGGL(k_in_partial, dim3(nchunk), dim3(256), 0, s, x, P, C, r->in_part);
    hipLaunchKernelGGL(k_in_final, dim3((C + 63) / 64), dim3(64), 0, s, r->in_part, nchunk, P, C, r->in_alpha, r->in_beta);
  }
  hipLaunchKernelGGL(k_affine, dim3(nblk(P * C)), dim3(256), 0, s, x, al, be, relu, res, y, P, C, (int)(r->prec == AF_RAFT_FP16));
  return hipGetLastError();
}

hipError_t run_encoder(af_raft* r, int which, float* out, int act) {
  const Encoder& E = r->enc[which];
  const bool bn = which == 1;
  hipStream_t s = r->stream;
  hipError_t e;
  int H = r->Hp / 2, W = r->Wp / 2;
  float *X = r->sx, *A = r->sa, *Bf = r->sb, *D = r->sd;
  Epi plain;
  RCHK(launch_rconv(E.conv1, r->img, 3, 1, r->Hp, r->Wp, X, 64, plain, s, r->prec));
  RCHK(run_norm(r, bn ? &E.n0 : nullptr, X, (long long)H * W, 64, 1, nullptr, X));
  int cin = 64;
  for (int i = 0; i < 6; ++i) {
    const int c = kBlockC[i], st = kBlockS[i];
    const int Ho = (H - 1) / st + 1, Wo = (W - 1) / st + 1;
    const long long Po = (long long)Ho * Wo;
    RCHK(launch_rconv(E.c1[i], X, cin, 1, H, W, A, c, plain, s, r->prec));
    RCHK(run_norm(r, bn ? &E.n1[i] : nullptr, A, Po, c, 1, nullptr, A));
    RCHK(launch_rconv(E.c2[i], A, c, 1, Ho, Wo, Bf, c, plain, s, r->prec));
    const float* res = X;
    if (st != 1) {
      RCHK(launch_rconv(E.down[i], X, cin, 1, H, W, D, c, plain, s, r->prec));
      RCHK(run_norm(r, bn ? &E.n3[i] : nullptr, D, Po, c, 0, nullptr, D));
      res = D;
    }
    RCHK(run_norm(r, bn ? &E.n2[i] : nullptr, Bf, Po, c, 1, res, Bf));      // relu(x + relu(norm2(conv2)))
    std::swap(X, Bf);
    H = Ho; W = Wo; cin = c;
  }
  Epi ep; ep.act = act;
  return launch_rconv(E.conv2, X, 128, 1, H, W, out, 256, ep, s, r->prec);
}

// The state of batch element e for the pair-direction a -> b: hidden state, context, coords and the correlation pyramid.
hipError_t setup_element(af_raft* r, int e_, int a, int b) {
  hipStream_t s = r->stream;
  hipError_t e;
  const long long P = r->P;
  const float* ctx = r->ctx + (size_t)a * P * 256;
  float *hx = r->hx + (size_t)e_ * P * HXC, *rhx = r->rhx + (size_t)e_ * P * HXC;
  hipLaunchKernelGGL(k_slice, dim3(nblk(P * 256)), dim3(256), 0, s, ctx, 256LL, hx, (long long)HXC, P, 256);              // h | inp
  hipLaunchKernelGGL(k_slice, dim3(nblk(P * HD)), dim3(256), 0, s, ctx + HD, 256LL, rhx + HD, (long long)HXC, P, HD);      // inp
  RCHK(hipGetLastError());
  RCHK(hipMemcpyAsync(r->coords1 + (size_t)e_ * P * 2, r->coords0, P * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
  // all-pairs correlation: fmap(a) (P, 256) times fmap(b)^T [256][Npad], / 16 (fp32 in either precision mode, as the reference's fmap.float())
  ConvLayer L; L.cout = (int)P; L.cin_used = 256; L.K = 256; L.Kpad = 256; L.Npad = r->Npad; L.wt = r->fmapT + (size_t)b * 256 * r->Npad; L.bias = nullptr;
  Epi ep; ep.oscale = 0.0625f;
  RCHK(launch_rconv(L, r->fmap + (size_t)a * P * 256, 256, 1, r->h8, r->w8, r->vol[0] + (size_t)e_ * P * P, P, ep, s));
  for (int l = 1; l < 4; ++l) {
    const long long n = P * r->lh[l] * r->lw[l];
    hipLaunchKernelGGL(k_pool, dim3(nblk(n)), dim3(256), 0, s, r->vol[l - 1] + (size_t)e_ * P * r->lh[l - 1] * r->lw[l - 1], P, r->lh[l - 1], r->lw[l - 1],
                       r->vol[l] + (size_t)e_ * n);
  }
  return hipGetLastError();
}

Pyr pyramid(const af_raft* r) {
  Pyr py;
  for (int l = 0; l < 4; ++l) { py.lvl[l] = r->vol[l]; py.h[l] = r->lh[l]; py.w[l] = r->lw[l]; py.bstride[l] = (long long)r->P * r->lh[l] * r->lw[l]; }
  return py;
}

// One update iteration of B batch elements.
hipError_t run_iteration(af_raft* r, int B) {
  hipStream_t s = r->stream;
  hipError_t e;
  const Update& U = r->up;
  const int h = r->h8, w = r->w8;
  const long long M = (long long)B * r->P;
  hipLaunchKernelGGL(k_lookup, dim3(nblk(M * CORRC)), dim3(256), 0, s, pyramid(r), r->coords1, B, r->P, r->corr);
  hipLaunchKernelGGL(k_flow, dim3(nblk(M * 2)), dim3(256), 0, s, r->coords1, r->coords0, M * 2, r->flow, r->hx, r->rhx);
  RCHK(hipGetLastError());
  Epi relu; relu.act = ACT_RELU;
  RCHK(launch_rconv(U.convc1, r->corr, CORRC, B, h, w, r->c1, 256, relu, s, r->prec));
  RCHK(launch_rconv(U.convc2, r->c1, 256, B, h, w, r->corflo, 256, relu, s, r->prec));
  RCHK(launch_rconv(U.convf1, r->flow, 2, B, h, w, r->f1, 128, relu, s, r->prec));
  RCHK(launch_rconv(U.convf2, r->f1, 128, B, h, w, r->corflo + 192, 256, relu, s, r->prec));
  Epi mo = relu; mo.y2 = r->rhx + 256; mo.ldy2 = HXC;
  RCHK(launch_rconv(U.conv, r->corflo, 256, B, h, w, r->hx + 256, HXC, mo, s, r->prec));
  for (int g = 0; g < 2; ++g) {
    Epi zr; zr.epi = EPI_GRU_ZR; zr.h = r->hx; zr.ldh = HXC; zr.z = r->z;
    RCHK(launch_rconv(U.zr[g], r->hx, HXC, B, h, w, r->rhx, HXC, zr, s, r->prec));
    Epi q; q.epi = EPI_GRU_Q; q.h = r->hx; q.ldh = HXC; q.z = r->z;
    RCHK(launch_rconv(U.q[g], r->rhx, HXC, B, h, w, r->hx, HXC, q, s, r->prec));
  }
  RCHK(launch_rconv(U.fh1, r->hx, HXC, B, h, w, r->fh, 256, relu, s, r->prec));
  Epi none;
  RCHK(launch_rconv(U.fh2, r->fh, 256, B, h, w, r->delta, 2, none, s, r->prec));
  hipLaunchKernelGGL(k_axpy1, dim3(nblk(M * 2)), dim3(256), 0, s, r->coords1, r->delta, M * 2);
  return hipGetLastError();
}

// After the last iteration: flow = coords1 - coords0, the mask head (x 0.25) and the convex upsampling.
hipError_t run_tail(af_raft* r, int B) {
  hipStream_t s = r->stream;
  hipError_t e;
  const long long M = (long long)B * r->P;
  hipLaunchKernelGGL(k_flow, dim3(nblk(M * 2)), dim3(256), 0, s, r->coords1, r->coords0, M * 2, r->flow, (float*)nullptr, (float*)nullptr);
  RCHK(hipGetLastError());
  Epi relu; relu.act = ACT_RELU;
  RCHK(launch_rconv(r->up.mk0, r->hx, HXC, B, r->h8, r->w8, r->fh, 256, relu, s, r->prec));
  Epi q; q.oscale = 0.25f;
  RCHK(launch_rconv(r->up.mk2, r->fh, 256, B, r->h8, r->w8, r->mask, 576, q, s, r->prec));
  hipLaunchKernelGGL(k_upsample, dim3(nblk((long long)B * r->Hp * r->Wp)), dim3(256), 0, s, r->flow, r->mask, B, r->h8, r->w8, r->upf);
  return hipGetLastError();
}
#undef RCHK

}  // namespace

extern "C" {

int af_raft_create(int device_ordinal, int h, int w, int capacity, af_raft** out) {
  if (!out) return fail(AF_EINVAL, "af_raft_create: null argument");
  *out = nullptr;
  if (h <= 0 || w <= 0 || h > 8192 || w > 8192 || capacity < 1 || capacity > 64) return fail(AF_EINVAL, "af_raft_create: h and w must be 1..8192, capacity 1..64");
  const int Hp = h + (((h / 8) + 1) * 8 - h) % 8, Wp = w + (((w / 8) + 1) * 8 - w) % 8;
  if (Hp < 128 || Wp < 128)
    return fail(AF_EINVAL, "af_raft_create: the padded frame must be at least 128 x 128: below a 16 x 16 grid the coarsest correlation level is one cell wide and the reference's "
                           "2 x / (W - 1) divides by zero (its flow is NaN)");
  const long long P = (long long)(Hp / 8) * (Wp / 8);
  if (P * P * capacity > (1LL << 36)) return fail(AF_EINVAL, "af_raft_create: correlation volumes of this capacity exceed 256 GiB");
  hipError_t e = hipSetDevice(device_ordinal);
  if (e != hipSuccess) return hfail("af_raft_create: hipSetDevice", e);
  af_raft* r = new af_raft();
  r->device = device_ordinal; r->h = h; r->w = w; r->Hp = Hp; r->Wp = Wp; r->top = (Hp - h) / 2; r->left = (Wp - w) / 2;
  r->cap = capacity; r->slots = 2 * capacity; r->h8 = Hp / 8; r->w8 = Wp / 8; r->P = (int)P; r->Npad = (int)((P + 127) / 128 * 128);
  r->slot_valid.assign(r->slots, 0);
  for (int l = 0; l < 4; ++l) { r->lh[l] = r->h8 >> l; r->lw[l] = r->w8 >> l; }
  e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
  const size_t P2 = (size_t)(Hp / 2) * (Wp / 2), B = capacity;
  r->img_in = r->alloc((size_t)h * w * 3, e); r->img = r->alloc((size_t)Hp * Wp * 3, e);
  r->sx = r->alloc(P2 * 64, e); r->sa = r->alloc(P2 * 64, e); r->sb = r->alloc(P2 * 64, e); r->sd = r->alloc(P2 * 64, e);
  r->in_alpha = r->alloc(128, e); r->in_beta = r->alloc(128, e);
  if (e == hipSuccess) e = hipMalloc(&r->in_part, ((P2 + IN_CHUNK - 1) / IN_CHUNK) * 128 * 2 * sizeof(double));
  r->fmap = r->alloc((size_t)r->slots * P * 256, e); r->fmapT = r->alloc((size_t)r->slots * 256 * r->Npad, e); r->ctx = r->alloc((size_t)r->slots * P * 256, e);
  for (int l = 0; l < 4; ++l) r->vol[l] = r->alloc(B * P * r->lh[l] * r->lw[l], e);
  r->hx = r->alloc(B * P * HXC, e); r->rhx = r->alloc(B * P * HXC, e); r->corr = r->alloc(B * P * CORRC, e); r->c1 = r->alloc(B * P * 256, e);
  r->corflo = r->alloc(B * P * 256, e); r->f1 = r->alloc(B * P * 128, e); r->z = r->alloc(B * P * HD, e); r->fh = r->alloc(B * P * 256, e);
  r->delta = r->alloc(B * P * 2, e); r->coords0 = r->alloc(B * P * 2, e); r->coords1 = r->alloc(B * P * 2, e); r->flow = r->alloc(B * P * 2, e);
  r->mask = r->alloc(B * P * 576, e); r->upf = r->alloc(B * (size_t)Hp * Wp * 2, e);
  if (e == hipSuccess) e = hipMemsetAsync(r->fmapT, 0, (size_t)r->slots * 256 * r->Npad * 4, r->stream);
  if (e == hipSuccess) { hipLaunchKernelGGL(k_coords0, dim3(nblk(B * P)), dim3(256), 0, r->stream, r->coords0, (int)B, r->h8, r->w8); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e != hipSuccess) { delete r; return hfail("af_raft_create", e); }
  *out = r;
  return AF_OK;
}

void af_raft_destroy(af_raft* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipStreamSynchronize(r->stream);
  delete r;
}

size_t af_raft_param_count(const af_raft* r) { return r ? raft_param_count() : 0; }

int af_raft_info(const af_raft* r, int* hp, int* wp, int* slots) {
  if (!r) return fail(AF_EINVAL, "af_raft_info: null handle");
  if (hp) *hp = r->Hp;
  if (wp) *wp = r->Wp;
  if (slots) *slots = r->slots;
  return AF_OK;
}

int af_raft_set_precision(af_raft* r, int precision) {
  if (!r) return fail(AF_EINVAL, "af_raft_set_precision: null handle");
  if (precision != AF_RAFT_FP32 && precision != AF_RAFT_FP16)
    return fail(AF_EINVAL, "af_raft_set_precision: precision must be AF_RAFT_FP32 (0) or AF_RAFT_FP16 (1), got " + std::to_string(precision));
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  if ((e = hipStreamSynchronize(r->stream)) != hipSuccess) return hfail("af_raft_set_precision", e);
  r->prec = precision;
  std::fill(r->slot_valid.begin(), r->slot_valid.end(), 0);       // the encoded frames are the other arithmetic's
  r->last_a = r->last_b = -1; r->last_iters = 0;
  return AF_OK;
}

int af_raft_get_precision(const af_raft* r, int* precision) {
  if (!r || !precision) return fail(AF_EINVAL, "af_raft_get_precision: null argument");
  *precision = r->prec;
  return AF_OK;
}

int af_raft_set_params(af_raft* r, const float* flat, size_t n) {
  if (!r || !flat) return fail(AF_EINVAL, "af_raft_set_params: arguments");
  if (n != raft_param_count()) return fail(AF_EINVAL, "af_raft_set_params: expected " + std::to_string(raft_param_count()) + " parameters, got " + std::to_string(n));
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  if ((e = hipStreamSynchronize(r->stream)) != hipSuccess) return hfail("af_raft_set_params", e);
  r->loaded = false;
  std::fill(r->slot_valid.begin(), r->slot_valid.end(), 0);
  Cursor c{flat, n};
  if ((e = walk_encoder(c, &r->enc[0], false, 256)) != hipSuccess || (e = walk_encoder(c, &r->enc[1], true, 256)) != hipSuccess ||
      (e = walk_update(c, &r->up)) != hipSuccess)
    return hfail("af_raft_set_params", e);
  if (!c.ok || c.left != 0) return fail(AF_EINVAL, "af_raft_set_params: parameter walk does not match the count");
  r->loaded = true;
  return AF_OK;
}

int af_raft_encode(af_raft* r, int slot, const float* image, int on_device) {
  if (!r || !image || slot < 0 || slot >= r->slots) return fail(AF_EINVAL, "af_raft_encode: arguments (slot must be 0.." + std::to_string(r ? r->slots - 1 : 0) + ")");
  if (!r->loaded) return fail(AF_ESTATE, "af_raft_encode: parameters must be set first");
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  hipStream_t s = r->stream;
  const float* src = image;
  if (!on_device) {
    if ((e = hipMemcpyAsync(r->img_in, image, (size_t)r->h * r->w * 3 * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return hfail("upload image", e);
    src = r->img_in;
  } else if ((e = hipDeviceSynchronize()) != hipSuccess) {
    return hfail("af_raft_encode", e);
  }
  r->slot_valid[slot] = 0;
  hipLaunchKernelGGL(k_prep, dim3(nblk((long long)r->Hp * r->Wp * 3)), dim3(256), 0, s, src, r->h, r->w, r->img, r->Hp, r->Wp, r->top, r->left);
  if ((e = hipGetLastError()) != hipSuccess) return hfail("k_prep", e);
  float* fm = r->fmap + (size_t)slot * r->P * 256;
  if ((e = run_encoder(r, 0, fm, ACT_NONE)) != hipSuccess) return hfail("feature encoder", e);
  hipLaunchKernelGGL(k_transpose, dim3((r->P + 31) / 32, 256 / 32), dim3(256), 0, s, fm, r->P, 256, r->fmapT + (size_t)slot * 256 * r->Npad, r->Npad);
  if ((e = hipGetLastError()) != hipSuccess) return hfail("k_transpose", e);
  if ((e = run_encoder(r, 1, r->ctx + (size_t)slot * r->P * 256, ACT_TANH_RELU)) != hipSuccess) return hfail("context encoder", e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hfail("af_raft_encode", e);
  r->slot_valid[slot] = 1;
  return AF_OK;
}

static int check_pair(af_raft* r, int a, int b, const char* who) {
  if (a < 0 || a >= r->slots || b < 0 || b >= r->slots) return fail(AF_EINVAL, std::string(who) + ": slot out of range");
  if (!r->slot_valid[a] || !r->slot_valid[b]) return fail(AF_ESTATE, std::string(who) + ": a slot has no encoded frame");
  return AF_OK;
}

int af_raft_flow(af_raft* r, int n, const int* slot_a, const int* slot_b, int iters, float* flow_up, float* flow_lo, int on_device) {
  if (!r || !slot_a || !slot_b || n < 1 || iters < 1 || iters > 1000) return fail(AF_EINVAL, "af_raft_flow: arguments");
  if (n > r->cap) return fail(AF_EINVAL, "af_raft_flow: " + std::to_string(n) + " pair-directions, the handle's capacity is " + std::to_string(r->cap));
  if (!r->loaded) return fail(AF_ESTATE, "af_raft_flow: parameters must be set first");
  for (int i = 0; i < n; ++i) { const int rc = check_pair(r, slot_a[i], slot_b[i], "af_raft_flow"); if (rc != AF_OK) return rc; }
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  hipStream_t s = r->stream;
  for (int i = 0; i < n; ++i) if ((e = setup_element(r, i, slot_a[i], slot_b[i])) != hipSuccess) return hfail("correlation", e);
  for (int it = 0; it < iters; ++it) if ((e = run_iteration(r, n)) != hipSuccess) return hfail("update iteration", e);
  if ((e = run_tail(r, n)) != hipSuccess) return hfail("upsampling", e);
  r->last_a = slot_a[0]; r->last_b = slot_b[0]; r->last_iters = iters;
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (flow_up && (e = hipMemcpyAsync(flow_up, r->upf, (size_t)n * r->Hp * r->Wp * 2 * 4, k, s)) != hipSuccess) return hfail("copy flow", e);
  if (flow_lo && (e = hipMemcpyAsync(flow_lo, r->flow, (size_t)n * r->P * 2 * 4, k, s)) != hipSuccess) return hfail("copy 1/8 flow", e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hfail("af_raft_flow", e);
  return AF_OK;
}

int af_raft_step(af_raft* r, int slot_a, int slot_b, const float* net, const float* coords1, float* net_out, float* delta_out) {
  if (!r || !net || !coords1) return fail(AF_EINVAL, "af_raft_step: arguments");
  if (!r->loaded) return fail(AF_ESTATE, "af_raft_step: parameters must be set first");
  const int rc = check_pair(r, slot_a, slot_b, "af_raft_step"); if (rc != AF_OK) return rc;
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  hipStream_t s = r->stream;
  const size_t P = r->P;
  if ((e = setup_element(r, 0, slot_a, slot_b)) != hipSuccess) return hfail("correlation", e);
  std::vector<float> net16;
  if (r->prec == AF_RAFT_FP16) {        // the hidden state is an fp16 tensor in this mode: rounded once on upload (coords1 stays fp32)
    net16.resize(P * HD);
    for (size_t i = 0; i < P * HD; ++i) net16[i] = (float)(_Float16)net[i];
    net = net16.data();
  }
  if ((e = hipMemcpy2DAsync(r->hx, HXC * 4, net, HD * 4, HD * 4, P, hipMemcpyHostToDevice, s)) != hipSuccess) return hfail("upload state", e);
  if (r->prec == AF_RAFT_FP16 && (e = hipStreamSynchronize(s)) != hipSuccess) return hfail("upload state", e);
  if ((e = hipMemcpyAsync(r->coords1, coords1, P * 2 * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return hfail("upload state", e);
  if ((e = run_iteration(r, 1)) != hipSuccess) return hfail("update iteration", e);
  if ((e = run_tail(r, 1)) != hipSuccess) return hfail("upsampling", e);
  r->last_a = slot_a; r->last_b = slot_b; r->last_iters = 1;
  if (net_out && (e = hipMemcpy2DAsync(net_out, HD * 4, r->hx, HXC * 4, HD * 4, P, hipMemcpyDeviceToHost, s)) != hipSuccess) return hfail("copy net", e);
  if (delta_out && (e = hipMemcpyAsync(delta_out, r->delta, P * 2 * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return hfail("copy delta", e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hfail("af_raft_step", e);
  return AF_OK;
}

int af_raft_lookup(af_raft* r, int slot_a, int slot_b, const float* coords, float* out) {
  if (!r || !coords || !out) return fail(AF_EINVAL, "af_raft_lookup: arguments");
  if (!r->loaded) return fail(AF_ESTATE, "af_raft_lookup: parameters must be set first");
  const int rc = check_pair(r, slot_a, slot_b, "af_raft_lookup"); if (rc != AF_OK) return rc;
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  hipStream_t s = r->stream;
  const size_t P = r->P;
  if ((e = setup_element(r, 0, slot_a, slot_b)) != hipSuccess) return hfail("correlation", e);
  if ((e = hipMemcpyAsync(r->coords1, coords, P * 2 * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return hfail("upload coords", e);
  hipLaunchKernelGGL(k_lookup, dim3(nblk((long long)P * CORRC)), dim3(256), 0, s, pyramid(r), r->coords1, 1, r->P, r->corr);
  if ((e = hipGetLastError()) != hipSuccess) return hfail("k_lookup", e);
  if ((e = hipMemcpyAsync(out, r->corr, P * CORRC * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return hfail("copy lookup", e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hfail("af_raft_lookup", e);
  r->last_a = slot_a; r->last_b = slot_b; r->last_iters = 0;
  return AF_OK;
}

int af_raft_debug_activation(af_raft* r, const char* name, float* out, size_t n) {
  if (!r || !name || !out) return fail(AF_EINVAL, "af_raft_debug_activation: arguments");
  if (r->last_a < 0) return fail(AF_ESTATE, "af_raft_debug_activation: no flow has run");
  const size_t P = r->P;
  const float* src = nullptr; size_t rows = P, C = 0, ld = 0;
  const std::string s(name);
  if (s == "fmap1") { src = r->fmap + (size_t)r->last_a * P * 256; C = ld = 256; }
  else if (s == "fmap2") { src = r->fmap + (size_t)r->last_b * P * 256; C = ld = 256; }
  else if (s == "net0") { src = r->ctx + (size_t)r->last_a * P * 256; C = HD; ld = 256; }
  else if (s == "inp") { src = r->ctx + (size_t)r->last_a * P * 256 + HD; C = HD; ld = 256; }
  else if (s.size() == 7 && s.compare(0, 6, "corr_l") == 0 && s[6] >= '0' && s[6] <= '3') { src = r->corr + 81 * (s[6] - '0'); C = 81; ld = CORRC; }
  else if (s.size() == 9 && s.compare(0, 8, "corr_vol") == 0 && s[8] >= '0' && s[8] <= '3') { const int l = s[8] - '0'; src = r->vol[l]; C = ld = (size_t)r->lh[l] * r->lw[l]; }
  else if (s == "motion") { src = r->hx + 256; C = HD; ld = HXC; }
  else if (s == "net") { src = r->hx; C = HD; ld = HXC; }
  else if (s == "delta") { src = r->delta; C = ld = 2; }
  else if (s == "flow_lo") { src = r->flow; C = ld = 2; }
  else if (s == "mask") { src = r->mask; C = ld = 576; }
  else return fail(AF_EINVAL, std::string("af_raft_debug_activation: unknown name ") + name);
  if (r->last_iters == 0 && (s == "motion" || s == "net" || s == "delta" || s == "mask" || s == "flow_lo"))
    return fail(AF_ESTATE, std::string("af_raft_debug_activation: no update iteration has run (") + name + ")");
  if (n != rows * C) return fail(AF_EINVAL, std::string("af_raft_debug_activation: ") + name + " has " + std::to_string(rows * C) + " values");
  hipError_t e = hipSetDevice(r->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  if ((e = hipStreamSynchronize(r->stream)) != hipSuccess) return hfail("af_raft_debug_activation", e);
  if ((e = hipMemcpy2D(out, C * 4, src, ld * 4, C * 4, rows, hipMemcpyDeviceToHost)) != hipSuccess) return hfail("af_raft_debug_activation", e);
  return AF_OK;
}

static int bad_precision(const std::string& who, int precision) {
  return fail(AF_EINVAL, who + ": precision must be AF_RAFT_FP32 (0) or AF_RAFT_FP16 (1), got " + std::to_string(precision));
}

static int conv2d_impl(const std::string& who, int prec, int device_ordinal, const float* x, int batch, int h, int w, int cin, const float* weight, const float* bias,
                       int cout, int kh, int kw, int stride, int act, float* y) {
  if (prec != AF_RAFT_FP32 && prec != AF_RAFT_FP16) return bad_precision(who, prec);
  if (!x || !weight || !y || batch <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || kh < 1 || kw < 1 || kh > 7 || kw > 7 || !(kh & 1) || !(kw & 1) ||
      (stride != 1 && stride != 2) || (act != ACT_NONE && act != ACT_RELU && act != ACT_TANH && act != ACT_SIGMOID))
    return fail(AF_EINVAL, who + ": arguments");
  if ((long long)batch * h * w * std::max(cin, cout) > (1LL << 30)) return fail(AF_EINVAL, who + ": tensor too large");
  if (prec == AF_RAFT_FP16 && (h > 16384 || w > 16384)) return fail(AF_EINVAL, who + ": the fp16 tile packs a pixel's row and column into 16 bits each: h and w at most 16384");
  hipError_t e = hipSetDevice(device_ordinal); if (e != hipSuccess) return hfail("hipSetDevice", e);
  ConvLayer L;
  const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
  const size_t xb = (size_t)batch * h * w * cin * 4, yb = (size_t)batch * ho * wo * cout * 4;
  float *dx = nullptr, *dy = nullptr;
  e = upload_layer(L, cin, cin, kh, kw, stride, 0, {weight}, {bias}, cout);
  if (e == hipSuccess && prec == AF_RAFT_FP16) e = upload_layer_h(L, cin, {weight}, {bias}, cout);
  if (e == hipSuccess) e = hipMalloc(&dx, xb);
  if (e == hipSuccess) e = hipMalloc(&dy, yb);
  if (e == hipSuccess) e = hipMemcpy(dx, x, xb, hipMemcpyHostToDevice);
  Epi ep; ep.act = act;
  if (e == hipSuccess) e = launch_rconv(L, dx, cin, batch, h, w, dy, cout, ep, nullptr, prec);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(y, dy, yb, hipMemcpyDeviceToHost);
  free_layer(L); (void)hipFree(dx); (void)hipFree(dy);
  return e == hipSuccess ? AF_OK : hfail(who.c_str(), e);
}

int af_raft_conv2d(int device_ordinal, const float* x, int batch, int h, int w, int cin, const float* weight, const float* bias, int cout, int kh, int kw,
                   int stride, int act, float* y) {
  return conv2d_impl("af_raft_conv2d", AF_RAFT_FP32, device_ordinal, x, batch, h, w, cin, weight, bias, cout, kh, kw, stride, act, y);
}

int af_raft_conv2d_prec(int precision, int device_ordinal, const float* x, int batch, int h, int w, int cin, const float* weight, const float* bias, int cout,
                        int kh, int kw, int stride, int act, float* y) {
  return conv2d_impl("af_raft_conv2d_prec", precision, device_ordinal, x, batch, h, w, cin, weight, bias, cout, kh, kw, stride, act, y);
}

static int gru_impl(const std::string& who, int prec, int device_ordinal, int batch, int h, int w, int vertical, const float* net, const float* x, const float* wz,
                    const float* bz, const float* wr, const float* br, const float* wq, const float* bq, float* net_out) {
  if (prec != AF_RAFT_FP32 && prec != AF_RAFT_FP16) return bad_precision(who, prec);
  if (!net || !x || !wz || !bz || !wr || !br || !wq || !bq || !net_out || batch <= 0 || h <= 0 || w <= 0 || (long long)batch * h * w > (1 << 22))
    return fail(AF_EINVAL, who + ": arguments");
  if (prec == AF_RAFT_FP16 && (h > 16384 || w > 16384)) return fail(AF_EINVAL, who + ": the fp16 tile packs a pixel's row and column into 16 bits each: h and w at most 16384");
  hipError_t e = hipSetDevice(device_ordinal); if (e != hipSuccess) return hfail("hipSetDevice", e);
  const size_t M = (size_t)batch * h * w;
  const int kh = vertical ? 5 : 1, kw = vertical ? 1 : 5;
  ConvLayer Lzr, Lq;
  float *hx = nullptr, *rhx = nullptr, *z = nullptr;
  e = upload_layer(Lzr, HXC, HXC, kh, kw, 1, 0, {wz, wr}, {bz, br}, HD);
  if (e == hipSuccess) e = upload_layer(Lq, HXC, HXC, kh, kw, 1, 0, {wq}, {bq}, HD);
  if (e == hipSuccess && prec == AF_RAFT_FP16) e = upload_layer_h(Lzr, HXC, {wz, wr}, {bz, br}, HD);
  if (e == hipSuccess && prec == AF_RAFT_FP16) e = upload_layer_h(Lq, HXC, {wq}, {bq}, HD);
  if (e == hipSuccess) e = hipMalloc(&hx, M * HXC * 4);
  if (e == hipSuccess) e = hipMalloc(&rhx, M * HXC * 4);
  if (e == hipSuccess) e = hipMalloc(&z, M * HD * 4);
  if (e == hipSuccess) e = hipMemcpy2D(hx, HXC * 4, net, HD * 4, HD * 4, M, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy2D(hx + HD, HXC * 4, x, 256 * 4, 256 * 4, M, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy2D(rhx + HD, HXC * 4, x, 256 * 4, 256 * 4, M, hipMemcpyHostToDevice);
  Epi zr; zr.epi = EPI_GRU_ZR; zr.h = hx; zr.ldh = HXC; zr.z = z;
  if (e == hipSuccess) e = launch_rconv(Lzr, hx, HXC, batch, h, w, rhx, HXC, zr, nullptr, prec);
  Epi q; q.epi = EPI_GRU_Q; q.h = hx; q.ldh = HXC; q.z = z;
  if (e == hipSuccess) e = launch_rconv(Lq, rhx, HXC, batch, h, w, hx, HXC, q, nullptr, prec);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy2D(net_out, HD * 4, hx, HXC * 4, HD * 4, M, hipMemcpyDeviceToHost);
  free_layer(Lzr); free_layer(Lq); (void)hipFree(hx); (void)hipFree(rhx); (void)hipFree(z);
  return e == hipSuccess ? AF_OK : hfail(who.c_str(), e);
}

int af_raft_gru(int device_ordinal, int batch, int h, int w, int vertical, const float* net, const float* x, const float* wz, const float* bz, const float* wr,
                const float* br, const float* wq, const float* bq, float* net_out) {
  return gru_impl("af_raft_gru", AF_RAFT_FP32, device_ordinal, batch, h, w, vertical, net, x, wz, bz, wr, br, wq, bq, net_out);
}

int af_raft_gru_prec(int precision, int device_ordinal, int batch, int h, int w, int vertical, const float* net, const float* x, const float* wz, const float* bz,
                     const float* wr, const float* br, const float* wq, const float* bq, float* net_out) {
  return gru_impl("af_raft_gru_prec", precision, device_ordinal, batch, h, w, vertical, net, x, wz, bz, wr, br, wq, bq, net_out);
}

static int instance_norm_impl(const std::string& who, int prec, int device_ordinal, const float* x, int h, int w, int c, int relu, const float* residual, float* y) {
  if (prec != AF_RAFT_FP32 && prec != AF_RAFT_FP16) return bad_precision(who, prec);
  if (!x || !y || h <= 0 || w <= 0 || (c != 64 && c != 96 && c != 128) || (long long)h * w * c > (1LL << 30)) return fail(AF_EINVAL, who + ": arguments (c in 64, 96, 128)");
  hipError_t e = hipSetDevice(device_ordinal); if (e != hipSuccess) return hfail("hipSetDevice", e);
  const long long P = (long long)h * w;
  const int nchunk = (int)((P + IN_CHUNK - 1) / IN_CHUNK);
  float *dx = nullptr, *dr = nullptr, *ab = nullptr; double* part = nullptr;
  e = hipMalloc(&dx, P * c * 4);
  if (e == hipSuccess) e = hipMalloc(&ab, 256 * 4);
  if (e == hipSuccess) e = hipMalloc(&part, (size_t)nchunk * c * 2 * sizeof(double));
  if (e == hipSuccess && residual) e = hipMalloc(&dr, P * c * 4);
  if (e == hipSuccess) e = hipMemcpy(dx, x, P * c * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && residual) e = hipMemcpy(dr, residual, P * c * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_in_partial, dim3(nchunk), dim3(256), 0, nullptr, dx, P, c, part);
    hipLaunchKernelGGL(k_in_final, dim3((c + 63) / 64), dim3(64), 0, nullptr, part, nchunk, P, c, ab, ab + 128);
    hipLaunchKernelGGL(k_affine, dim3(nblk(P * c)), dim3(256), 0, nullptr, dx, ab, ab + 128, relu, dr, dx, P, c, (int)(prec == AF_RAFT_FP16));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(y, dx, P * c * 4, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dr); (void)hipFree(ab); (void)hipFree(part);
  return e == hipSuccess ? AF_OK : hfail(who.c_str(), e);
}

int af_raft_instance_norm(int device_ordinal, const float* x, int h, int w, int c, int relu, const float* residual, float* y) {
  return instance_norm_impl("af_raft_instance_norm", AF_RAFT_FP32, device_ordinal, x, h, w, c, relu, residual, y);
}

int af_raft_instance_norm_prec(int precision, int device_ordinal, const float* x, int h, int w, int c, int relu, const float* residual, float* y) {
  return instance_norm_impl("af_raft_instance_norm_prec", precision, device_ordinal, x, h, w, c, relu, residual, y);
}

}  // extern "C"
