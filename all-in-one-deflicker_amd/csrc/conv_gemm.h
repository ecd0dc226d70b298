// conv_gemm.h — the implicit-GEMM convolution core of stage 2 (filter.hip, k_conv) and of the RAFT precompute (raft.hip, k_rconv), and
// the host side that goes with it: the layer record, the OIHW -> [Kpad][Npad] repack + upload, the BN launch dispatch, the handle's
// allocation pool and the error helpers.  Everything lands in the including unit's anonymous namespace.
//
// M = output pixels (of B stacked images), N = output channels, K = (ky, kx, ci).  A block owns a 128 x BN tile; K runs in chunks of 16
// on the fp32-input matrix pipe (v_mfma_f32_32x32x2_f32: exact fp32 products, a k-ordered fmaf chain).  The two kernels stay two
// instantiation families of conv_tile: the compile-time switches keep the batch index out of stage 2's gather (it costs k_rconv<32> a
// wave of occupancy) and the reflection branch out of RAFT's.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/atlasfit.h"

extern "C" void af_set_thread_error(const char* m);     // host.hip: the message af_last_error(NULL) reports

namespace {

constexpr int CBM = 128, CBK = 16;        // conv tile: 128 output pixels x BN output channels, K in chunks of 16

struct ConvGeom {
  const float* x; long long ldx;          // input: B images (H, W, Cin) stacked, pixel stride ldx (a channel slice of a wider buffer)
  int B, H, W, Cin;
  const float* wt;                        // [Kpad][Npad]: row k = (ky * kw + kx) * Cin + ci, zero rows / columns beyond K / Cout
  const float* bias;                      // [Npad] or null
  int K, Kpad, Npad, Cout;
  int kh, kw, stride, padh, padw, reflect;      // pad = k / 2 per axis; reflect: ReflectionPad2d, else zero padding
  int Ho, Wo;
};

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// One tile: epi(m, co, sum + bias) for every output element (m < M, co < Cout) of block (blockIdx.x, blockIdx.y).
// BATCH: B images along M (else B is not read and M = Ho * Wo).  REFLECT: g.reflect is honoured (else it is not read: zero padding).
template <int BN, bool BATCH, bool REFLECT, class Epi>
__device__ __forceinline__ void conv_tile(const ConvGeom& g, const Epi& epi) {
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  constexpr int NT = BN / 32, BPT = BN * CBK / 256;
  __shared__ float As[CBK][CBM + 1];
  __shared__ float Bs[CBK][BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int PO = g.Ho * g.Wo, M = BATCH ? g.B * PO : PO;
  const int m0 = blockIdx.x * CBM, n0 = blockIdx.y * BN;
  // each thread gathers one k (tid & 15) of 8 pixels (tid >> 4) + 16 j per chunk: 16 neighbouring threads read 16 consecutive channels
  const int kk = tid & 15;
  int iy0[8], ix0[8], ib[BATCH ? 8 : 1];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + (tid >> 4) + 16 * j;
    if (m < M) {
      int p = m;
      if constexpr (BATCH) { const int b = m / PO; p = m - b * PO; ib[j] = b * g.H * g.W; }
      const int oy = p / g.Wo, ox = p - oy * g.Wo;
      iy0[j] = oy * g.stride - g.padh; ix0[j] = ox * g.stride - g.padw;
    } else {
      iy0[j] = -(1 << 28); ix0[j] = 0;      // a pixel past M: reads 0
      if constexpr (BATCH) ib[j] = 0;
    }
  }
  float ra[8], rb[BPT];
  auto load = [&](int k0) {
    const int k = k0 + kk;
    const bool kv = k < g.K;
    int ky = 0, kx = 0, ci = 0;
    if (kv) { const int tap = k / g.Cin; ci = k - tap * g.Cin; ky = tap / g.kw; kx = tap - ky * g.kw; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int iy = iy0[j] + ky, ix = ix0[j] + kx;
      float v = 0.f;
      if constexpr (REFLECT) {
        if (kv && iy0[j] > -(1 << 27)) {      // reflection would fold a pixel past M back into the image
          if (g.reflect) { iy = reflect_idx(iy, g.H); ix = reflect_idx(ix, g.W); }
          if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = g.x[((size_t)(BATCH ? ib[j] : 0) + (size_t)iy * g.W + ix) * g.ldx + ci];
        }
      } else {
        if (kv && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = g.x[((size_t)(BATCH ? ib[j] : 0) + (size_t)iy * g.W + ix) * g.ldx + ci];
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const int e = tid + 256 * j, n = e % BN, kr = e / BN;
      rb[j] = g.wt[(size_t)(k0 + kr) * g.Npad + n0 + n];
    }
  };
  // two-level sum: each K chunk of 16 is one MFMA chain from zero (acc), added to the running sum (tot) after the chunk with Kahan's
  // compensation (cmp), so no fmaf chain is longer than 16 terms and the running sum of K / 16 chunk sums adds no error of its own
  const f32x16 zero = (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 tot[NT], cmp[NT], acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { tot[t] = zero; cmp[t] = zero; }
  load(0);
  for (int k0 = 0; k0 < g.Kpad; k0 += CBK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) As[kk][(tid >> 4) + 16 * j] = ra[j];
#pragma unroll
    for (int j = 0; j < BPT; ++j) { const int e = tid + 256 * j; Bs[e / BN][e % BN] = rb[j]; }
    __syncthreads();
    if (k0 + CBK < g.Kpad) load(k0 + CBK);      // the next chunk's global loads overlap this chunk's products
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = zero;
#pragma unroll
    for (int s = 0; s < CBK / 2; ++s) {
      const int kr = 2 * s + (lane >> 5);
      const float av = As[kr][32 * wave + (lane & 31)];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Bs[kr][32 * t + (lane & 31)], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x16 y = acc[t] - cmp[t], n = tot[t] + y;
      cmp[t] = (n - tot[t]) - y;
      tot[t] = n;
    }
    __syncthreads();
  }
  // C/D layout of the 32x32 form: column = lane & 31 (output channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pixel)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int co = n0 + 32 * t + (lane & 31);
    if (co >= g.Cout) continue;
    const float b = g.bias ? g.bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m < M) epi(m, co, tot[t][r] + b);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

inline unsigned nblk(long long n) { return (unsigned)((n + 255) / 256); }
inline int conv_bn(int cout) { return cout <= 32 ? 32 : (cout <= 64 ? 64 : 128); }

inline int fail(int code, const std::string& m) { af_set_thread_error(m.c_str()); return code; }
inline int hfail(const char* what, hipError_t e) { return fail(e == hipErrorOutOfMemory ? AF_ENOMEM : AF_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }

// The device buffers of a handle: freed with it.  A failed allocation is carried in `e`; the calls after it do nothing.
struct DevPool {
  std::vector<float*> allocs;
  float* alloc(size_t floats, hipError_t& e) {
    float* p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, std::max<size_t>(floats, 1) * sizeof(float));
    if (e == hipSuccess) allocs.push_back(p);
    return p;
  }
  ~DevPool() { for (float* p : allocs) (void)hipFree(p); }
};

struct ConvLayer {
  int cout = 0, cin_used = 0, kh = 1, kw = 1, stride = 1, reflect = 0; float *wt = nullptr, *bias = nullptr; int K = 0, Kpad = 0, Npad = 0;
  void* wt16 = nullptr; float* bias16 = nullptr; int Kpad16 = 0;      // the fp16 image of the fp16 precision modes (conv_gemm_h.h); null elsewhere
};

inline void free_layer(ConvLayer& L) {
  (void)hipFree(L.wt); (void)hipFree(L.bias); (void)hipFree(L.wt16); (void)hipFree(L.bias16);
  L.wt = L.bias = L.bias16 = nullptr; L.wt16 = nullptr;
}

// OIHW weights (cout_each, cin, kh, kw) of `parts` convolutions over the same input, concatenated along the output channels, of which
// the first cin_used input channels are read -> wt [Kpad][Npad] with row (ky * kw + kx) * cin_used + ci, and the biases -> [Npad]
// (L.bias stays null when no part has one).  Replaces what L held; on an error L holds nothing.
inline hipError_t upload_layer(ConvLayer& L, int cin, int cin_used, int kh, int kw, int stride, int reflect, const std::vector<const float*>& w,
                               const std::vector<const float*>& b, int cout_each) {
  const int parts = (int)w.size();
  free_layer(L);
  L.cout = cout_each * parts; L.cin_used = cin_used; L.kh = kh; L.kw = kw; L.stride = stride; L.reflect = reflect;
  const int bn = conv_bn(L.cout);
  L.K = kh * kw * cin_used; L.Kpad = (L.K + CBK - 1) / CBK * CBK; L.Npad = (L.cout + bn - 1) / bn * bn;
  std::vector<float> wt((size_t)L.Kpad * L.Npad, 0.f), bias(L.Npad, 0.f);
  bool has_bias = false;
  for (int q = 0; q < parts; ++q)
    for (int o = 0; o < cout_each; ++o) {
      for (int ci = 0; ci < cin_used; ++ci)
        for (int ky = 0; ky < kh; ++ky)
          for (int kx = 0; kx < kw; ++kx)
            wt[(size_t)((ky * kw + kx) * cin_used + ci) * L.Npad + q * cout_each + o] = w[q][(((size_t)o * cin + ci) * kh + ky) * kw + kx];
      if (b[q]) { bias[q * cout_each + o] = b[q][o]; has_bias = true; }
    }
  hipError_t e = hipMalloc(&L.wt, wt.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(L.wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && has_bias) e = hipMalloc(&L.bias, bias.size() * 4);
  if (e == hipSuccess && has_bias) e = hipMemcpy(L.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) free_layer(L);
  return e;
}

// The geometry of layer L on B images (H, W) at pixel stride ldx.
inline ConvGeom conv_geom(const ConvLayer& L, const float* x, long long ldx, int B, int H, int W) {
  ConvGeom g;
  g.x = x; g.ldx = ldx; g.B = B; g.H = H; g.W = W; g.Cin = L.cin_used;
  g.wt = L.wt; g.bias = L.bias; g.K = L.K; g.Kpad = L.Kpad; g.Npad = L.Npad; g.Cout = L.cout;
  g.kh = L.kh; g.kw = L.kw; g.stride = L.stride; g.padh = L.kh / 2; g.padw = L.kw / 2; g.reflect = L.reflect;
  g.Ho = (H + 2 * g.padh - g.kh) / g.stride + 1; g.Wo = (W + 2 * g.padw - g.kw) / g.stride + 1;
  return g;
}

// Launches the instantiation of a kernel family (k<32>, k<64>, k<128>; Args holds the geometry as `g`) that conv_bn picks for a.g.Cout.
template <class Args>
inline hipError_t launch_conv_family(void (*k32)(Args), void (*k64)(Args), void (*k128)(Args), const Args& a, hipStream_t s) {
  const int bn = conv_bn(a.g.Cout);
  const dim3 grid((unsigned)(((long long)a.g.B * a.g.Ho * a.g.Wo + CBM - 1) / CBM), (unsigned)(a.g.Npad / bn));
  void (*k)(Args) = bn == 32 ? k32 : (bn == 64 ? k64 : k128);
  hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace
