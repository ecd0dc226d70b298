// conv_gemm_h.h — the fp16 tile of the implicit-GEMM convolution core (conv_gemm.h), for the two fp16 precision modes: AF_RAFT_FP16
// (raft.hip, k_rconv_h: what the reference's encoders and update block compute under fp16 autocast on a GPU) and AF_FILTER_FP16
// (filter.hip, k_conv_h: both stage-2 nets under the same autocast).
//
// Same 128 x BN tile, same M / N / K and the same C/D walk as conv_tile; K runs in chunks of 32 on v_mfma_f32_32x32x16_f16.  The input
// stays NHWC fp32 in HBM and is rounded to fp16 (nearest even, subnormals kept, overflow to inf) as it is gathered; the weights come
// from an fp16 image [Npad][Kpad16] (k contiguous, Kpad16 a multiple of 32), so that a thread copies 16 bytes global -> LDS.  Both LDS
// tiles hold the 8 k of a lane contiguous: an operand fragment is one 16-byte read.  Rows are padded to 40 halves (80 bytes): the 16
// lanes of a ds_read_b128 group then sit on 16 different 16-byte slots of the 256-byte bank row (5 r mod 16 is a permutation).
// Products of fp16 values are exact in fp32 and are accumulated in the MFMA's fp32 accumulator.  As in conv_tile each K chunk is a chain
// from zero that joins the running sum with Kahan's compensation.  A plain chain over all of K rounds the running sum K / 16 times, and
// that error puts fp16(sum + bias) on the other side of a rounding boundary more often: on the 7x7 layer with K = 1617 of
// tests/test_gpu_raft_fp16.py, 14 of 16800 outputs differed from the fp64 contract with the plain chain, one of them by an ulp of
// 2^-9, against 8 with the compensated sum, all of them near zero (differences up to 2^-13).  epi receives fp16(sum + bias16) as a float.
// As conv_tile, the tile has the compile-time switches BATCH and REFLECT, and the two kernel families instantiate one side of each:
// RAFT <BN, true, false> (its gather is the code it was before the switch existed), stage 2 <BN, false, true>.
#pragma once
#include "conv_gemm.h"

namespace {

constexpr int HBK = 32, HLD = HBK + 8;     // K chunk; halves per LDS row

__device__ __forceinline__ float round_h(float v) { return (float)(_Float16)v; }

// ConvGeom of the fp16 route: g.wt is the fp16 image [Npad][g.Kpad] (Kpad a multiple of HBK), g.bias the fp16-rounded biases as floats.
// BATCH: B images along M (else B is not read and M = Ho * Wo).  REFLECT: g.reflect is honoured (else it is not read: zero padding).
template <int BN, bool BATCH, bool REFLECT, class Epi>
__device__ __forceinline__ void conv_tile_h(const ConvGeom& g, const Epi& epi) {
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
  constexpr int NT = BN / 32, NPIECE = BN * (HBK / 8), BPT = (NPIECE + 255) / 256;      // weight pieces of 8 halves
  __shared__ __attribute__((aligned(16))) _Float16 As[CBM][HLD];
  __shared__ __attribute__((aligned(16))) _Float16 Bs[BN][HLD];
  const _Float16* wt = reinterpret_cast<const _Float16*>(g.wt);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int PO = g.Ho * g.Wo, M = BATCH ? g.B * PO : PO;
  const int m0 = blockIdx.x * CBM, n0 = blockIdx.y * BN;
  // each thread gathers one k (tid & 31) of 16 pixels (tid >> 5) + 8 j per chunk: 32 neighbouring threads read 32 consecutive channels
  const int kk = tid & 31;
  int yx0[16], ib[BATCH ? 16 : 1];      // (iy0 << 16) | (ix0 & 0xffff), a register per pixel less: the callers keep H and W at or below 16384
  unsigned inm = 0;                     // REFLECT: bit j = pixel j lies below M (reflection would fold the sentinel row back into the image)
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int m = m0 + (tid >> 5) + 8 * j;
    if (m < M) {
      int p = m;
      if constexpr (BATCH) { const int b = m / PO; p = m - b * PO; ib[j] = b * g.H * g.W; }
      const int oy = p / g.Wo, ox = p - oy * g.Wo;
      yx0[j] = (int)((unsigned)(oy * g.stride - g.padh) << 16) | ((ox * g.stride - g.padw) & 0xffff);
      if constexpr (REFLECT) inm |= 1u << j;
    } else {
      yx0[j] = (int)0xc0000000u;            // a pixel past M: row -16384, reads 0
      if constexpr (BATCH) ib[j] = 0;
    }
  }
  float ra[16];
  u32x4 rb[BPT];
  auto load = [&](int k0) {
    const int k = k0 + kk;
    const bool kv = k < g.K;
    int ky = 0, kx = 0, ci = 0;
    if (kv) { const int tap = k / g.Cin; ci = k - tap * g.Cin; ky = tap / g.kw; kx = tap - ky * g.kw; }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int iy = (yx0[j] >> 16) + ky, ix = (int)(short)(yx0[j] & 0xffff) + kx;
      float v = 0.f;
      if constexpr (REFLECT) {
        if (kv && (inm >> j & 1u)) {
          if (g.reflect) { iy = reflect_idx(iy, g.H); ix = reflect_idx(ix, g.W); }      // single reflection: the callers keep the pad below the size
          if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = g.x[((size_t)(BATCH ? ib[j] : 0) + (size_t)iy * g.W + ix) * g.ldx + ci];
        }
      } else {
        if (kv && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = g.x[((size_t)(BATCH ? ib[j] : 0) + (size_t)iy * g.W + ix) * g.ldx + ci];
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const int e = tid + 256 * j;
      if (NPIECE % 256 == 0 || e < NPIECE) rb[j] = *reinterpret_cast<const u32x4*>(wt + (size_t)(n0 + (e >> 2)) * g.Kpad + k0 + 8 * (e & 3));
    }
  };
  const f32x16 zero = (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 tot[NT], cmp[NT], acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { tot[t] = zero; cmp[t] = zero; }
  load(0);
  for (int k0 = 0; k0 < g.Kpad; k0 += HBK) {
#pragma unroll
    for (int j = 0; j < 16; ++j) As[(tid >> 5) + 8 * j][kk] = (_Float16)ra[j];      // the operand rounding: nearest even
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const int e = tid + 256 * j;
      if (NPIECE % 256 == 0 || e < NPIECE) *reinterpret_cast<u32x4*>(&Bs[e >> 2][8 * (e & 3)]) = rb[j];
    }
    __syncthreads();
    if (k0 + HBK < g.Kpad) load(k0 + HBK);      // the next chunk's global loads overlap this chunk's products
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = zero;
    // operand lane map of the 32x32x16 form: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j = 0..7
#pragma unroll
    for (int s = 0; s < HBK / 16; ++s) {
      const int ko = 16 * s + 8 * (lane >> 5);
      const f16x8 av = *reinterpret_cast<const f16x8*>(&As[32 * wave + (lane & 31)][ko]);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, *reinterpret_cast<const f16x8*>(&Bs[32 * t + (lane & 31)][ko]), acc[t], 0, 0, 0);
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
      if (m < M) epi(m, co, round_h(tot[t][r] + b));
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// The fp16 image of a layer that upload_layer has filled (same arguments): wt16 [Npad][Kpad16] with k = (ky * kw + kx) * cin_used + ci,
// zero beyond K / Cout, and the fp16-rounded biases as floats [Npad] (null when no part has one).  On an error L keeps its fp32 image only.
inline hipError_t upload_layer_h(ConvLayer& L, int cin, const std::vector<const float*>& w, const std::vector<const float*>& b, int cout_each) {
  const int parts = (int)w.size(), kh = L.kh, kw = L.kw, cin_used = L.cin_used;
  L.Kpad16 = (L.K + HBK - 1) / HBK * HBK;
  std::vector<_Float16> wt((size_t)L.Npad * L.Kpad16, (_Float16)0.f);
  std::vector<float> bias(L.Npad, 0.f);
  bool has_bias = false;
  for (int q = 0; q < parts; ++q)
    for (int o = 0; o < cout_each; ++o) {
      _Float16* row = wt.data() + (size_t)(q * cout_each + o) * L.Kpad16;
      for (int ci = 0; ci < cin_used; ++ci)
        for (int ky = 0; ky < kh; ++ky)
          for (int kx = 0; kx < kw; ++kx) row[(ky * kw + kx) * cin_used + ci] = (_Float16)w[q][(((size_t)o * cin + ci) * kh + ky) * kw + kx];
      if (b[q]) { bias[q * cout_each + o] = (float)(_Float16)b[q][o]; has_bias = true; }
    }
  hipError_t e = hipMalloc(&L.wt16, wt.size() * sizeof(_Float16));
  if (e == hipSuccess) e = hipMemcpy(L.wt16, wt.data(), wt.size() * sizeof(_Float16), hipMemcpyHostToDevice);
  if (e == hipSuccess && has_bias) e = hipMalloc(&L.bias16, bias.size() * 4);
  if (e == hipSuccess && has_bias) e = hipMemcpy(L.bias16, bias.data(), bias.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(L.wt16); (void)hipFree(L.bias16); L.wt16 = nullptr; L.bias16 = nullptr; }
  return e;
}

// conv_geom with the fp16 image in the place of the fp32 one.
inline ConvGeom conv_geom_h(const ConvLayer& L, const float* x, long long ldx, int B, int H, int W) {
  ConvGeom g = conv_geom(L, x, ldx, B, H, W);
  g.wt = reinterpret_cast<const float*>(L.wt16); g.bias = L.bias16; g.Kpad = L.Kpad16;
  return g;
}

}  // namespace
