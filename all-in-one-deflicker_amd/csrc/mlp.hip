// mlp.hip — register-chained fused coordinate-MLP kernels for gfx950 (forward, and backward dX chain).
//
// Replaces, for the stage-1 hot path, every `model_F_*(x)` module call and the dX half of
// `loss.backward()` of the reference (src/stage1_neural_atlas.py:174,181,230;
// src/models/stage_1/loss_utils.py:154-159,235,305,312; IMLP.forward in
// src/models/stage_1/implicit_neural_networks.py:62-80).
//
// One wavefront owns 32 rows.  A layer is evaluated transposed, Y^T = W * X^T, with
// v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chains): A = packed weight image read from LDS with one
// ds_read_b128 per four MFMA steps, B = the previous layer's output, which is ALREADY in the right
// registers (see "C-layout" in af_dev.h).  The four waves of a workgroup share the weight stream, which is
// double-buffered in LDS in 64 KB chunks by global_load_lds (one barrier per chunk, 16 K MFMA cycles apart).
// LDS: 2 x 64 KB weight buffers + 8 KB bias rows.  Registers: 128 (activations) + 128 (accumulators, AGPR) + 64
// (A fragments) -> 1 wave / SIMD.  One kernel carries the chains of all four nets (k_mlp_*_multi, below): a launch is a
// list of independent (net, row-tile range) parts.
#include "mlp_common.h"

template <class NS, bool TRAIN, bool HID>      // HID: see mlp_fwd_body_bf (mlpbf.hip)
AF_DEV void mlp_fwd_body(const FwdArgs& a, int wg, char* smem) {
  ChainRows cr;
  if (!chain_rows(a, wg, cr)) return;
  const int tid = cr.tid, wave = cr.wave, lane = cr.lane, j = cr.j, h = cr.h, tile = cr.tile, row = cr.row; const bool live = cr.live;

  using CB = ChunkBytes<NS>;
  ChunkStream cs{nullptr, smem, wave, 0, nullptr, 0};
  cs.start(a.wimg, tid);

  const int nl = a.nl;
  stage_bias(nl, a.bias, smem + AF_BIAS_LDS, tid);
  constexpr int NPE = NS::PEG > 0 ? NS::PEG * 4 : 4;
  float pe[NPE];            // first-layer / skip B operand (PE features, or xyt for the mapping nets)
  chain_input<NS, TRAIN>(a, pe, row, tile, j, h, live);

  const int a_off8 = (h * 256 + j) * 16;     // lane offset inside a Mpad=256 image chunk
  const int voff_t = (4 * h * 32 + j) * 4;
  f32x16 acc[8];
  float in[128];
  TileStore ts{af_rsrc(a.acts, 0), voff_t};

  auto relu_out = [&](int l) {               // acc -> in[] = relu(Z_l) = X_{l+1}; its stores are deferred
    // ReLU sign bits, 32 per word: element e = (T&1)*16 + r of word T>>1 sits at bit 31-e.  One v_alignbit
    // shifts the sign of (0 - v) in: set exactly when v > 0 (0 - (+0) = +0), no VCC round trip.
    uint32_t mk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int T = 0; T < 8; ++T)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = af_relu(acc[T][r]);
        in[T * 16 + r] = v;
        if (TRAIN) mk[T >> 1] = __builtin_amdgcn_alignbit(mk[T >> 1], __builtin_bit_cast(uint32_t, 0.f - v), 31);
      }
    if constexpr (TRAIN) {
      if (live) {
        u32x4 m4 = {mk[0], mk[1], mk[2], mk[3]};
        *(u32x4*)(a.masks + (((size_t)l * a.nt_stride + tile) * 64 + lane) * 4) = m4;
      }
      ts.r = af_rsrc_uniform(a.acts + ((size_t)l * a.nt_stride + tile) * AF_TILE_F, live ? AF_TILE_F * 4 : 0);
    }
    // the element-wise ops above are inline asm (af_relu / bf_mask_keep): gfx950 needs TWO wait states between a VALU write of a VGPR and an MFMA
    // reading it as SrcA / SrcB (tools/hazardprobe.hip); hipcc pads its own VALU ops and cannot see these.  Left to the scheduler they sink to just in
    // front of the output layer's MFMAs (a two-layer net has nothing else behind them): stale operands, a corrupted chain.  isa_check.py rule (d)
    // proves on every build that no such pair exists
    AF_ELEMWISE_FENCE();
  };
  auto hook_dma = [&](auto gi) { if constexpr (decltype(gi)::value < 8) cs.issue2(); };
  auto hook_dma_store = [&](auto gi) {
    if constexpr (decltype(gi)::value < 8) cs.issue2();
    if constexpr (TRAIN) ts.template part<decltype(gi)::value>(in);
  };

  // ---- layer 0
  {
    const char* buf = cs.next<CB::L0>();            // its barrier also publishes the bias rows
    init_bias(acc, smem + AF_BIAS_LDS, 0, h);
    mm_block<8, NS::K0G, 0, 4>(acc, pe, buf + a_off8, hook_dma);
  }
  relu_out(0);

  // ---- hidden layers 1 .. NL-2
  if constexpr (HID) {
  int l = 1;
  do {
    init_bias(acc, smem + AF_BIAS_LDS, l, h);
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 0, 4>(acc, in, buf + a_off8, hook_dma_store); }
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 32, 4>(acc, in, buf + a_off8, hook_dma); }
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 64, 4>(acc, in, buf + a_off8, hook_dma); }
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 96, 4>(acc, in, buf + a_off8, hook_dma); }
    if constexpr (NS::SKIP != 0) {
      if ((NS::SKIP >> l) & 1) { const char* buf = cs.next<CB::SKIP>(); mm_block<8, NS::PEG, 0, 4>(acc, pe, buf + a_off8, hook_dma); }
    }
    relu_out(l);
  } while (++l <= nl - 2);
  }

  // ---- output layer (1..3 real outputs), tanh (chain_out_layer, mlp_common.h)
  chain_out_layer<NS, TRAIN>(a, nl, cs.next_rt(CB::last_bytes(nl)), smem + AF_BIAS_LDS + (nl - 1) * AF_HID * 4, in, pe, ts, row, lane, h, live);
}

// ------------------------------------------------------------------------------------------------
// Backward dX chain: dZ_{l-1} = (W_l^T dZ_l) . relu'(Z_{l-1}); writes every dZ_l in T-layout for the dW
// GEMMs (dw.hip).  For the atlas net the chain continues through layer 0 into the positional encoding
// and accumulates dL/d(uv) onto the mapping net's output gradient (the detached skip inputs carry no
// gradient: implicit_neural_networks.py:69).
template <class NS>
AF_DEV void mlp_bwd_body(const BwdArgs& a, int wg, char* smem) {
  ChainRows cr;
  if (!chain_rows(a, wg, cr)) return;
  const int tid = cr.tid, wave = cr.wave, lane = cr.lane, j = cr.j, h = cr.h, tile = cr.tile, row = cr.row; const bool live = cr.live;

  using CB = ChunkBytes<NS>;
  ChunkStream cs{nullptr, smem, wave, 0, nullptr, 0};
  cs.start(a.wimg, tid);
  const int nl = a.nl;

  float dzl[4];
  chain_seed<NS>(a, dzl, row, tile, j, h, live);

  const int a_off8 = (h * 256 + j) * 16;
  const int voff_t = (4 * h * 32 + j) * 4;
  f32x16 acc[8];
  float in[128];
  TileStore ts{af_rsrc(a.dz, 0), voff_t};

  auto mask_out = [&](int l) {      // acc = dX_l; mask with sign bits of X_l (masks[l-1]) -> in[] = dZ_{l-1}
    const u32x4 m4 = *(const u32x4*)(a.masks + (((size_t)(l - 1) * a.nt_stride + tile) * 64 + lane) * 4);
    const uint32_t mk[4] = {m4[0], m4[1], m4[2], m4[3]};
#pragma unroll
    for (int T = 0; T < 8; ++T)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        in[T * 16 + r] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, (float)acc[T][r]) &
                                                   (uint32_t)__builtin_amdgcn_sbfe((int)mk[T >> 1], 31 - ((T & 1) * 16 + r), 1));
    ts.r = af_rsrc_uniform(a.dz + ((size_t)(l - 1) * a.nt_stride + tile) * AF_TILE_F, live ? AF_TILE_F * 4 : 0);
    // the element-wise ops above are inline asm (af_relu / bf_mask_keep): gfx950 needs TWO wait states between a VALU write of a VGPR and an MFMA
    // reading it as SrcA / SrcB (tools/hazardprobe.hip); hipcc pads its own VALU ops and cannot see these.  Left to the scheduler they sink to just in
    // front of the output layer's MFMAs (a two-layer net has nothing else behind them): stale operands, a corrupted chain.  isa_check.py rule (d)
    // proves on every build that no such pair exists
    AF_ELEMWISE_FENCE();
  };
  auto hook_dma = [&](auto gi) { if constexpr (decltype(gi)::value < 8) cs.issue2(); };
  auto hook_dma_store = [&](auto gi) { if constexpr (decltype(gi)::value < 8) cs.issue2(); ts.template part<decltype(gi)::value>(in); };

  // ---- output layer: K = 8 (one group), only p < OUT non-zero
  { const char* buf = cs.next<CB::BLAST>(); mm_block<8, 1, 0, NS::OUT, true>(acc, dzl, buf + a_off8, hook_dma); }
  mask_out(nl - 1);

  for (int l = nl - 2; l >= 1; --l) {
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 0, 4, true>(acc, in, buf + a_off8, hook_dma_store); }
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 32, 4>(acc, in, buf + a_off8, hook_dma); }
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 64, 4>(acc, in, buf + a_off8, hook_dma); }
    { const char* buf = cs.next<CB::HID>(); mm_block<8, 8, 96, 4>(acc, in, buf + a_off8, hook_dma); }
    mask_out(l);
  }

  if constexpr (NS::DX0) {
    // dPE = W_0^T dZ_0  (M = 64 padded PE features, K = 256), then chain through sin/cos to the 2-D input
    f32x16 acc2[2];
    { const char* buf = cs.next<CB::BL0>(); mm_block<2, 32, 0, 4, true>(acc2, in, buf + (h * 64 + j) * 16, hook_dma_store); }
    chain_dpe_to_uv<NS>(a, acc2, row, tile, j, h, live);
  } else {
    ts.all(in);      // dZ_0 of a net whose input needs no gradient: nothing left to hide the stores behind
  }
}

// ------------------------------------------------------------------------------------------------
// The multi-part kernels (chains_fwd_multi, mlp_common.h)
struct Fp32Chains {
  template <class NS, bool TRAIN, bool HID> static AF_DEV void fwd(const FwdArgs& a, int wg, char* smem) { mlp_fwd_body<NS, TRAIN, HID>(a, wg, smem); }
  template <class NS> static AF_DEV void bwd(const BwdArgs& a, int wg, char* smem) { mlp_bwd_body<NS>(a, wg, smem); }
};

template <bool TRAIN>
__global__ __launch_bounds__(256, 1) void k_mlp_fwd_multi(MultiFwd m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  AF_STAMP(m, 0);
  chains_fwd_multi<Fp32Chains, TRAIN>(m, smem);
  AF_STAMP(m, 1);
}

__global__ __launch_bounds__(256, 1) void k_mlp_bwd_multi(MultiBwd m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  AF_STAMP(m, 0);
  chains_bwd_multi<Fp32Chains>(m, smem);
  AF_STAMP(m, 1);
}

extern "C" int af_launch_fwd_multi(MultiFwd* m, int train, hipStream_t s) {
  const int tot = multi_grid(*m);
  if (tot <= 0) return 0;
  const size_t lds = AF_LDS_BYTES;
  if (train) hipLaunchKernelGGL((k_mlp_fwd_multi<true>), dim3(tot), dim3(256), lds, s, *m);
  else       hipLaunchKernelGGL((k_mlp_fwd_multi<false>), dim3(tot), dim3(256), lds, s, *m);
  return (int)hipGetLastError();
}

extern "C" int af_launch_bwd_multi(MultiBwd* m, hipStream_t s) {
  const int tot = multi_grid(*m);
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(k_mlp_bwd_multi, dim3(tot), dim3(256), AF_LDS_BYTES, s, *m);
  return (int)hipGetLastError();
}

extern "C" int af_mlp_chunk_bytes(int net, int which, int nl) { return chunk_bytes<ChunkBytes>(net, which, nl); }
extern "C" int af_mlp_init() { return lds_opt_in(AF_LDS_BYTES, k_mlp_fwd_multi<true>, k_mlp_fwd_multi<false>, k_mlp_bwd_multi); }     // 128 KB dynamic LDS
