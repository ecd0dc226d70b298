// mlp_common.h — what the chains share: net shapes, the compile-time chunk plan, the LDS weight-chunk stream, the bias staging and the
// one-instruction ReLU (also used by the 16-row chains of mlp16.hip), and the scaffold of the three 32-row chain families — fp32 MFMA
// (mlp.hip), bf16x6 (mlpbf.hip), f16x3 (mlphf.hip): the row prologue, the input stage (positional encoding in the reference's feature
// order), the tanh output layer, the backward seed gradient, the dPE -> d(uv) tail, the multi-part dispatch, and on the host the launch
// grid, the chunk-size query and the LDS opt-in.  Each piece exists once, so the families agree on it by construction.  What is NOT
// here: the 256x256 hidden-layer products (k-steps, operand splits, LDS streams, publishes), hand-scheduled per arithmetic in each
// family's own file.
#pragma once
#include <utility>

#include "af_dev.h"

#ifndef AF_ABL
#define AF_ABL 0   // tools/ablate.hip timing probes: bit0 no tile stores, bit1 no LDS-DMA, bit2 no barriers, bit3 no LDS fragment reads, bit4 no
                   // sched_barrier, bit5 no operand split, bit6 only wave 0 issues the LDS-DMA, bit8 atlas PE without sin / cos, bit9 with sincosf
#endif

// NL is the SHIPPED layer count (config_flow_100.json); the kernels take the actual count from FwdArgs::nl / BwdArgs::nl.
struct NsMap1  { static constexpr int NL = 6, IN = AF_IN_XYT, K0G = 1, PEG = 0, OUT = 2; static constexpr unsigned SKIP = 0;                       static constexpr bool DX0 = false; };
struct NsMap2  { static constexpr int NL = 4, IN = AF_IN_XYT, K0G = 1, PEG = 0, OUT = 2; static constexpr unsigned SKIP = 0;                       static constexpr bool DX0 = false; };
struct NsAtlas { static constexpr int NL = 8, IN = AF_IN_PE2, K0G = 5, PEG = 5, OUT = 3; static constexpr unsigned SKIP = (1u << 4) | (1u << 7);   static constexpr bool DX0 = true;  };
struct NsMapPe { static constexpr int NL = 6, IN = AF_IN_PE3, K0G = 4, PEG = 4, OUT = 2; static constexpr unsigned SKIP = 0;                       static constexpr bool DX0 = false; };
struct NsAlpha { static constexpr int NL = 8, IN = AF_IN_PE3, K0G = 4, PEG = 4, OUT = 1; static constexpr unsigned SKIP = 0;                       static constexpr bool DX0 = false; };

// Byte sizes of the weight chunks, in stream order (host.hip plan_images lays the images out contiguously in
// exactly this order, so a chunk's address is the previous chunk's address plus its size: no table lookups
// inside the kernels).  A k-group of an Mpad-row image is 2*Mpad*16 bytes; sizes round up to 4 KB.
constexpr int af_round4k(int b) { return (b + 4095) / 4096 * 4096; }
template <class NS> struct ChunkBytes {
  static constexpr int L0   = af_round4k(NS::K0G * 2 * AF_HID * 16);                                            // forward layer 0
  static constexpr int HID  = 8 * 2 * AF_HID * 16;                                                            // a quarter of a 256x256 layer = 64 KB
  static constexpr int SKIP = af_round4k(NS::PEG * 2 * AF_HID * 16);                                            // PE columns of a skip layer
  static constexpr int LASTN = af_round4k(32 * 2 * 4 * 16);                                                   // forward output layer (Mpad 4) ...
  static constexpr int LASTS = af_round4k((32 + NS::PEG) * 2 * 4 * 16);                                       // ... with the PE columns of a skip-concat in front of it
  static constexpr bool out_skip(int nl) { return ((NS::SKIP >> (nl - 1)) & 1u) != 0; }                       // implicit_neural_networks.py:40-44: layer i in skip_layers, i == num_layers - 1
  static constexpr int last_bytes(int nl) { return out_skip(nl) ? LASTS : LASTN; }
  static constexpr int LAST = last_bytes(NS::NL);
  static constexpr int BLAST = 2 * AF_HID * 16;                                                               // backward output layer: one k-group
  static constexpr int BL0  = 32 * 2 * 64 * 16;                                                               // backward layer 0 (Mpad 64 PE slots)
  static constexpr int BL0C = BL0;                                                                            // the chunk it streams in: all of it
};
static_assert(ChunkBytes<NsMap1>::HID == AF_CHUNK_MAX && ChunkBytes<NsAtlas>::BL0 == AF_CHUNK_MAX, "chunk = LDS buffer");
// The chunks of the 16-bit chains (mlpbf.hip: SLOT = 48 KB, mlphf.hip: 64 KB): the fp32 blocks of ChunkBytes, a hidden 256x256 product
// in chunks of one LDS slot, the backward layer-0 block in two halves.
template <class NS, int SLOT> struct ChunkBytes16 {
  using F = ChunkBytes<NS>;
  static_assert(F::L0 <= SLOT && F::SKIP <= SLOT, "fp32 blocks must fit a slot");
  static constexpr int L0 = F::L0, SKIP = F::SKIP, LAST = F::LAST, BLAST = F::BLAST;
  static constexpr int HID = SLOT;                       // x8 (bf16x6) or x4 (f16x3) per hidden layer
  static constexpr int BL0C = 16 * 2 * 64 * 16;          // half of the backward layer-0 block (Mpad 64): two chunks of 32 KB
  static constexpr bool out_skip(int nl) { return F::out_skip(nl); }
  static constexpr int last_bytes(int nl) { return F::last_bytes(nl); }
};

template <int G> struct GIdx { static constexpr int value = G; };

// Double-buffered LDS stream of weight chunks shared by the four waves of the workgroup.  Every stage moves
// a full 64 KB buffer (16 x 1 KB per wave) whatever the chunk's real size — the image buffers are padded so
// the over-read stays in bounds — which keeps the issue sites branch-free: two LDS-DMA instructions per
// k-group ride in the shadow of that group's 32 MFMAs.
struct ChunkStream {
  const char* src;                                     // this lane's 16-B column of the chunk being staged
  char* smem; int wave, cidx;
  char* p_dst; int p_it;                               // chunk being staged (issued incrementally)
  AF_DEV void begin_stage(int c) { p_dst = smem + (c & 1) * AF_CHUNK_MAX + wave * 1024; p_it = 0; }
  AF_DEV void issue2() {
    if constexpr (AF_ABL & 2) { p_it += 2; return; }
    af_glds16(src + p_it * 4096, p_dst + p_it * 4096);
    af_glds16(src + p_it * 4096 + 4096, p_dst + p_it * 4096 + 4096);
    p_it += 2;
  }
  AF_DEV void start(const void* img, int tid) { src = (const char*)img + tid * 16; cidx = 0; begin_stage(0); }
  // Make chunk `cidx` (BYTES long) visible to every wave (and know every wave is done with chunk cidx-1), then
  // arm the staging of chunk cidx+1 — which starts BYTES further on — into the buffer chunk cidx-1 used.
  // Returns the LDS base of chunk cidx.  After the last chunk the stream stages 64 KB of whatever follows
  // (the image buffers are padded for that) into the idle buffer: harmless, and the issue sites stay branch-free.
  template <int BYTES> AF_DEV const char* next() { return next_rt(BYTES); }
  AF_DEV const char* next_rt(int BYTES) {
    while (p_it < 16) issue2();
    if constexpr (!(AF_ABL & 4)) { af_wait_vm0(); __syncthreads(); }
    const int cur = cidx;
    cidx = cur + 1;
    src += BYTES;
    begin_stage(cidx);
    return smem + (cur & 1) * AF_CHUNK_MAX;
  }
};

// max(z, 0) as ONE v_max_f32 (the C-level fmaxf adds a canonicalising v_max in front).  v_max_f32 returns 0 for a NaN input
// where torch.relu propagates it: a NaN pre-activation needs a non-finite parameter or input (Adam's steps are bounded by
// lr), and k_adam raises AF_ENAN for any non-finite parameter (elem.hip), so the condition is reported, not healed silently.
AF_DEV float af_relu(float z) { float v; asm("v_max_f32 %0, 0, %1" : "=v"(v) : "v"(z)); return v; }
#ifdef AF_NO_ELEMWISE_FENCE      // experiment: the build that corrupted two-layer nets in round 3 (tools/experiments/README.md, "element-wise fence")
#define AF_ELEMWISE_FENCE() do { } while (0)
#else
#define AF_ELEMWISE_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

// Accumulator initialisation = bias.  The net's padded bias rows ([NL][256] floats, <= 8 KB) are copied once per
// workgroup into LDS behind the two weight buffers: 32 ds_read_b128 per layer cost a fraction of the 32 VMEM loads
// they replace (each VMEM instruction steals ~40 cycles of MFMA issue from the only wave of its SIMD).
#define AF_BIAS_LDS (2 * AF_CHUNK_MAX)          // byte offset of the bias rows in dynamic LDS
#define AF_LDS_BYTES (2 * AF_CHUNK_MAX + AF_MAX_LAYERS * AF_HID * 4)
// Row tiles a launch really has: the static count, or — when the batch's flow-match rows are compacted on the device
// (k_prep, elem.hip) — the tiles up to the last live row.
template <class Args> AF_DEV int live_tiles(const Args& a) {
  if (!a.live_rows) return a.NT;
  const int nt = (a.live_base + *a.live_rows + 31) >> 5;
  return nt < a.NT ? nt : a.NT;
}

AF_DEV void stage_bias(int nl, const float* bias, char* bias_lds, int tid) {
  float* dst = (float*)bias_lds;
  for (int i = 0; i < nl; ++i) dst[i * AF_HID + tid] = bias[i * AF_HID + tid];     // 256 threads x nl rows; visible after the first barrier
}

// ---- blocks shared by the fp32 chains (mlp.hip) and the bf16x6 chains (mlpbf.hip) ----------------------------------------
#ifndef AF_SGB
#define AF_SGB 1     // explicit MFMA / memory-instruction interleave (sched_group_barrier) inside every k-group
#endif
#ifndef AF_AFRAG
#define AF_AFRAG 1   // A fragments in AGPRs (see lds_frag)
#endif

// One A fragment (four consecutive k of one output row) from the LDS weight image, pinned to the accumulator half of
// the register file: ds_read_b128 writes AGPRs directly and the MFMA takes its A operand from there, so the 64
// fragment registers do not compete with the 128 activation registers for the 256 architectural VGPRs (with all of
// them in VGPRs the allocator is full and sinks every group's reads to the end of the previous group, where their
// latency is exposed behind an s_waitcnt lgkmcnt(0)).
AF_DEV f32x4 lds_frag(const char* p) { return *(const f32x4*)p; }
// The pin sits at the fragment's first USE (top of its k-group), not at the load: the compiler's s_waitcnt for the
// read lands there too, a whole group (32 MFMAs) after the read was issued.
AF_DEV void pin_acc(f32x4& v) {
#if AF_AFRAG
  asm("" : "+a"(v));
#endif
}

// acc[T] += A(image in LDS) * b[B0 + 4*g + p]  for NG k-groups; a_lds already includes the lane offset
// (h*MPAD + j)*16.  NP < 4 skips reduction indices that are structurally zero.  hook(g) is called once per
// k-group right after that group's A-fragment reads were issued: work placed there (LDS-DMA issue of the
// next weight chunk, stores of the previous layer's activations) runs in the shadow of the group's MFMAs
// instead of in front of an empty matrix pipe.
template <int MT, int NG, int B0, int NP, bool ZI, int NB, class Hook, int... Gs>
AF_DEV void mm_block_impl(f32x16 (&acc)[MT], const float (&b)[NB], const char* a_lds, Hook& hook, std::integer_sequence<int, Gs...>) {
  constexpr int MPAD = MT * 32;
  f32x4 a[2][MT];
#pragma unroll
  for (int T = 0; T < MT; ++T) a[0][T] = lds_frag(a_lds + T * 32 * 16);
  if constexpr (AF_ABL & 8) {
#pragma unroll
    for (int T = 0; T < MT; ++T) a[1][T] = a[0][T];
  }
  auto step = [&](auto gi) {
    constexpr int g = decltype(gi)::value;
#pragma unroll
    for (int T = 0; T < MT; ++T) pin_acc(a[g & 1][T]);
    if constexpr (g + 1 < NG && !(AF_ABL & 8)) {
#pragma unroll
      for (int T = 0; T < MT; ++T) a[(g + 1) & 1][T] = lds_frag(a_lds + ((g + 1) * 2 * MPAD + 32 * T) * 16);
    }
    hook(gi);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int T = 0; T < MT; ++T) {
        if constexpr (ZI && g == 0) {
          if (p == 0) { const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][T][0], b[B0], z, 0, 0, 0); continue; }
        }
        acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g & 1][T][p], b[B0 + g * 4 + p], acc[T], 0, 0, 0);
      }
    }
#if AF_SGB
    // Issue order inside the group: one LDS fragment read and one VMEM instruction (LDS-DMA piece / tile store) behind
    // each MFMA, so that every memory instruction issues in the shadow of a 64-cycle MFMA instead of in one burst
    // behind which the matrix pipe drains (hipcc's own order: 24 MFMAs, then 8 reads + 2 DMA + up to 16 stores).
#pragma unroll
    for (int i = 0; i < NP * MT; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
    }
#endif
    if constexpr (!(AF_ABL & 16)) __builtin_amdgcn_sched_barrier(0);     // keep each group's DMA / stores inside its own MFMA shadow
  };
  (step(GIdx<Gs>{}), ...);
}
// ZI: the accumulators start at zero — the first MFMA of each takes an inline-constant 0 as C instead of
// a previously zeroed register block (saves MT*16 v_accvgpr_write per layer in the backward chain).
template <int MT, int NG, int B0, int NP, bool ZI = false, int NB, class Hook>
AF_DEV void mm_block(f32x16 (&acc)[MT], const float (&b)[NB], const char* a_lds, Hook&& hook) {
  mm_block_impl<MT, NG, B0, NP, ZI>(acc, b, a_lds, hook, std::make_integer_sequence<int, NG>{});
}

AF_DEV void init_bias(f32x16 (&acc)[8], const char* bias_lds /* the staged [NL][256] rows */, int layer, int h) {
  const char* b = bias_lds + (layer * AF_HID + 4 * h) * 4;
#pragma unroll
  for (int T = 0; T < 8; ++T) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b4 = *(const f32x4*)(b + (32 * T + 8 * q) * 4);
      acc[T][q * 4 + 0] = b4[0]; acc[T][q * 4 + 1] = b4[1]; acc[T][q * 4 + 2] = b4[2]; acc[T][q * 4 + 3] = b4[3];
    }
  }
}

// Store 1/8 (feature tile T) of a C-layout block (reg = 16T+4q+p <-> feature 32T+8q+4h+p) into a T-layout
// tile [256][32].
template <int T>
AF_DEV void store_tile_part(const float (&v)[128], __amdgpu_buffer_rsrc_t r, int voff) {
  // the 128-B steps between p = 0..3 ride in the instruction's immediate offset: one soffset per (T, q)
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) af_bs32_tile(v[T * 16 + rr], r, voff + (rr & 3) * 128, (32 * T + 8 * (rr >> 2)) * 128);
}

// Deferred stores of one 32x256 block: one feature tile per k-group of the following GEMM block.
// A dead wave (tile past the end) carries a zero-length buffer descriptor: its stores are dropped by the
// hardware bounds check, so the store sites need no branch.
struct TileStore {
  __amdgpu_buffer_rsrc_t r; int voff;
  template <int G> AF_DEV void part(const float (&v)[128]) const { if constexpr (G < 8 && !(AF_ABL & 1)) store_tile_part<G>(v, r, voff); }
  AF_DEV void all(const float (&v)[128]) const {      // the whole block at once, where no GEMM is left to hide the stores behind
    part<0>(v); part<1>(v); part<2>(v); part<3>(v); part<4>(v); part<5>(v); part<6>(v); part<7>(v);
  }
};


// ---- device scaffold of the 32-row chain families (mlp.hip, mlpbf.hip, mlphf.hip) -----------------------------------------------------
// The rows of a chain: wave `wave` of workgroup wg owns row tile `tile`, lane (j, h) row j of it.  A wave past the last live tile takes that
// tile (live = false: its stores are masked or dropped).  false: the workgroup has no rows this iteration — the caller returns (uniform:
// before any barrier).
struct ChainRows { int tid, wave, lane, j, h, tile, row; bool live; };
template <class Args> AF_DEV bool chain_rows(const Args& a, int wg, ChainRows& r) {
  r.tid = threadIdx.x;
  r.wave = __builtin_amdgcn_readfirstlane(r.tid >> 6);
  r.lane = r.tid & 63; r.j = r.lane & 31; r.h = r.lane >> 5;
  r.tile = a.tile0 + wg * 4 + r.wave;
  const int NT = live_tiles(a);
  if (a.tile0 + wg * 4 >= NT) return false;
  r.live = r.tile < NT;
  if (!r.live) r.tile = NT - 1;
  r.row = r.tile * 32 + r.j;
  return true;
}

// First-layer / skip B operand of a row: the xyt pass-through of the mapping nets, or the positional encoding in the reference's feature
// order (accurate sinf / cosf); a training forward also stores the PE features as a T-layout tile [64][32] for the dW GEMMs.
template <class NS, bool TRAIN, int NPE>
AF_DEV void chain_input(const FwdArgs& a, float (&pe)[NPE], int row, int tile, int j, int h, bool live) {
  const f32x4 v = row < a.split_row ? *(const f32x4*)(a.in + (size_t)row * 4) : *(const f32x4*)(a.in1 + (size_t)(row - a.split_row) * 4);
  if constexpr (NS::IN == AF_IN_XYT) {
#pragma unroll
    for (int p = 0; p < 4; ++p) pe[p] = (h == 0 && p < 3) ? v[p] : 0.f;
  } else if constexpr (NS::IN == AF_IN_PE2) {
    const float sh = row < a.split_row ? a.in_shift0 : a.in_shift1;
    const float x0 = v[0] * a.in_scale + sh, x1 = v[1] * a.in_scale + sh;
#pragma unroll
    for (int g = 0; g < 5; ++g) {
      const float b = h ? __builtin_ldexpf(3.14159265358979323846f, 2 * g + 1) : __builtin_ldexpf(3.14159265358979323846f, 2 * g);
      const float p0 = x0 * b, p1 = x1 * b;
      if constexpr ((AF_ABL & 256) != 0) { pe[g * 4 + 0] = p0; pe[g * 4 + 1] = p1; pe[g * 4 + 2] = -p0; pe[g * 4 + 3] = -p1; }      // timing probe: no sin / cos
      else if constexpr ((AF_ABL & 512) != 0) { sincosf(p0, &pe[g * 4 + 0], &pe[g * 4 + 2]); sincosf(p1, &pe[g * 4 + 1], &pe[g * 4 + 3]); }
      else { pe[g * 4 + 0] = sinf(p0); pe[g * 4 + 1] = sinf(p1); pe[g * 4 + 2] = cosf(p0); pe[g * 4 + 3] = cosf(p1); }
    }
  } else {   // AF_IN_PE3: lane half h owns k in {2h, 2h+1} (+ sin/cos triple of k = 4)
    const float x[3] = {v[0], v[1], v[2]};
    const float bA = __builtin_ldexpf(3.14159265358979323846f, 2 * h), bB = __builtin_ldexpf(3.14159265358979323846f, 2 * h + 1);
    const float b4 = __builtin_ldexpf(3.14159265358979323846f, 4);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      pe[d] = sinf(x[d] * bA); pe[3 + d] = cosf(x[d] * bA);
      pe[6 + d] = sinf(x[d] * bB); pe[9 + d] = cosf(x[d] * bB);
      pe[12 + d] = h ? cosf(x[d] * b4) : sinf(x[d] * b4);
    }
    pe[15] = 0.f;
  }
  if constexpr (TRAIN && NS::PEG > 0) {
    if (live) {   // PE features in reference feature order, T-layout [64][32], for the dW GEMMs
      const auto r = af_rsrc_uniform(a.pe_tile + (size_t)tile * 64 * 32, 64 * 32 * 4);
      if constexpr (NS::IN == AF_IN_PE2) {
#pragma unroll
        for (int g = 0; g < 5; ++g)
#pragma unroll
          for (int p = 0; p < 4; ++p) af_bs32(pe[g * 4 + p], r, (4 * h * 32 + j) * 4, (8 * g + p) * 128);
      } else {
#pragma unroll
        for (int rho = 0; rho < 15; ++rho) {
          if (rho < 12) af_bs32(pe[rho], r, (12 * h * 32 + j) * 4, rho * 128);
          else          af_bs32(pe[rho], r, (3 * h * 32 + j) * 4, (24 + rho - 12) * 128);
        }
      }
    }
  }
}

// Forward output layer (1..3 real outputs), tanh; buf: the layer's chunk in LDS, bias_row: its staged bias row.  A training chain first stores
// the last hidden layer's activation tile.  A 32-wide MFMA tile would spend 128+ full-rate MFMAs on 2 or 3 useful rows (3 % of the whole
// chain); v_mfma_f32_4x4x1_16B_f32 does the same dot products in 4-output blocks: lane l = block (l >> 2) = (k-half h, row quad), column
// l & 3 = row within the quad, so the B operand is the activation register as it stands (lane = row, register = feature 8g+4h+p) and the A
// operand is W[l & 3][8g+4h+p] — the usual packed image with Mpad = 4.  Each k-half accumulates its own partial; one shuffle adds them.
template <class NS, bool TRAIN, int NPE>
AF_DEV void chain_out_layer(const FwdArgs& a, int nl, const char* buf, const char* bias_row, const float (&in)[128], const float (&pe)[NPE],
                            const TileStore& ts, int row, int lane, int h, bool live) {
  if constexpr (TRAIN) ts.all(in);
  const char* al = buf + (h * 4 + (lane & 3)) * 16;
  f32x4 o4[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) o4[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < 32; ++g) {
    const f32x4 w = *(const f32x4*)(al + g * 2 * 4 * 16);
#pragma unroll
    for (int p = 0; p < 4; ++p) o4[p] = __builtin_amdgcn_mfma_f32_4x4x1f32(w[p], in[4 * g + p], o4[p], 0, 0, 0);
  }
  if constexpr (NS::SKIP != 0) {
    if (ChunkBytes<NS>::out_skip(nl)) {
#pragma unroll
      for (int g = 0; g < NS::PEG; ++g) {
        const f32x4 w = *(const f32x4*)(al + (32 + g) * 2 * 4 * 16);
#pragma unroll
        for (int p = 0; p < 4; ++p) o4[p] = __builtin_amdgcn_mfma_f32_4x4x1f32(w[p], pe[4 * g + p], o4[p], 0, 0, 0);
      }
    }
  }
  const f32x4 bias = *(const f32x4*)bias_row;
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float z = (o4[0][i] + o4[1][i]) + (o4[2][i] + o4[3][i]);
    z += __shfl_xor(z, 32);
    o[i] = i < NS::OUT ? tanhf(z + bias[i]) : 0.f;
  }
  if (live && h == 0) *(f32x4*)(a.out + (size_t)row * 4) = o;
}

// Seed of the backward chain through the tanh head: dZ_last = dout . (1 - o^2), also stored for the output layer's dW.
template <class NS>
AF_DEV void chain_seed(const BwdArgs& a, float (&dzl)[4], int row, int tile, int j, int h, bool live) {
  const f32x4 o = *(const f32x4*)(a.out + (size_t)row * 4);
  const f32x4 d = *(const f32x4*)(a.dout + (size_t)row * 4);
#pragma unroll
  for (int p = 0; p < 4; ++p) dzl[p] = (h == 0 && p < NS::OUT) ? d[p] * (1.f - o[p] * o[p]) : 0.f;
  if (live && h == 0) {
#pragma unroll
    for (int p = 0; p < NS::OUT; ++p) a.dz_last[((size_t)tile * 32 + p) * 32 + j] = dzl[p];
  }
}

// The atlas net's input gradient: dPE = W_0^T dZ_0 (acc2: M = 64 padded PE features) through sin / cos (the PE tile the forward stored) to
// the 2-D input, accumulated onto the mapping net's output gradient (the detached skip inputs carry none: implicit_neural_networks.py:69).
template <class NS>
AF_DEV void chain_dpe_to_uv(const BwdArgs& a, const f32x16 (&acc2)[2], int row, int tile, int j, int h, bool live) {
  static_assert(NS::IN == AF_IN_PE2, "input gradient is only needed for the atlas net");
  const auto r = af_rsrc_uniform(a.pe_tile + (size_t)tile * 64 * 32, 64 * 32 * 4);
  float dx0 = 0.f, dx1 = 0.f;
#pragma unroll
  for (int g = 0; g < 5; ++g) {
    float pv[4], dv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      pv[p] = af_bl32(r, (4 * h * 32 + j) * 4, (8 * g + p) * 128);
      dv[p] = acc2[g >> 2][(g & 3) * 4 + p];
    }
    const float b = h ? __builtin_ldexpf(3.14159265358979323846f, 2 * g + 1) : __builtin_ldexpf(3.14159265358979323846f, 2 * g);
    dx0 += b * (pv[2] * dv[0] - pv[0] * dv[2]);
    dx1 += b * (pv[3] * dv[1] - pv[1] * dv[3]);
  }
  dx0 += __shfl_xor(dx0, 32);
  dx1 += __shfl_xor(dx1, 32);
  if (live && h == 0 && row < a.nrows) {
    float* dst = row < a.split_row ? a.din0 + (size_t)row * 4 : a.din1 + (size_t)(row - a.split_row) * 4;
    dst[0] += a.din_scale * dx0;
    dst[1] += a.din_scale * dx1;
  }
}

// One launch, up to AF_MAX_NETS row-tile ranges of different nets back to back ("parts").  A workgroup finds its part by its index and runs
// that net's chain.  Packing several nets (or the odd last round of one net next to another net) into one grid removes the idle tail of
// separate launches: 2188 row tiles of the 7-segment mapping batch are 2.14 rounds of the 1024 SIMDs but cost 3 as a launch of their own.
// Parts of one launch must be independent of each other (the host orders dependent work across launches).
// Chains: the family's bodies as template <class NS, bool TRAIN, bool HID> fwd(...) and template <class NS> bwd(...); HID: the net has
// hidden 256 -> 256 layers (nl >= 3) — a two-layer net takes the copy without the layer loop (see mlp_fwd_body_bf).
template <class Chains, class NS, bool TRAIN> AF_DEV void chains_fwd_part(const FwdArgs& a, int wg, char* smem) {
  if (a.nl > 2) Chains::template fwd<NS, TRAIN, true>(a, wg, smem); else Chains::template fwd<NS, TRAIN, false>(a, wg, smem);
}
template <class Chains, bool TRAIN>
AF_DEV void chains_fwd_multi(const MultiFwd& m, char* smem) {
  int s = 0, base = 0;
  const int wg = blockIdx.x;
  while (s + 1 < m.n && wg >= m.wg_end[s]) { base = m.wg_end[s]; ++s; }
  switch (m.net[s]) {
    case AF_NET_MAP1:    chains_fwd_part<Chains, NsMap1, TRAIN>(m.a[s], wg - base, smem); break;
    case AF_NET_MAP2:    chains_fwd_part<Chains, NsMap2, TRAIN>(m.a[s], wg - base, smem); break;
    case AF_NET_ATLAS:   chains_fwd_part<Chains, NsAtlas, TRAIN>(m.a[s], wg - base, smem); break;
    case AF_KIND_MAP_PE: chains_fwd_part<Chains, NsMapPe, TRAIN>(m.a[s], wg - base, smem); break;
    default:             chains_fwd_part<Chains, NsAlpha, TRAIN>(m.a[s], wg - base, smem); break;
  }
}
template <class Chains>
AF_DEV void chains_bwd_multi(const MultiBwd& m, char* smem) {
  int s = 0, base = 0;
  const int wg = blockIdx.x;
  while (s + 1 < m.n && wg >= m.wg_end[s]) { base = m.wg_end[s]; ++s; }
  switch (m.net[s]) {
    case AF_NET_MAP1:    Chains::template bwd<NsMap1>(m.a[s], wg - base, smem); break;
    case AF_NET_MAP2:    Chains::template bwd<NsMap2>(m.a[s], wg - base, smem); break;
    case AF_NET_ATLAS:   Chains::template bwd<NsAtlas>(m.a[s], wg - base, smem); break;
    case AF_KIND_MAP_PE: Chains::template bwd<NsMapPe>(m.a[s], wg - base, smem); break;
    default:             Chains::template bwd<NsAlpha>(m.a[s], wg - base, smem); break;
  }
}

// ---- host side of the three chain families -----------------------------------------------------------------------------------------
// Host side of a multi-part launch: fills m.wg_end[] from the parts' tile ranges (four row tiles per workgroup), returns the grid size.
template <class Multi> inline int multi_grid(Multi& m) {
  int tot = 0;
  for (int i = 0; i < m.n; ++i) { tot += (m.a[i].NT - m.a[i].tile0 + 3) / 4; m.wg_end[i] = tot; }
  return tot;
}

// The chunk sizes a family's kernels assume (CB: ChunkBytes, or the family's ChunkBytes16), for the host planner to check its layout
// against: which = 0 fwd layer 0, 1 hidden-layer chunk, 2 skip columns, 3 fwd output layer, 4 bwd output layer, 5 bwd layer-0 chunk;
// nl: layers of the net (the output-layer chunk is longer when it carries skip columns).
template <template <class> class CB> inline int chunk_bytes(int net, int which, int nl) {
  auto pick = [&](auto ns) -> int {
    using C = CB<decltype(ns)>;
    const int v[6] = {C::L0, C::HID, C::SKIP, C::last_bytes(nl), C::BLAST, C::BL0C};
    return which >= 0 && which < 6 ? v[which] : -1;
  };
  switch (net) {
    case AF_NET_MAP1:    return pick(NsMap1{});
    case AF_NET_MAP2:    return pick(NsMap2{});
    case AF_NET_ATLAS:   return pick(NsAtlas{});
    case AF_NET_ALPHA:   return pick(NsAlpha{});
    case AF_KIND_MAP_PE: return pick(NsMapPe{});
    default: return -1;
  }
}

// Opt kernels in to `bytes` of dynamic LDS (beyond the default 64 KB); returns the last failure, if any.
template <class... K> inline int lds_opt_in(int bytes, K... kernels) {
  hipError_t e = hipSuccess;
  for (const void* k : {(const void*)kernels...}) { const hipError_t r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); if (r != hipSuccess) e = r; }
  return (int)e;
}
