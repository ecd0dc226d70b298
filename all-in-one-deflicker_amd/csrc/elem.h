// elem.h — argument blocks of the non-GEMM kernels (see elem.hip) and, under each, the host entry point that launches it: one declaration
// for the unit that defines it and for its callers.  A launch returns 0 or a hipError_t.
#pragma once
#include "af_dev.h"

struct PackArgs {
  const float* frames;    // (resy, resx, 3, F)      reference layout, unwrap_utils.py:113
  const float* flow_f;    // (resy, resx, 2, F[,1])  frame i -> i+1 at index i
  const float* flow_b;    // (resy, resx, 2, F[,1])  frame j -> j-1 at index j
  const float* mask_f;    // (resy, resx, F[,1])
  const float* mask_b;
  const float* mask_fg;   // (resy, resx, F) or null
  float* table;           // [F*resy*resx][16]
  int resx, resy, F;
  unsigned long long* nvalid;   // [64][2] += records with a valid forward / backward flow match (64 spread counters; what the batch planner expects per sample)
};
extern "C" int af_launch_pack(const PackArgs* a, hipStream_t s);

// Input builder (load_input_data*, unwrap_utils.py:40-163): bilinear resize with cv2.resize's INTER_LINEAR geometry
// (half-pixel centres, edge clamp, no anti-aliasing; :35,131) from an HWC source into an arbitrarily strided
// destination, and the forward/backward flow-consistency field || f12 + remap(f21, f12) || (:10-23).
struct ResizeArgs {
  const void* src; int src_u8;        // HWC contiguous, float32 or uint8 (uint8 is divided by 255 first, :128)
  int sh, sw, ch;
  float* dst; int dh, dw;
  long long pix_stride, ch_stride, offset;   // dst index = (y*dw + x)*pix_stride + c*ch_stride + offset
  double scale0, scale1;              // per-channel multipliers of channels 0 / 1 (resize_flow, :36-37); 1 for images
};
extern "C" int af_launch_resize(const ResizeArgs* a, hipStream_t s);
// cv2.resize(..., INTER_AREA) of a uint8 HWC image when shrinking (RAFTWrapper.load_image, raft_wrapper.py:40-44).  mode picks
// OpenCV's path: the integer 2x2 average, the integer block sum times one fp32 reciprocal, or the per-axis coverage tables.
enum { AREA_GENERAL = 0, AREA_BLOCK = 1, AREA_2X2 = 2 };
struct AreaArgs {
  const unsigned char* src; int sh, sw, ch;   // HWC contiguous, ch in 1..4
  unsigned char* dst; int dh, dw;             // HWC contiguous
  int mode;
  int isx, isy; float inv_area;               // block modes: the integer scales and float(1.f / (isx * isy))
  const int* xofs; const int* yofs;           // general mode: entries xofs[d] .. xofs[d + 1] - 1 belong to destination d ([dw + 1] / [dh + 1])
  const int* xidx; const int* yidx;           //   source index of an entry
  const float* xa; const float* ya;           //   its weight (alpha / beta), built on the host in fp64 and stored as float
};
extern "C" int af_launch_resize_area(const AreaArgs* a, hipStream_t s);
// Luminance grids of uint8 RGB frames (shots.hip, af_luma_grid): cell (i, j) of a gh x gw grid covers rows [i*h/gh, (i+1)*h/gh) and columns
// [j*w/gw, (j+1)*w/gw) (floors); a cell's rows are cut into `strips` strips of strip_rows rows, one workgroup each.
struct LumaArgs {
  const unsigned char* src; int n, h, w;      // n contiguous HWC RGB frames
  int gh, gw;                                 // already clamped to h and w: no cell is empty
  int strip_rows, strips;
  unsigned long long* part;                   // [n][gh * gw][strips] sums of 77 R + 150 G + 29 B
};
extern "C" int af_launch_luma_grid(const LumaArgs* a, hipStream_t s);
// YCbCr <-> RGB of one YUV4MPEG2 frame payload (yuv_core.h, instantiated by yuv.hip for af_yuv_to_rgb / af_rgb_to_yuv and by yuv16.hip for
// the deep entries): Y plane h x w, then Cb, then Cr, each ch x cw; integer arithmetic only, coefficients
// round(real * 2^Q) built on the host in fp64, Q = 14 at 8 bits.  S is the stored sample.
enum { YUV_AXIS_FULL = 0, YUV_AXIS_CENTRED = 1, YUV_AXIS_COSITED = 2 };      // chroma sampling of one axis
template <class S> struct YuvArgsT {
  const S* src; S* dst;                       // payload -> HWC RGB (reading), HWC RGB -> payload (writing)
  int h, w, ch, cw;
  int hmode, vmode, mono;                     // YUV_AXIS_* of the chroma planes; mono: the payload is the Y plane alone
  int y0;                                     // 16 2^(D-8) (limited) or 0 (full)
  int cy, crv, cgu, cgv, cbu;                 // reading: R = cy Y' + crv Cr', G = cy Y' + cgu Cb' + cgv Cr', B = cy Y' + cbu Cb'
  int ky[3], ku[3], kv[3];                    // writing: rows of the RGB -> Y, Cb, Cr matrix (ky sums to its scale, ku and kv to 0)
};
typedef YuvArgsT<unsigned char> YuvArgs;
extern "C" int af_launch_yuv_to_rgb(const YuvArgs* a, hipStream_t s);
extern "C" int af_launch_rgb_to_yuv(const YuvArgs* a, hipStream_t s);
// Mask propagation along the flows (maskprop.hip, af_mask_step / af_mask_blend): fp32 planes of one size h x w.
struct MaskStepArgs {
  const float* m_s; const float* c_s;         // (h, w) source mask and confidence
  const float* f_ts; const float* f_st;       // (h, w, 2) flow from the target to the source and back
  int h, w; float thresh2;                    // (float)(thresh * thresh)
  float* m_t; float* c_t;
};
struct MaskBlendArgs {
  const float* m_f; const float* c_f; const float* m_b; const float* c_b; int h, w;
  float to_b, from_a, span;                   // (float)(b - t), (float)(t - a), (float)(b - a)
  float* out;
};
extern "C" int af_launch_mask_step(const MaskStepArgs* a, hipStream_t s);
extern "C" int af_launch_mask_blend(const MaskBlendArgs* a, hipStream_t s);
// Residual guided transfer (guided.hip, af_guided_coeffs / af_guided_apply): the guided filter's coefficients of the
// residual P - I with guide I at the proxy size, their box means, and the full-size apply.  Planes are (h, w, 3) fp32, images HWC uint8.
struct GuidedCoeffArgs {
  const unsigned char* I; const unsigned char* P; int h, w;      // proxy input and proxy output
  int r; float eps;                                              // window radius 1..32; eps in squared 8-bit levels
  float* a; float* b;                                            // the raw coefficients
};
struct GuidedSmoothArgs {
  const float* a; const float* b; int h, w, r;
  float* am; float* bm;                                          // their box means over the clipped window
};
struct GuidedApplyArgs {
  const unsigned char* F; int H, W;                              // the full-size frame
  const float* a; const float* b; int h, w;                      // the smoothed planes
  double scale_x, scale_y;                                       // (double)w / (double)W and (double)h / (double)H
  unsigned char* out;                                            // (H, W, 3)
};
extern "C" int af_launch_guided_coeffs(const GuidedCoeffArgs* a, hipStream_t s);
extern "C" int af_launch_guided_smooth(const GuidedSmoothArgs* a, hipStream_t s);
extern "C" int af_launch_guided_apply(const GuidedApplyArgs* a, hipStream_t s);
// The colour guide (guided.hip, af_guided_coeffs_colour / af_guided_apply_colour): the 21 exact window sums of a proxy pair
// as int32 planes of h x w, plane-major, in the order S_c (0..2), S_dk (3..5), S_cc' (6..11: 00 01 02 11 12 22), S_c,dk (12 + 3k + c); the
// per-pixel fp64 solve to A (h, w, 9), entry 3k + c, and b (h, w, 3).  The box means and the apply take GuidedSmoothArgs and the apply
// blocks with `a` the nine-channel plane.
struct GuidedMomentArgs {
  const unsigned char* I; const unsigned char* P; int h, w, r;
  int* S;                                                        // (21, h, w)
};
struct GuidedSolveArgs {
  const int* S; int h, w, r; float eps;
  float* A; float* b;                                            // the raw coefficients
};
extern "C" int af_launch_guided_moments(const GuidedMomentArgs* a, hipStream_t s);
extern "C" int af_launch_guided_solve(const GuidedSolveArgs* a, hipStream_t s);
extern "C" int af_launch_guided_smooth_colour(const GuidedSmoothArgs* a, hipStream_t s);
extern "C" int af_launch_guided_apply_colour(const GuidedApplyArgs* a, hipStream_t s);
// Frames of more than 8 bits per sample: samples are uint16 holding D = bits bits, M = maxv = 2^D - 1, a stored sample
// above M reads as M.  The conversions (af_yuv_to_rgb16 / af_rgb_to_yuv16) run the body of the 8-bit ones under yuv16.hip's depth policy,
// which reads from the block what the 8-bit policy fixes at compile time: coefficients of Q = D + 6 fraction bits (they fit an int: below
// 2.2 * 2^22), products and sums in int64.  The depth reduction (yuv16.hip, af_depth_reduce) is element-wise; the deep apply is
// guided.hip's one apply kernel under its deep sample policy.
struct Yuv16Args : YuvArgsT<unsigned short> {
  int q, maxv, c16;                           // Q, M and 16 C = 2^(D+3)
};
extern "C" int af_launch_yuv_to_rgb16(const Yuv16Args* a, hipStream_t s);
extern "C" int af_launch_rgb_to_yuv16(const Yuv16Args* a, hipStream_t s);
struct DepthReduceArgs {
  const unsigned short* src; unsigned char* dst; long long count;
  int maxv;                                   // v8 = (510 min(v, M) + M) / (2 M)
};
extern "C" int af_launch_depth_reduce(const DepthReduceArgs* a, hipStream_t s);
struct GuidedApply16Args {                                         // GuidedApplyArgs with a deep frame; guided.hip's one apply kernel reads both
  const unsigned short* F; int H, W;
  const float* a; const float* b; int h, w;                      // the smoothed planes of the 8-bit pair
  double scale_x, scale_y;
  int maxv; float s;                                             // M; (float)((double)M / 255.0), from the host
  unsigned short* out;
};
extern "C" int af_launch_guided_apply16(const GuidedApply16Args* a, hipStream_t s);
extern "C" int af_launch_guided_apply_colour16(const GuidedApply16Args* a, hipStream_t s);
// PSNR / SSIM between two uint8 RGB sequences (fidelity.hip, af_fidelity): per workgroup and channel one 64-bit partial of
// the squared error and one fp64 partial of the SSIM values; the host adds them in block order.
struct FidelityArgs {
  const unsigned char* a; const unsigned char* b; int n, h, w;   // n contiguous HWC RGB frames each
  int win; double c1, c2;                                        // odd window 3..15; (0.01 * 255)^2 N^2 and (0.03 * 255)^2 N (N - 1), N = win^2
  unsigned long long* sse_part;                                  // [n][blocks][3] (SSIM launch: or NULL)
  double* ssim_part;                                             // [n][blocks][3] (SSIM launch)
  double* map;                                                   // [n][h - win + 1][w - win + 1][3] or NULL
};
extern "C" int af_launch_fidelity_ssim(const FidelityArgs* a, hipStream_t s);
extern "C" int af_launch_fidelity_sse(const FidelityArgs* a, hipStream_t s);
struct ConsistencyArgs {
  const float* f12; const float* f21; int h, w;     // (h, w, 2) each
  float* out; long long pix_stride, offset;         // out[(y*w + x)*pix_stride + offset] = norm (thresh <= 0) or norm < thresh
  float thresh;
};
extern "C" int af_launch_consistency(const ConsistencyArgs* a, hipStream_t s);

struct PrepArgs {
  const float* table;
  const int64_t* inds;    // [N] pixel-frame indices of this iteration, or null -> device Philox
  uint64_t seed; uint32_t iter;
  int N, resx, resy, F;
  float half_main, half_grad, half_frames;   // larger_dim/2, resx/2, F/2
  int d_local, d_global, nseg;
  float* coords;          // [rows_pad][4]   mapping1 rows
  float* x0_tile;         // [NT][32][32]
  float* samples;         // [N][16]
  int* counts;            // [2]
  // fg/bg path (stage1_neural_atlas_seg.py): mapping2 sees the same rows except the global-rigidity
  // neighbours (its own finite-difference distance); the alpha net sees segments 0,1,2 and, behind them, the compacted flow matches.
  float* coords2;         // null in the single-atlas path
  float* x0_tile2;
  float* coordsA;         // [5N pad][4]
  int d_global2;
  // compaction of the flow-match rows (loss_utils.py:328-335 evaluates the mapping nets on the VALID matches only): the
  // matches of the batch are ranked sample-major (fwd before bwd) by a decoupled look-back scan over the blocks of this
  // launch and written behind the fixed segments, row flow_base + rank (alpha net: 3N + rank).
  int* flow_rank;         // [N][2] rank of the sample's fwd / bwd match among the valid matches, -1 when invalid
  unsigned long long* scan;   // [gridDim.x] (epoch << 32 | matches of the block), indexed by the block's TICKET
  uint32_t epoch;         // unique per launch: a stale entry of an earlier launch can never satisfy the look-back
  unsigned long long* ticket; // [1] monotonic over the handle's k_prep launches: a block's virtual id = its ticket - ticket_base
  unsigned long long ticket_base;   // blocks launched by all earlier k_prep launches of the handle
  int* live;              // [1] valid matches of the batch = live rows behind flow_base
};
extern "C" int af_launch_prep(const PrepArgs* a, hipStream_t s);

struct LossArgs {
  const float* samples; const float* out_map; const float* out_atlas;
  float* dout_map; float* dout_atlas;
  const int* counts;
  const int* flow_rank; const int* live;      // see PrepArgs: rows of the valid flow matches, and how many there are
  float* loss_part;       // [nblocks][AF_LOSS_W]: rgb, gradient, rigidity, global rigidity, flow fwd, flow bwd (sums)
  int N, nseg;
  float L, uv_scale; int d_local, d_global;
  float c_rgb, c_grad, c_rig, c_grig, c_flow;
};
extern "C" int af_launch_loss_single(const LossArgs* a, hipStream_t s);

// Loss stack of the fg/bg path (stage1_neural_atlas_seg.py:220-311).  Row layouts: mapping nets as in PrepArgs
// (fixed segment s, sample n -> row s*N+n; flow matches behind them by rank, see k_prep); alpha net rows {centre, (x,y+1), (x+1,y)} + the
// same ranked flow matches behind 3N;
// atlas rows {m1 centre, m1 (x,y+1), m1 (x+1,y), m2 centre, m2 (x,y+1), m2 (x+1,y)}.
// loss_part sums: 0 rgb, 1 gradient, 2 rigidity1, 3 rigidity2, 4 global rigidity1, 5 global rigidity2,
// 6 flow1 fwd, 7 flow1 bwd, 8 flow2 fwd, 9 flow2 bwd, 10 alpha-flow fwd, 11 alpha-flow bwd, 12 BCE, 13 sparsity.
struct LossSegArgs {
  const float* samples;
  const float* out_m1; const float* out_m2; const float* out_alpha; const float* out_atlas;
  float* dout_m1; float* dout_m2; float* dout_alpha; float* dout_atlas;
  const int* counts; float* loss_part;
  const int* flow_rank; const int* live;
  int N, nseg;
  float L, uv_scale; int d_local, d_global_fg, d_global_bg;
  float c_rgb, c_grad, c_rig, c_grig_fg, c_grig_bg, c_flow, c_boot, c_aflow, c_sparse;
};
extern "C" int af_launch_loss_seg(const LossSegArgs* a, hipStream_t s);

struct PrePrepArgs {
  const int64_t* ys; const int64_t* xs;   // host-provided rows/cols or null
  uint64_t seed; uint32_t iter;
  int N, resx, resy;
  float half_main, t;
  float* coords; float* x0_tile;
};
struct PreLossArgs { const float* coords; const float* out_map; float* dout_map; float* loss_part; int N; float uv_scale; };
extern "C" int af_launch_pre_prep(const PrePrepArgs* a, hipStream_t s);
extern "C" int af_launch_pre_loss(const PreLossArgs* a, hipStream_t s);

// render (k_frame_coords_at / k_frame_finish_at): one band [r0, r0 + n) of the row-major pixels of an oh x ow grid; the lattice is one band
struct CoordsAtArgs {
  float* coords;          // [n_pad][4]
  int resx, resy;         // the stage-1 lattice the nets were fitted on
  int oh, ow;
  float half_main, t;
  long long r0; int n, n_pad;
};
struct FinishAtArgs {
  const float* out_atlas; const float* out_alpha; size_t row2;     // chain outputs of the band; out_alpha NULL: single atlas, else the bg rows start row2 rows in
  int n;
  float* rgb_out;               // [n][3] or NULL
  unsigned char* u8_out;        // [n][3] or NULL
  const unsigned char* ref;     // [n][3] or NULL: the reference image's pixels of the band
  const float* table; size_t rec0;     // or NULL: the record table, the band's pixels are records rec0 .. rec0 + n (at most one of ref, table)
  double* sse_part;             // [ceil(n / 256)] or NULL
};
extern "C" int af_launch_frame_coords_at(const CoordsAtArgs* a, hipStream_t s);
extern "C" int af_launch_frame_finish_at(const FinishAtArgs* a, hipStream_t s);

struct AdamJob {
  uint32_t part_off, part_blk, nslots, pld;
  uint32_t out_real, in_real, out_real_pad;
  uint32_t p_off;       // flat param offset of W[0][col0]
  uint32_t p_ld;        // in_features of the layer (canonical row length)
  uint32_t col0;
  int32_t  b_off;       // flat param offset of the bias, or -1 when another job of the layer owns it
  uint32_t f_off;       // forward image: float offset of this layer's image
  uint32_t f_mpad;
  int32_t  b_img_off;   // backward image (W^T) float offset, or -1
  uint32_t b_mpad;
  uint32_t bias_img_off;// float offset in the padded bias array
  uint32_t pe_kind;     // column -> slot permutation for columns >= hid_cols (0/1 identity, 2 alpha)
  uint32_t hid_cols;    // leading identity-mapped columns of the LAYER (256 for skip layers, 0 for PE first layers, p_ld otherwise)
  // weight streams of the bf16x6 chains (mlpbf.hip): byte offset of the block this job writes, its kind (0 = fp32 block packed like
  // the fp32 images with row padding *_mpad and reduction index k - sf_k0; 1 = 256x256 block as three bf16 images), -1 = none
  int32_t  sf_off; uint32_t sf_kind, sf_mpad, sf_k0;
  int32_t  sb_off; uint32_t sb_kind, sb_mpad;
  // weight streams of the f16x3 chains (mlphf.hip): the same blocks in that stream's plan (fp32 blocks as above; kind 1 = 256x256 block as two fp16 images of 2^12 W)
  int32_t  hf_off, hb_off;
};
struct AdamHyper { float step_size, bc2_sqrt, one_minus_b1, beta2, one_minus_b2, eps; };
struct AdamBufs { float* params; float* m; float* v; float* img_f; float* img_b; float* bias_img; char* sf; char* sb; char* hf; char* hb; };
struct AdamArgs {
  const AdamJob* jobs; const float* partial;
  AdamBufs bufs; AdamHyper hy;
  float* grad_out;           // optional: reduced gradient in flat param order (tests)
  const float* loss_part; float* loss_out; int* counts; int loss_nblk;
  int* nan_flag;             // bit 0: a parameter is not finite, a folded loss term is NaN, or (check_counts) a flow-match set is empty;
                             // bit 1: a hidden-layer weight with |w| >= 8 (the fixed 2^12 scale of the fp16 images covers |w| < 16: mlphf.hip)
  int check_counts;
};
extern "C" int af_launch_adam(const AdamArgs* a, int njobs, int update, hipStream_t s);

// texture-edit propagation (layers.hip k_edit): per layer L (0 fg, 1 bg) the window and texture; a layer with active[L] == 0 is skipped
struct EditArgs {
  const float* uv1; const float* uv2; const float* out_alpha;     // chain outputs, [rows][4]
  int npix, res;
  int active[2]; float minx[2], miny[2], pixel_size[2];
  const float* tex[2];        // (res, res, 3) or NULL: usage masks only
  float* edit; float* edit_layer[2]; float* use[2];                // each may be NULL
  unsigned char* edit_u8;     // [rows][3] or NULL: the truncated byte of edit (the edit sessions)
};
extern "C" int af_launch_edit(const EditArgs* a, hipStream_t s);
// the other launches of layers.hip take their arguments one by one
extern "C" int af_launch_area_reduce(const float* uv, const float* out_alpha, const float* table, size_t rec0, int npix, int which, float* part, hipStream_t s);
extern "C" int af_launch_tex_coords(float* coords, int res, int row0, int nrows, float sx, float ex, float sy, float ey, int rows_pad, hipStream_t s);
extern "C" int af_launch_tex_finish(const float* out_atlas, int rows, float* out, hipStream_t s);
extern "C" int af_launch_layer_finish(const float* uv1s, const float* uv2s, const float* out_atlas, size_t row2, const float* out_alpha, int npix,
                                      float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2, unsigned char* alpha_u8, hipStream_t s);

// per-pixel loss maps of one frame (lossmaps.hip): input rows in segments of rows_pad rows (seg_* < 0: not built), chain outputs, maps
struct LossMapArgs {
  float* coords; const float* table; size_t rec0;
  int resx, resy, rows_pad, frame, d;
  int seg_c, seg_ym, seg_xm, seg_t;
  float half_main, half_frames, t_centre;
  const float* out_m1; const float* out_m2;       // mapping chains over segments [0, nseg_map)
  const float* out_alpha;                          // null: single path (alpha = 1); else centre rows, then rows_pad rows later the target rows
  const float* out_atlas;                          // fg rows, then rows_pad rows later the bg rows
  int flow_map;                                    // the mapping nets saw the flow-target segment (not on the last frame)
  float L, uv_scale;
  float* rigidity1; float* rigidity2; float* flow1; float* flow2; float* flow_alpha; float* rgb_err; float* residual;   // each may be NULL
};
extern "C" int af_launch_lossmap_rows(const LossMapArgs* a, hipStream_t s);
extern "C" int af_launch_lossmap_finish(const LossMapArgs* a, hipStream_t s);

// warping error of frame pairs (warperr.hip): strided sources (see k_warp_error), optional per-pixel outputs, fp64 block partials
struct WarpErrArgs {
  const float* img1; const float* img2; const float* flow12; const float* flow21;
  size_t img_pair_stride, flow_pair_stride;        // floats between consecutive pairs (0: one pair)
  int h, w, align_corners;
  float* noc; float* warped;                       // [npairs][h*w] and [npairs][h*w][3], each may be NULL
  double* part;                                    // [npairs][nblk][2]
};
extern "C" int af_launch_warp_error(const WarpErrArgs* a, int kind, int npairs, hipStream_t s);
