/* atlasfit.h — C ABI of libatlasfit.so: the MI355X-native (gfx950) implementation of the stage-1
 * neural-atlas optimisation loop of All-In-One-Deflicker.
 *
 * The reference has no plugin/operator API for this path; its seams are the stage-1 script and the
 * Python objects it drives.  Each entry point below names the reference code it replaces
 * (paths relative to the reference repository root).  A handle owns ONE video on ONE device with ONE
 * stream (reference: one process per GPU via CUDA_VISIBLE_DEVICES, src/stage1_neural_atlas.py:267-268).
 *
 * Conventions: every function returns 0 on success and a negative af_status on failure (message via
 * af_last_error); nothing throws across the boundary; host buffers are borrowed for the duration of
 * the call; the handle owns all device memory.  All tensors are fp32 unless stated.
 */
#ifndef ATLASFIT_H
#define ATLASFIT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct af_handle af_handle;

enum af_status { AF_OK = 0, AF_EINVAL = -1, AF_EHIP = -2, AF_ENOMEM = -3, AF_ENAN = -4, AF_ESTATE = -5,
                 AF_ERANGE = -6   /* af_set_mlp_mode(h, 3) only: a hidden-layer weight left the range its fp16 images are scaled for (|w| >= 8) */ };
enum af_net { AF_MAPPING1 = 0, AF_ATLAS = 1, AF_MAPPING2 = 2, AF_ALPHA = 3 };

/* Mirrors the keys of src/config/config_flow_100.json that the loop reads
 * (src/stage1_neural_atlas.py:28-90) plus the sizes main() derives (resx, resy, number_of_frames). */
typedef struct af_config {
  int32_t resx, resy, number_of_frames;          /* stage1_neural_atlas.py:31-38,108 */
  int32_t samples_batch;                         /* config :7 */
  /* number_of_channels_*: 1..256 (a narrower net runs exactly, zero-padded inside the 256-wide kernels; all flat parameter / Adam-state / gradient
   * buffers of this ABI are in the CONFIGURED net's state_dict order and size); number_of_layers_*: 2..8 */
  int32_t number_of_channels_mapping1, number_of_layers_mapping1;   /* config :24-25  (256, 6) */
  int32_t number_of_channels_atlas, number_of_layers_atlas;         /* config :19-20  (256, 8) */
  int32_t positional_encoding_num_atlas;         /* config :31 (10) */
  int32_t use_positional_encoding_mapping1;      /* config :32 (false) */
  int32_t derivative_amount;                     /* config :10 */
  int32_t include_global_rigidity_loss;          /* config :39 */
  int32_t global_rigidity_derivative_amount_fg;  /* config :40 */
  int32_t stop_global_rigidity;                  /* config :44 */
  int32_t use_gradient_loss;                     /* config :29 (true); false: the gradient term is 0 and carries no gradient (stage1_neural_atlas.py:185-190) */
  float rgb_coeff, gradient_loss_coeff, rigidity_coeff, optical_flow_coeff;   /* config :11,28,12,8 */
  float global_rigidity_coeff_fg;                /* config :42 */
  float uv_mapping_scale;                        /* config :13 */
  float lr;                                      /* 1e-4, hard-coded at stage1_neural_atlas.py:134 */
  int32_t pretrain_batch;                        /* 10000, hard-coded at unwrap_utils.py:182-183 */
  /* ---- fg/bg dual-atlas path (src/stage1_neural_atlas_seg.py:27-107); read only when two_layer != 0 ---- */
  int32_t two_layer;                             /* 0: stage1_neural_atlas.py   1: stage1_neural_atlas_seg.py */
  int32_t number_of_channels_mapping2, number_of_layers_mapping2;   /* config :26-27  (256, 4) */
  int32_t number_of_channels_alpha, number_of_layers_alpha;         /* config :21-22  (256, 8) */
  int32_t positional_encoding_num_alpha;         /* config :18 (5) */
  int32_t use_positional_encoding_mapping2;      /* config :34 (false) */
  int32_t global_rigidity_derivative_amount_bg;  /* config :41 */
  int32_t stop_bootstrapping_iteration;          /* config :23 */
  float global_rigidity_coeff_bg;                /* config :43 */
  float alpha_bootstrapping_factor, alpha_flow_factor, sparsity_coeff;   /* config :16,17,30 */
  int32_t number_of_positional_encoding_mapping1;   /* config :33 (4): frequencies K of mapping1's PE (3 -> 6K), 1..5, read when use_positional_encoding_mapping1 */
  int32_t number_of_positional_encoding_mapping2;   /* config :35 (2): the same for mapping2 */
  int32_t reserved[2];
} af_config;

/* Replaces model construction + optimizer construction (stage1_neural_atlas.py:112-134).  Parameters
 * start at zero; load them with af_set_params. */
int af_create(const af_config* cfg, int device_ordinal, af_handle** out);
size_t af_config_size(void);                     /* sizeof(af_config) of this build: bindings check their mirror against it */
void af_destroy(af_handle* h);
const char* af_last_error(const af_handle* h);   /* h may be NULL: message of the last failed af_create */

/* Replaces the tensors returned by load_input_data_single (src/models/stage_1/unwrap_utils.py:105-163),
 * the dx/dy construction (:132-133) and get_tuples (:166-173; the index table is arithmetic here).
 * Layouts are the reference's: frames (resy,resx,3,F); flows (resy,resx,2,F[,1]); masks (resy,resx,F[,1]);
 * mask_fg (resy,resx,F) or NULL.  on_device != 0: the pointers are device pointers on this handle's GPU. */
int af_upload_video(af_handle* h, const float* frames, const float* flow_fwd, const float* flow_bwd,
                    const float* mask_fwd, const float* mask_bwd, const float* mask_fg, int on_device);

/* ---- input builder (the device side of load_input_data / load_input_data_single, unwrap_utils.py:40-163) ----------
 * Stateless utilities on `device_ordinal`; with on_device != 0 the pointers are device pointers, else host buffers.
 *
 * af_resize_bilinear: cv2.resize(src, (dw, dh)) with the default INTER_LINEAR geometry (half-pixel centres, edge clamp,
 * no anti-aliasing; unwrap_utils.py:35,131).  src is HWC contiguous, float32 (src_u8 = 0) or uint8 (src_u8 = 1: divided
 * by 255 first, :128).  dst element (y, x, c) is written at dst[(y*dw + x)*pix_stride + c*ch_stride + offset] — e.g.
 * frame f of video_frames (resy,resx,3,F): pix_stride 3F, ch_stride F, offset f.  scale0/scale1 multiply channels 0/1
 * (resize_flow's newh/oldh and neww/oldw, :36-37); pass 1 for images.
 * af_flow_consistency: out[(y*w + x)*pix_stride + offset] = || f12 + remap(f21, f12) ||_2 (:10-23, bilinear, zero
 * border) if thresh <= 0, else 1.0 / 0.0 for norm < thresh (the mask of :151-159 with thresh = 1).
 *
 * af_resize_area: cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) of a uint8 image when shrinking, the resize
 * RAFTWrapper.load_image applies to a frame longer than --max_long_edge (raft_wrapper.py:40-44).  src (sh, sw, ch) and dst
 * (dh, dw, ch) are HWC contiguous uint8, ch in 1..4.  The arithmetic is OpenCV 4.x's: integer scales on both
 * axes take the block-sum path ((s + 2) >> 2 for 2x2 unless ch == 2, else (float)sum times the float 1.f / area), any other
 * size the fp64-built, float-stored coverage tables with fp32 accumulation in OpenCV's order; round half to even, clamp.
 * AF_EINVAL (message through af_last_error(NULL)) for null pointers, ch outside 1..4, dh < 1, dw < 1, dh > sh, dw > sw and
 * dh == sh && dw == sw: enlarging and copying are not this function's business.  Host-synchronous like its neighbours.
 *
 * af_luma_grid: the exact luminance grids the cut detector scores (shots.py).  src is n contiguous HWC RGB uint8
 * frames of h x w; sums_out is HOST memory of n * GH * GW values, GH = min(gh, h), GW = min(gw, w) (no cell is empty).  Cell (i, j)
 * covers rows [floor(i*h/GH), floor((i+1)*h/GH)) and columns [floor(j*w/GW), floor((j+1)*w/GW)); its value is the integer sum of
 * 77 R + 150 G + 29 B over the cell, 64 bits wide (a cell's total can pass 2^32).  Integer arithmetic only: the result is exact and
 * independent of the order of summation.  AF_EINVAL for null pointers, n, h or w < 1, gh or gw outside 1..64 (and an axis longer
 * than 2^24).  Stateless and host-synchronous.
 *
 * af_yuv_to_rgb / af_rgb_to_yuv: one YUV4MPEG2 frame payload <-> one (h, w, 3) uint8 RGB image, HWC contiguous (y4m.py).
 * The payload is the Y plane h x w, then Cb, then Cr, each ch x cw, cw = ceil(w / 2) where the layout is horizontally subsampled (422
 * and both 420) and ch = ceil(h / 2) where it is vertically subsampled (both 420); AF_YUV_MONO is the Y plane alone (R = G = B on the
 * way in).  Chroma siting: 420JPEG centred on both axes; 420MPEG2 and 422 left-cosited horizontally (420MPEG2 centred vertically).
 * matrix: BT.601 (Kr 0.299, Kb 0.114) or BT.709 (Kr 0.2126, Kb 0.0722); full_range 0: Y in 16..235, chroma 16..240, else 0..255.
 * 8 bits per sample, progressive.  Integer arithmetic only (14-bit coefficients built on the host in fp64, chroma interpolated /
 * filtered exactly, one rounding per output byte): the result is exact and independent of any order.  AF_EINVAL (message through
 * af_last_error(NULL)) for null pointers, h or w outside 1..16384, an unknown layout or matrix.  Stateless and host-synchronous.
 * af_yuv_frame_bytes: the size of that payload, 0 for an argument the two calls would refuse.
 *
 * af_mask_step / af_mask_blend: propagation of a fg mask along the flows (masks.py).  All planes are fp32, row-major, of
 * one size h x w; a flow is (h, w, 2) with x in component 0.  af_mask_step makes one step from a source frame s to a neighbouring
 * target frame t: m_s, c_s are the source's mask and confidence (values in [0, 1]), f_ts the flow from t to s, f_st the flow from s to
 * t.  Target pixel (x, y) looks up q = (x + f_ts[y,x,0], y + f_ts[y,x,1]); where q lies in the frame (0 <= qx <= w - 1 and
 * 0 <= qy <= h - 1; a NaN does not) and the round trip f_ts[y,x] + bil(f_st)(q) is shorter than thresh, m_t = bil(m_s)(q) and
 * c_t = bil(c_s)(q); elsewhere m_t = m_s[y,x] and c_t = 0 (the value is held and carries no confidence).  bil is the bilinear look-up
 * with x0 = (int)qx, x1 = min(x0 + 1, w - 1), ax = qx - x0: (v00 (1 - ax) + v01 ax)(1 - ay) + (v10 (1 - ax) + v11 ax) ay.  The test is
 * dx dx + dy dy < (float)(thresh * thresh); thresh = 1 is the reference's flow filter (unwrap_utils.py:10-23).  af_mask_blend serves a
 * frame t strictly between two keys a < t < b: wf = (b - t) c_f, wb = (t - a) c_b, out = (wf m_f + wb m_b) / (wf + wb) where that sum is
 * positive, else ((b - t) m_f + (t - a) m_b) / (b - a); clamped to [0, 1].  Every operation is a single fp32 operation in the order
 * written (no fused multiply-add), so both functions can be restated exactly on a host.  AF_EINVAL (message through
 * af_last_error(NULL)) for null pointers, h or w outside 1..16384, thresh not finite or <= 0, not a < t < b, and an output that overlaps
 * an input (or the other output); the outputs are then untouched.  Stateless and host-synchronous.
 *
 * af_guided_coeffs / af_guided_apply: residual guided transfer (guided.py): the correction a pipeline made on a proxy-size
 * copy of a frame, carried to the full-size frame as a smooth gain and offset field.  Images are HWC contiguous uint8 with 3 channels,
 * coefficient planes (h, w, 3) fp32; every channel is treated on its own.  af_guided_coeffs takes the proxy input I and the proxy output
 * P (both h x w) and runs the guided filter of the residual d = P - I with guide I: over the (2r + 1)^2 window of a pixel clipped to the
 * frame (n pixels) the exact integer sums S_I, S_d, S_II, S_Id; a = float(n S_Id - S_I S_d) / (float(n S_II - S_I^2) + eps float(n n)),
 * b = (float(S_d) - a float(S_I)) / float(n) (the integer expressions in int64); a_out and b_out receive the box means of a and b over
 * the same clipped window, summed in fp32 along each row left to right from 0, then down the rows top to bottom from 0, then divided by
 * float(n).  eps is in squared 8-bit levels.  work: NULL, or with on_device 2 * h * w * 3 floats of device memory for the unsmoothed
 * planes (else the call allocates them).  af_guided_apply samples the two planes bilinearly at the centres of the H x W pixels, source
 * position s = (X + 0.5) * (w / W) - 0.5 in fp64 clamped to [0, w - 1], x0 = (int)s, x1 = min(x0 + 1, w - 1), ax = (float)(s - x0) (y alike),
 * top = v00 + ax (v01 - v00), bot = v10 + ax (v11 - v10), v = top + ay (bot - top), and writes
 * out = clamp(rint(F + (abar F + bbar)), 0, 255), rounding half to even.  Every operation is a single correctly rounded operation in
 * the order written (no fused multiply-add), so both can be restated exactly on a host; P == I returns F, P == I + c (nothing clipped)
 * returns F + c.  AF_EINVAL (message through af_last_error(NULL)) for null pointers, r outside 1..32, eps not finite or <= 0, a side
 * outside 1..16384, a proxy larger than the full frame and outputs that overlap an input or each other.  Stateless and host-synchronous.
 *
 * af_fidelity: PSNR and SSIM material between two sequences (fidelity.py).  a and b are n contiguous HWC RGB uint8 frames
 * of h x w (host or device pointers, on_device); every channel is treated on its own.  sse_out and ssim_out are HOST memory of n * 3
 * values whatever on_device says, ssim_map (n, h - win + 1, w - win + 1, 3) fp64 follows on_device; each may be NULL.  sse_out[f][c] is
 * the integer sum of (a - b)^2 over the frame: exact, independent of the order of summation (a 16384 x 16384 frame stays below 2^64).
 * The SSIM is skimage.metrics.structural_similarity's at its defaults for uint8 (uniform win x win window, sample covariance, K1 0.01,
 * K2 0.03, data range 255) at every window that lies wholly inside the frame, which is skimage's crop of (win - 1) / 2.  With N = win^2
 * and the exact integer window sums Sx, Sy, Sxx, Syy, Sxy (int64 expressions), c1 = (0.01 * 255)^2 N^2 and c2 = (0.03 * 255)^2 N (N - 1)
 * built in fp64 ((k * k) * (double)(N * N), (k * k) * (double)(N * (N - 1))):
 *   A1 = (double)(2 Sx Sy) + c1, B1 = (double)(Sx^2 + Sy^2) + c1, A2 = (double)(2 (N Sxy - Sx Sy)) + c2,
 *   B2 = (double)((N Sxx - Sx^2) + (N Syy - Sy^2)) + c2, S = (A1 A2) / (B1 B2),
 * every fp64 operation one correctly rounded operation in the order written (no fused multiply-add), so a host can restate S exactly.
 * ssim_map receives S; ssim_out[f][c] is the sum of S over the windows divided by their count, the sum taken in fp64 from per-workgroup
 * partials in one fixed order without atomics: two calls agree bitwise.  AF_EINVAL (message through af_last_error(NULL), outputs
 * untouched) for a null a or b, all three outputs null, ssim_map without ssim_out, n < 1, win even or outside 3..15, h or w below win or
 * above 16384.  Stateless and host-synchronous.
 *
 * af_yuv_to_rgb16 / af_rgb_to_yuv16 / af_depth_reduce / af_guided_apply16: frames of more than 8 bits per sample (y4m.py, guided.py,
 * DESIGN.md 2.18).  A sample is a uint16 holding a value of `bits` bits, bits (written D) in 8..16, M = 2^D - 1; a stored sample above M
 * reads as M.  Every uint16 pointer must be 2-byte aligned.
 * The two conversions are af_yuv_to_rgb / af_rgb_to_yuv restated at depth D: the payload is the same planes as uint16, the image (h, w, 3)
 * uint16.  The coefficients carry Q = D + 6 fraction bits (14 at D = 8), built on the host in fp64 by the same expressions and rounded
 * with nearbyint(v 2^Q), the forward rows adjusted at their largest entry to sum to nearbyint(sy 2^Q) and to 0.  y0 = 16 2^(D-8) in limited
 * range, else 0; the chroma centre is C = 2^(D-1); sy = 219 2^(D-8) / M and sc = 224 2^(D-8) / M in limited range, else 1.  Reading: with
 * the interpolated chroma c16 in sixteenths (the 8-bit weights and clamped indices), acc = cy 16 (Y - y0) + cu (cb16 - 16 C) + cv (cr16 - 16 C)
 * in int64 and out = clamp((acc + 2^(Q+3)) >> (Q+4), 0, M).  Writing: Y = clamp(((ky . rgb + 2^(Q-1)) >> Q) + y0, 0, M); chroma is left
 * unrounded per pixel, summed over the 8-bit taps, rounded once by Q plus the taps' log2, has C added and is clamped to [0, M].  Integer
 * arithmetic only: exact, independent of any order, and at bits = 8 on bytes widened to uint16 the values of the 8-bit calls.
 * af_depth_reduce maps count samples to bytes, v8 = (510 min(v, M) + M) / (2 M) in integer division: round(255 v / M), where no tie
 * exists; the identity at D = 8.  count is 1..2^32.
 * af_guided_apply16 is af_guided_apply on a uint16 frame with the planes of an 8-bit pair: the same geometry and taps, and with
 * f = (float)min(F, M) and s = (float)((double)M / 255.0): p = abar f, q = bbar s, t = p + q, out = clamp(rint(f + t), 0, M), each one fp32
 * operation, rounding half to even, a NaN becomes 0.  s is exactly 1 at D = 8 (the bytes of af_guided_apply) and 257 at D = 16.
 * AF_EINVAL (message through af_last_error(NULL), outputs untouched) for what the 8-bit siblings refuse, bits outside 8..16, a misaligned
 * uint16 pointer and a count outside its range.  Stateless and host-synchronous.
 *
 * af_guided_coeffs_colour / af_guided_apply_colour / af_guided_apply_colour16: the guided transfer with a colour guide (guided.py,
 * DESIGN.md 2.19): every output channel k is fitted on all three guide channels, d_k ~ sum_c A_kc I_c + b_k, so the field can carry a
 * correction that mixes channels.  Arguments as the per-channel siblings', with A_out (h, w, 9) fp32, entry 3k + c, and b_out (h, w, 3).
 * Over the clipped (2r + 1)^2 window of a proxy pixel (n pixels), with d_k = P_k - I_k, the exact integer sums S_c (3), S_dk (3),
 * S_cc' = sum I_c I_c' (6) and S_c,dk = sum I_c d_k (9), each below 4225 * 255^2 (int32); in int64
 *   Sigma_cc' = n S_cc' - S_c S_c',   kappa_ck = n S_c,dk - S_c S_dk   (both below 2^53: exact as fp64).
 * With e = (double)eps * (double)(n n), m_cc' = (double)Sigma_cc' (+ e where c = c'), the system (Sigma + e I) x_k = kappa_.k is solved in
 * fp64 by LDL^T without pivoting, every line one correctly rounded fp64 operation per operator in the order written, no fused multiply-add:
 *   d0 = m00;  l10 = m01 / d0;  l20 = m02 / d0;
 *   d1 = m11 - l10 * m01;
 *   t21 = m12 - l20 * m01;  l21 = t21 / d1;
 *   d2 = (m22 - l20 * m02) - l21 * t21;
 * and for each k, with r_c = (double)kappa_ck:
 *   z0 = r0;  z1 = r1 - l10 * z0;  z2 = (r2 - l20 * z0) - l21 * z1;
 *   x2 = z2 / d2;  x1 = z1 / d1 - l21 * x2;  x0 = (z0 / d0 - l10 * x1) - l20 * x2;
 *   b_k = ((double)S_dk - ((x0 * (double)S_0 + x1 * (double)S_1) + x2 * (double)S_2)) / (double)n;
 * A_k0, A_k1, A_k2 = (float)x0, (float)x1, (float)x2 and b_k = (float)b_k: one rounding to fp32 each.  In exact arithmetic every pivot
 * d is at least e, so eps has a floor: 2^-20 (the pivots' rounding error is a few ulp of n^2 255^2, and they keep more than 16 good bits
 * there).  A_out and b_out receive the box means of the 12 planes in af_guided_coeffs's fp32 order.  work: NULL, or with on_device
 * 33 * h * w four-byte words of device memory (the 21 int32 planes of sums, then the unsmoothed A and b); else the call allocates them.
 * af_guided_apply_colour samples the 12 planes with af_guided_apply's taps and bilinear expression and, per output channel k in fp32,
 * one operation per step: t = A_k0 f_0; t = t + A_k1 f_1; t = t + A_k2 f_2; t = t + b_k; out_k = clamp(rint(f_k + t), 0, 255).
 * af_guided_apply_colour16 is that on a uint16 frame of `bits` bits: f = (float)min(F, M), t = t + b_k s with s of af_guided_apply16,
 * clamped to M.  With A = diag(a) the added terms are exact zeros and the result is af_guided_apply's (af_guided_apply16's) byte for byte;
 * P == I returns F, P == I + c (nothing clipped) returns F + c: kappa is then exactly 0 and b exactly c.  AF_EINVAL (message through
 * af_last_error(NULL), outputs untouched) for what the per-channel siblings refuse, and for eps below 2^-20.  Stateless and
 * host-synchronous. */
enum { AF_YUV_444 = 0, AF_YUV_422 = 1, AF_YUV_420JPEG = 2, AF_YUV_420MPEG2 = 3, AF_YUV_MONO = 4 };
enum { AF_YUV_BT601 = 0, AF_YUV_BT709 = 1 };
int af_resize_bilinear(int device_ordinal, const void* src, int src_u8, int sh, int sw, int ch, float* dst, int dh, int dw,
                       int64_t pix_stride, int64_t ch_stride, int64_t offset, double scale0, double scale1, int on_device);
int af_resize_area(int device_ordinal, const uint8_t* src, int sh, int sw, int ch, uint8_t* dst, int dh, int dw, int on_device);
int af_luma_grid(int device_ordinal, const uint8_t* src, int n, int h, int w, int gh, int gw, uint64_t* sums_out, int on_device);
int af_yuv_to_rgb(int device_ordinal, const uint8_t* yuv, int h, int w, int layout, int matrix, int full_range, uint8_t* rgb, int on_device);
int af_rgb_to_yuv(int device_ordinal, const uint8_t* rgb, int h, int w, int layout, int matrix, int full_range, uint8_t* yuv, int on_device);
int64_t af_yuv_frame_bytes(int h, int w, int layout);
int af_mask_step(int device_ordinal, const float* m_s, const float* c_s, const float* f_ts, const float* f_st, int h, int w, float thresh,
                 float* m_t, float* c_t, int on_device);
int af_mask_blend(int device_ordinal, const float* m_f, const float* c_f, const float* m_b, const float* c_b, int h, int w, int a, int t, int b,
                  float* out, int on_device);
int af_guided_coeffs(int device_ordinal, const uint8_t* proxy_in, const uint8_t* proxy_out, int h, int w, int r, float eps,
                     float* a_out, float* b_out, float* work, int on_device);
int af_guided_apply(int device_ordinal, const uint8_t* full, int H, int W, const float* a, const float* b, int h, int w, uint8_t* out,
                    int on_device);
int af_yuv_to_rgb16(int device_ordinal, const uint16_t* yuv, int h, int w, int layout, int matrix, int full_range, int bits, uint16_t* rgb,
                    int on_device);
int af_rgb_to_yuv16(int device_ordinal, const uint16_t* rgb, int h, int w, int layout, int matrix, int full_range, int bits, uint16_t* yuv,
                    int on_device);
int af_depth_reduce(int device_ordinal, const uint16_t* src, int64_t count, int bits, uint8_t* dst, int on_device);
int af_guided_apply16(int device_ordinal, const uint16_t* full, int H, int W, int bits, const float* a, const float* b, int h, int w,
                      uint16_t* out, int on_device);
int af_guided_coeffs_colour(int device_ordinal, const uint8_t* proxy_in, const uint8_t* proxy_out, int h, int w, int r, float eps,
                            float* A_out, float* b_out, float* work, int on_device);
int af_guided_apply_colour(int device_ordinal, const uint8_t* full, int H, int W, const float* A, const float* b, int h, int w, uint8_t* out,
                           int on_device);
int af_guided_apply_colour16(int device_ordinal, const uint16_t* full, int H, int W, int bits, const float* A, const float* b, int h, int w,
                             uint16_t* out, int on_device);
int af_fidelity(int device_ordinal, const uint8_t* a, const uint8_t* b, int n, int h, int w, int win,
                uint64_t* sse_out,   /* [n][3] or NULL */
                double*   ssim_out,  /* [n][3] or NULL */
                double*   ssim_map,  /* [n][h-win+1][w-win+1][3] or NULL */
                int on_device);
int af_flow_consistency(int device_ordinal, const float* f12, const float* f21, int h, int w, float* out,
                        int64_t pix_stride, int64_t offset, float thresh, int on_device);

/* IMLP.state_dict() order: hidden.0.weight (out,in) row-major, hidden.0.bias, hidden.1.weight, ...
 * (src/models/stage_1/implicit_neural_networks.py:37-52). */
size_t af_param_count(const af_handle* h, int net);
int af_set_params(af_handle* h, int net, const float* flat, size_t n);
int af_get_params(af_handle* h, int net, float* flat, size_t n);
/* torch.optim.Adam state of optimizer_all (exp_avg, exp_avg_sq, step) for one net's parameters. */
int af_get_adam_state(af_handle* h, int net, float* exp_avg, float* exp_avg_sq, int64_t* step);
int af_set_adam_state(af_handle* h, int net, const float* exp_avg, const float* exp_avg_sq, int64_t step);

/* pre_train_mapping (src/models/stage_1/unwrap_utils.py:176-198): pretrain_iters x number_of_frames Adam
 * steps (own optimizer, zeroed per call) on `net` (AF_MAPPING1/2).  It steps at cfg.lr: the reference hard-codes
 * 1e-4 here and has no such config field, so a caller who sets `lr` gets it in pre-training as well.
 * ys/xs: [pretrain_iters*F][pretrain_batch]
 * row / column draws in the reference's order (i_s then j_s), or NULL for the device sampler(seed).
 * losses_out: [pretrain_iters*F] mean loss per step, or NULL.
 * When AF_ERANGE is returned the steps have run and losses_out is written, as by af_train_steps (AF_ENAN: not). */
int af_pretrain(af_handle* h, int net, int pretrain_iters, const int64_t* ys, const int64_t* xs,
                uint64_t seed, float* losses_out);

/* The loop body (src/stage1_neural_atlas.py:151-231, or src/stage1_neural_atlas_seg.py:191-315 for a
 * two_layer handle) for iterations first_iter .. first_iter+n_iters-1.
 * inds: [n_iters][samples_batch] values of inds_foreground (:159-160), or NULL for the device sampler.
 * losses_out: [n_iters][af_loss_width(h)] or NULL.
 *   single (width 8): rgb, gradient, rigidity, global rigidity, flow, total, #valid fwd, #valid bwd
 *     (the un-weighted terms of :186-218 and the weighted sum of :220-227);
 *   two_layer (width 16): rgb, gradient, rigidity1, rigidity2, global rigidity1, global rigidity2, flow1, flow2,
 *     alpha-flow, alpha bootstrapping (BCE), sparsity, total, #valid fwd, #valid bwd, 0, 0
 *     (stage1_neural_atlas_seg.py:237-311). */
int af_train_steps(af_handle* h, int first_iter, int n_iters, const int64_t* inds, uint64_t seed,
                   float* losses_out);
int af_loss_width(const af_handle* h);

/* Forward-only reconstruction of one frame (src/models/stage_1/evaluate.py:640-661):
 * rgb_out (resy,resx,3) host buffer or NULL; sse_out: sum of squared error vs the input frame (fp64). */
int af_render_frame(af_handle* h, int frame, float* rgb_out, double* sse_out);
/* The same reconstruction (same chains, same finish arithmetic, same error cache for af_psnr) handed on without a host round trip:
 * rgb_out (resy,resx,3) fp32 and u8_out (resy,resx,3) bytes, each optional (NULL: not written); with on_device != 0 both are device
 * pointers on the handle's device, else host pointers.  u8_out = (uint8)((double)rgb * 255), truncated: the cast the reference
 * applies before it writes stage_1/output (evaluate.py:732-733), so u8_out is that PNG's pixels.  Returns host-synchronous. */
int af_render_frame_u8(af_handle* h, int frame, float* rgb_out, uint8_t* u8_out, int on_device, double* sse_out);
/* The reconstruction of one frame at another size: the fitted nets evaluated at the pixel centres of an oh x ow grid (1..16384 each)
 * laid over the stage-1 lattice resx x resy, instead of a resize of af_render_frame's image.  Geometry: OpenCV's pixel-centre rule, the
 * one the builder's down-scale and stage 2's up-scale use.  Output column X reads the lattice position
 *     sx = (float)clamp(((double)X + 0.5) * ((double)resx / ow) - 0.5, 0, resx - 1)
 * (rows: sy from Y, resy / oh) and the nets see x = sx / half_main - 1, y = sy / half_main - 1 in fp32 with half_main = max(resx, resy) / 2
 * of the stage-1 lattice, and the frame's t.  The clamp is cv2.resize's border rule: the nets stay inside the lattice they were fitted
 * on.  With oh == resy and ow == resx the result is af_render_frame's bit for bit; for an odd integer factor k, output pixel
 * k*i + (k-1)/2 is lattice pixel i.
 * rgb_out (oh,ow,3) fp32 and u8_out (oh,ow,3) bytes (the truncating cast of af_render_frame_u8), each optional; ref_u8 (oh,ow,3) bytes,
 * optional, with sse_out = sum over the image of ((double)ref / 255 - (double)rgb)^2 (fp64, fixed summation order: two calls agree
 * bitwise).  on_device != 0: rgb_out, u8_out and ref_u8 are device pointers on the handle's device, else host pointers.  AF_EINVAL: frame
 * out of range, oh / ow out of range, nothing to do (the three pointers NULL), sse_out without ref_u8 or ref_u8 without sse_out.
 * The frame is processed in bands of at most resx * resy pixels: no more activation memory than af_render_frame.  Forward-only: the
 * training state and af_psnr's error cache are not touched, and no uploaded video is needed.  Returns host-synchronous. */
int af_render_frame_at(af_handle* h, int frame, int oh, int ow, float* rgb_out, uint8_t* u8_out, const uint8_t* ref_u8, double* sse_out,
                       int on_device);
/* Mean over frames of skimage PSNR(data_range=1) (evaluate.py:740-743,775); per_frame[F] optional. */
int af_psnr(af_handle* h, double* mean_psnr, double* per_frame);

/* ---- layer decomposition of a two_layer handle (src/models/stage_1/evaluate.py:24-200,300-438) ------------------------------
 * Forward-only; none of these touches the training state or the per-frame error af_psnr caches.
 *
 * af_render_layers: the layers of one frame (evaluate.py:302-337, 361-369): uv1 / uv2 (resy,resx,2) = the raw outputs of mapping1 /
 * mapping2, alpha (resy,resx) = 0.99 * 0.5(a+1) + 0.001 of the alpha net's output a, rgb1 / rgb2 (resy,resx,3) = (t+1)/2 of the atlas at
 * uv1*0.5+0.5 / uv2*0.5-0.5.  Every pointer may be NULL (not written).  A single-atlas handle has uv1, rgb1 and alpha == 1 only (uv2 / rgb2
 * non-NULL: AF_EINVAL); its rgb1 is af_render_frame's rgb bit for bit, and on a two_layer handle af_render_frame's rgb is
 * rgb1*alpha + rgb2*(1-alpha) of these values.  Needs no uploaded video. */
int af_render_layers(af_handle* h, int frame, float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2);
/* af_mapping_area: get_mapping_area (evaluate.py:142-190) over all F x resy x resx pixel-frames, coordinates normalised by the larger
 * side and t = f/(F/2) - 1 in fp32 (:160-162).  which = 0: foreground, the uploaded fg mask > 0.5 and a > 0.95, uv1*0.5+0.5
 * (:239-243); which = 1: background, every pixel with -a > -0.5, uv2*0.5-0.5 (:235-238).  a is the RAW alpha-net output.
 * out5 = {maxx, minx, maxy, miny, edge}: min starts at 1 and max at -1, both clamped to [-1, 1], edge = max(maxx-minx, maxy-miny) —
 * an empty selection returns (-1, 1, -1, 1, -2).  two_layer handle with an uploaded video only (AF_ESTATE otherwise). */
int af_mapping_area(af_handle* h, int which, float out5[5]);
/* af_render_atlas_texture: texture_orig of get_high_res_texture (evaluate.py:87-104, without the cv2.putText overlay): out (res,res,3)
 * = (atlas(x, y) + 1)/2 with x = torch.linspace(minx, minx+edge, res)[column], y = torch.linspace(miny, miny+edge, res)[row] in
 * torch's fp32 arithmetic.  1 <= res <= 16384.  Any handle; needs no video. */
int af_render_atlas_texture(af_handle* h, int res, float minx, float miny, float edge, float* out);
/* af_render_edit: texture-edit propagation of one frame (evaluate.py:373-438 with get_colors / bilinear_interpolate_numpy :24-84).
 * Layer fg samples tex_fg (res,res,3) at (uv1*0.5+0.5 - min) * res/edge of its window win_fg = {minx, miny, edge}, layer bg tex_bg at
 * uv2*0.5-0.5 in win_bg; "relevant" pixels as get_colors defines them.  edit_fg = rgb_fg*alpha, edit_bg = rgb_bg, edit = the sum of
 * rgb_fg*alpha and rgb_bg*(1-alpha) over the relevant layers; 0 where a pixel is not relevant (all (resy,resx,3)).
 * use_fg / use_bg (res,res): texel usage ACCUMULATED into the caller's arrays (zero them before the first frame): use_fg = max of alpha
 * over the floor/ceil texels of every relevant pixel (the true maximum; the reference's fancy-indexed assignment keeps the last of
 * duplicate texels instead), use_bg = 1 on any use.  A layer with a NULL window is skipped; a NULL texture with a window
 * gives the usage masks only (edit / that layer's edit_* must then be NULL).  two_layer handle only (AF_ESTATE). */
int af_render_edit(af_handle* h, int frame, int res, const float* tex_fg, const float win_fg[3], const float* tex_bg, const float win_bg[3],
                   float* edit, float* edit_fg, float* edit_bg, float* use_fg, float* use_bg);

/* ---- layers and texture edits at any size ------------------------------------------------------------------------------------
 * The layer products above on an oh x ow grid (1..16384 each) instead of the stage-1 lattice: the geometry, the bands of at most
 * resx * resy pixels and the activation memory are the ones of the render at another size (see its comment above), the values the ones
 * of the lattice calls.  Forward-only, in every mlp_mode; no uploaded video is needed; the training state and the error cache of the PSNR
 * call are not touched.  With oh == resy and ow == resx every float output is the lattice call's bit for bit; for an odd integer factor k,
 * output pixel k*i + (k-1)/2 is lattice pixel i.  All return host-synchronous.
 *
 * af_render_layers_at: uv1 / uv2 (oh,ow,2), alpha (oh,ow), rgb1 / rgb2 (oh,ow,3) as the lattice call defines them, and alpha_u8 (oh,ow)
 * = (uint8)(int)((double)alpha * 255), the byte written to alpha/%05d.png.  Every pointer may be NULL, not all of them (AF_EINVAL).
 * on_device != 0: every pointer is a device pointer on the handle's device, else a host pointer.  A single-atlas handle has uv1, rgb1
 * and alpha == 1 (alpha_u8 == 255); uv2 / rgb2 non-NULL: AF_EINVAL.  AF_EINVAL also for a frame, oh or ow out of range. */
int af_render_layers_at(af_handle* h, int frame, int oh, int ow, float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2,
                        uint8_t* alpha_u8, int on_device);
/* Edit sessions: the texture-edit propagation of the lattice call with the textures and the usage masks kept on the device, so a clip
 * uploads its textures once and no mask crosses the bus per frame.  A session holds textures, windows and usage masks only; the nets are
 * the handle's at the time of each frame call, so a fit may go on between calls.
 *
 * af_edit_create: host textures tex_fg / tex_bg (res,res,3) and windows {minx, miny, edge} under the lattice call's rules: a layer
 * without a window is skipped, a window without a texture gives usage masks only, a texture without its window is AF_EINVAL, as are
 * res outside 1..16384 and two NULL windows.  The textures are copied into device memory the session owns (they may be freed when the
 * call returns); track_usage != 0 adds zeroed (res,res) usage masks on the device for every layer with a window.  two_layer handle
 * only (AF_ESTATE).
 * af_edit_frame: frame `frame` on an oh x ow grid.  edit, edit_fg, edit_bg (oh,ow,3) fp32 as the lattice call defines them, edit_u8
 * (oh,ow,3) = (uint8)(int)((double)edit * 255) (textures are expected in [0, 1]); each may be NULL, and at least one output or usage
 * tracking is needed (AF_EINVAL).  edit_fg / edit_bg without that layer's texture, or edit / edit_u8 with a window that has no texture:
 * AF_EINVAL.  on_device != 0: device pointers on the handle's device.  With usage tracking every call accumulates into the session's
 * masks: use_fg = max of alpha over the floor/ceil texels of every relevant fg pixel (an atomic max on the bits of alpha), use_bg = 1 on
 * any use (plain stores); both commute, so the masks are bitwise reproducible whatever the size, the banding and the order of calls.
 * af_edit_usage: the masks so far into host arrays (res,res), each may be NULL; a layer without a window gives zeros.  A session
 * without usage tracking: AF_ESTATE.  af_edit_reset_usage zeroes them.
 * af_edit_destroy frees the session.  Destroying the handle first is allowed: it frees the device memory of its live sessions and
 * marks them dead; every later session call then returns AF_ESTATE (message: the error call with a NULL handle), and af_edit_destroy
 * only frees the host struct. */
typedef struct af_edit af_edit;
int af_edit_create(af_handle* h, int res, const float* tex_fg, const float win_fg[3], const float* tex_bg, const float win_bg[3],
                   int track_usage, af_edit** out);
int af_edit_frame(af_edit* e, int frame, int oh, int ow, float* edit, float* edit_fg, float* edit_bg, uint8_t* edit_u8, int on_device);
int af_edit_usage(af_edit* e, float* use_fg, float* use_bg);
int af_edit_reset_usage(af_edit* e);
void af_edit_destroy(af_edit* e);

/* ---- per-pixel loss maps (src/models/stage_1/evaluate.py:338-384 fg/bg, :650-705 single) -----------------------------------
 * af_render_loss_maps: the maps evaluate.py computes for visualisation, for every pixel of one frame.  Each output is [resy][resx] fp32
 * (residual: [resy][resx][3]); NULL outputs are not written and the rows only they need are not evaluated.  Forward-only: the
 * training state and af_psnr's cache do not move.
 *   rigidity1/2  get_rigidity_loss(return_all) of mapping1 / mapping2 with derivative_amount (loss_utils.py:227-280)
 *   flow1/2      get_optical_flow_loss_all (loss_utils.py:283-296) with the uploaded forward flow and mask: the uv distance to the flow
 *                target (x + fx, y + fy, f + 1) times larger_dim / (2 uv_mapping_scale), 0 where the mask is 0, times alpha (flow1) /
 *                1 - alpha (flow2); alpha = 1 on a single-atlas handle.  0 on the last frame (evaluate.py:374-376, :692)
 *   flow_alpha   get_optical_flow_alpha_loss_all (loss_utils.py:412-424): |alpha - alpha(target)|, 0 where the mask is 0 (every frame)
 *   rgb_err      ||frame - rgb||^2 and residual = frame - rgb, rgb = af_render_frame's reconstruction
 * Single-atlas handle: rigidity2, flow2 and flow_alpha must be NULL.  AF_EINVAL also for a frame out of range or no uploaded video. */
int af_render_loss_maps(af_handle* h, int frame, float* rigidity1, float* rigidity2, float* flow1, float* flow2,
                        float* flow_alpha, float* rgb_err, float* residual);

/* ---- warping error E_warp (Lai et al., ECCV 2018; building blocks: src/models/utils.py:478-572) -----------------------------
 * Pair (I_t = img1, I_{t+1} = img2, fw_t = flow12, bw_{t+1} = flow21), all HWC fp32 (flows in pixels, channel 0 = x):
 *   warped = flow_warping(img2, flow12) (:504-529): position (x + fx, y + fy) normalised by max(w - 1, 1) / max(h - 1, 1), then
 *            grid_sample bilinear with zero padding.  align_corners 1 ("exact"): zero flow is the identity; 0 ("reference"): what the
 *            reference's function computes under torch >= 1.3, whose grid_sample defaults to align_corners=False.
 *   noc    = 1 - detect_occlusion(flow21, flow12) (:532-572), on img1's grid: with A_w = flow_warping(flow21, flow12),
 *            |A_w + B|^2 > 0.01 (|A_w|^2 + |B|^2) + 0.5 or the motion-boundary test of B = flow12 (fp64 gradient terms) occludes.
 *   err    = sum_p,c noc (warped - img1)^2 / (3 sum_p noc); 3 h w in the denominator when every pixel is occluded (err is then 0).
 * Accumulated in fp64 from fixed per-block partials in a fixed order: two calls are bitwise equal.
 *
 * af_warp_error_pair: stateless, like af_resize_bilinear.  With on_device != 0 every pointer is a device pointer, else host.  noc
 * ([h][w], 0 / 1) and warped ([h][w][3]) may be NULL.  AF_EINVAL for h or w < 2, a NULL input or err, or align_corners not 0 / 1.
 * af_warp_error: E_t of every consecutive pair of the handle's video, with the uploaded flows (optical_flows of frame t,
 * optical_flows_reverse of frame t+1) in every mlp_mode, on single and two_layer handles.  which 0: the uploaded frames; which 1: the
 * reconstruction, af_render_frame's rgb bit for bit.  per_pair ([F-1]) and mean (the mean of the E_t) may be NULL.  Forward-only: the
 * training state and af_psnr's cache do not move.  AF_EINVAL for a bad which / align_corners or F < 2; AF_ESTATE with no video. */
int af_warp_error_pair(int device_ordinal, const float* img1, const float* img2, const float* flow12, const float* flow21, int h, int w,
                       int align_corners, double* err, float* noc, float* warped, int on_device);
int af_warp_error(af_handle* h, int which, int align_corners, double* per_pair, double* mean);

int af_sync(af_handle* h);

/* ---- stage 2: neural filter + local refinement (src/neural_filter_and_refinement.py:44-130) ------------------------------
 * An af_filter handle is independent of af_handle: one video size on one device, both nets of stage 2 in eval mode, and the
 * recurrence state of the frame loop.  h, w: the original frame size; the handle pads to Hp x Wp, the next multiples of 32
 * (InputPadder mode 'other', replicate: (Wp - w) / 2 columns on the left, the rest on the right, all rows at the bottom).
 * Errors of these calls are reported through af_last_error(NULL) on the calling thread.
 * net 0: UNet(6, 3, 32) (src/models/network_filter.py); net 1: TransformNet(nf 32, blocks 5, nc_in 12, nc_out 3)
 * (src/models/network_local.py).  flat: the state_dict in its own order with the InstanceNorm buffers dropped
 * (*.norm_layer.running_mean / running_var / num_batches_tracked: the nets never apply them), weights OIHW as torch stores them.
 * af_filter_frame: content / style HWC fp32 at (h, w) (the input frame and the stage-1 frame, both / 255, style resized to the
 * content's size); pred_out / final_out (either may be NULL) receive HWC fp32 at (Hp, Wp), unclamped: pred = UNet(cat(content,
 * style)); frame 0 after create / reset: final = pred; later frames: final = pred + TransformNet(cat(pred, o1, pred, p1)) with
 * p1 = the previous pred and o1 = the previous final.  on_device != 0: every pointer is a device pointer on the handle's GPU.
 * AF_ESTATE before both nets' parameters are set.
 * af_filter_debug_activation: a named intermediate of the last frame as HWC fp32, n = its exact size: input (Hp, Wp, 6), enc1..enc4,
 * bottleneck, dec4..dec1, pred (UNet); E1a, E1b, E2a, E2b, E3, RB, hidden, D2, D1, Y (TransformNet, AF_ESTATE when the last frame
 * was a frame 0); final.  Level l of the pyramid is (Hp >> l, Wp >> l).
 * af_conv2d: one convolution as the nets run it, stateless: x (h, w, cin) HWC, weight (cout, cin, k, k), bias (cout) or NULL,
 * padding k / 2 (pad_mode 0 zeros, 1 reflection), k in {1, 3, 7}, stride 1 or 2, act 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 tanh,
 * residual (ho, wo, cout) or NULL added after the activation, y (ho, wo, cout) with ho = (h - 1) / stride + 1 (likewise wo).
 * Precision mode (opt-in; AF_FILTER_FP32 is the default and keeps its bits): AF_FILTER_FP16 is both nets as the reference's modules
 * compute them under fp16 autocast.  Every convolution rounds its operands to fp16 as it gathers them (nearest even, subnormals kept,
 * overflow to inf), accumulates the exact products in fp32 on v_mfma_f32_32x32x16_f16 and gives y = fp16(sum + fp16(bias)); the
 * activation is evaluated in fp32 on y and rounded to fp16 once, a residual is added after that and the sum rounded once.  The
 * bilinear upsampling rounds once, the LSTM finish after each step (both gates, tanh(cell gate), cell, hidden), final = fp16(pred + Y);
 * the padding, packing, pooling and nearest upsampling move values.  Buffers and outputs stay fp32 and hold fp16-representable values;
 * nothing is clamped (overflow gives inf, as torch's cast does); frame 0 still has final == pred bit for bit.
 * af_filter_set_precision: allowed at any time (both weight images are resident once the parameters are set) and performs
 * af_filter_reset: the next frame is a frame 0.  AF_EINVAL for any other value, and then nothing changes.
 * af_conv2d_prec: af_conv2d with a leading precision argument; in AF_FILTER_FP16 the tile packs a pixel's row and column into 16 bits
 * each, so h, w <= 16384 (AF_EINVAL beyond; af_filter_create has the same limit in either mode). */
typedef struct af_filter af_filter;
enum { AF_FILTER_FP32 = 0, AF_FILTER_FP16 = 1 };
int af_filter_create(int device_ordinal, int h, int w, af_filter** out);
void af_filter_destroy(af_filter* f);
size_t af_filter_param_count(const af_filter* f, int net);
int af_filter_set_params(af_filter* f, int net, const float* flat, size_t n);
int af_filter_reset(af_filter* f);
int af_filter_frame(af_filter* f, const float* content, const float* style, float* pred_out, float* final_out, int on_device);
int af_filter_debug_activation(af_filter* f, const char* name, float* out, size_t n);
int af_conv2d(int device_ordinal, const float* x, int h, int w, int cin, const float* weight, const float* bias, int cout, int k, int stride,
              int pad_mode, int act, const float* residual, float* y, int on_device);
int af_filter_set_precision(af_filter* f, int precision);
int af_filter_get_precision(const af_filter* f, int* precision);
int af_conv2d_prec(int precision, int device_ordinal, const float* x, int h, int w, int cin, const float* weight, const float* bias, int cout, int k,
                   int stride, int pad_mode, int act, const float* residual, float* y, int on_device);

/* ---- optical-flow precompute: RAFT forward (raft.hip; reference: src/preprocess_optical_flow.py, src/models/stage_1/core) ----
 * An opaque handle independent of af_handle and af_filter: RAFT "basic" (small=False), forward only, test mode, in fp32 (what the
 * reference computes on a CPU; on a GPU it runs under fp16 autocast).  Frames of (h, w) are padded as InputPadder mode 'sintel' does
 * (replicate, pad / 2 before, the rest after, both axes to multiples of 8) to (Hp, Wp), and the flow keeps the padded size, as the
 * reference's saved .npy files do.  AF_EINVAL for Hp < 128 or Wp < 128 (the reference's own flow is NaN there).
 * capacity = pair-directions run per batch; the handle has 2 * capacity frame slots.
 * af_raft_set_params: flat fp32 in the reference's state_dict order, BatchNorm running_mean / running_var included,
 * num_batches_tracked excluded (cnet's downsample.1.* repeat norm3.* as the state_dict does).
 * af_raft_encode: image (h, w, 3) HWC fp32 with values 0..255 -> slot: one fnet and one cnet pass.
 * af_raft_flow: n <= capacity pair-directions slot_a[i] -> slot_b[i] in one batch, iters update steps; flow_up (n, Hp, Wp, 2) and
 * flow_lo (n, Hp / 8, Wp / 8, 2) (either may be NULL), (x, y) displacement.  on_device != 0: image / flow pointers are device pointers.
 * af_raft_step: one update iteration of slot_a -> slot_b from a given state (net (P, 128), coords1 (P, 2), host, P = Hp / 8 * Wp / 8).
 * af_raft_lookup: the 324-channel correlation lookup of slot_a -> slot_b at the given coords (P, 2) -> out (P, 324), host.
 * af_raft_debug_activation: a named intermediate of batch element 0 of the last flow / step / lookup call, (P, C) fp32, n its exact
 * size: fmap1, fmap2 (256), net0, inp (128), corr_l0..corr_l3 (81 each: the last lookup), motion, net (128), delta, flow_lo (2),
 * mask (576), corr_vol0..corr_vol3 (the correlation pyramid, C = grid positions of that level).
 * af_raft_conv2d / af_raft_gru / af_raft_instance_norm: the building blocks stand-alone on host tensors (NHWC): a convolution with a
 * kh x kw kernel (odd, <= 7), padding k / 2, act 0 none, 1 ReLU, 3 tanh, 4 sigmoid, over a batch of images; one half of SepConvGRU
 * (vertical = 0: 1x5, 1: 5x1) on net (M, 128) and x (M, 256) with the reference's OIHW weights; InstanceNorm2d (+ ReLU, + residual
 * as relu(residual + y)) for c in {64, 96, 128}.
 * Precision mode (opt-in; AF_RAFT_FP32 is the default and keeps its bits): AF_RAFT_FP16 is the arithmetic the reference runs on a GPU,
 * both encoders and the update block under fp16 autocast.  Every convolution of fnet, cnet and the update block rounds its operands to
 * fp16 (nearest even, subnormals kept, overflow to inf), accumulates the exact products in fp32 on v_mfma_f32_32x32x16_f16, and rounds
 * sum + bias, and the activation's result, to fp16; the GRU gates, r * h and the new hidden state and the norms' outputs are rounded
 * once each.  Buffers stay NHWC fp32 (holding fp16-representable values); the correlation volume, pooling, lookup, coords1 += delta,
 * flow = coords1 - coords0 and the convex upsampling stay fp32, as in the reference.  Setting the precision is allowed at any time and
 * invalidates the encoded slots (both weight images are resident); AF_EINVAL for any other value.  In this mode the step call
 * rounds the incoming net to fp16.  The three *_prec calls are the stand-alone building blocks with a leading precision argument. */
typedef struct af_raft af_raft;
enum { AF_RAFT_FP32 = 0, AF_RAFT_FP16 = 1 };
int af_raft_create(int device_ordinal, int h, int w, int capacity, af_raft** out);
void af_raft_destroy(af_raft* r);
size_t af_raft_param_count(const af_raft* r);
int af_raft_info(const af_raft* r, int* hp, int* wp, int* slots);
int af_raft_set_params(af_raft* r, const float* flat, size_t n);
int af_raft_encode(af_raft* r, int slot, const float* image, int on_device);
int af_raft_flow(af_raft* r, int n, const int* slot_a, const int* slot_b, int iters, float* flow_up, float* flow_lo, int on_device);
int af_raft_step(af_raft* r, int slot_a, int slot_b, const float* net, const float* coords1, float* net_out, float* delta_out);
int af_raft_lookup(af_raft* r, int slot_a, int slot_b, const float* coords, float* out);
int af_raft_debug_activation(af_raft* r, const char* name, float* out, size_t n);
int af_raft_conv2d(int device_ordinal, const float* x, int batch, int h, int w, int cin, const float* weight, const float* bias, int cout, int kh, int kw,
                   int stride, int act, float* y);
int af_raft_gru(int device_ordinal, int batch, int h, int w, int vertical, const float* net, const float* x, const float* wz, const float* bz, const float* wr,
                const float* br, const float* wq, const float* bq, float* net_out);
int af_raft_instance_norm(int device_ordinal, const float* x, int h, int w, int c, int relu, const float* residual, float* y);
int af_raft_set_precision(af_raft* r, int precision);
int af_raft_get_precision(const af_raft* r, int* precision);
int af_raft_conv2d_prec(int precision, int device_ordinal, const float* x, int batch, int h, int w, int cin, const float* weight, const float* bias, int cout,
                        int kh, int kw, int stride, int act, float* y);
int af_raft_gru_prec(int precision, int device_ordinal, int batch, int h, int w, int vertical, const float* net, const float* x, const float* wz, const float* bz,
                     const float* wr, const float* br, const float* wq, const float* bq, float* net_out);
int af_raft_instance_norm_prec(int precision, int device_ordinal, const float* x, int h, int w, int c, int relu, const float* residual, float* y);

/* ---- test / measurement hooks (not part of the reference surface) --------------------------------- */
/* Run one net forward on caller rows: in [rows][4] host -> out [rows][4] host. */
int af_debug_forward(af_handle* h, int net, const float* in, int rows, float* out);
/* Debug: the tensors the LAST training step left in HBM for the weight-gradient GEMMs, as the kernels wrote them (per row tile of 32 rows):
 * which = 0 activation plane `layer` (relu(Z_layer) = X_{layer+1}, [256 features][32 rows]), 1 gradient plane (dZ_layer), 2 its sign-bit words
 * (copied as 256 x 32-bit per tile), 3 the PE features [64][32], 4 dZ of the output layer [32][32], 5 the xyt rows [32][32], 6 the net's output rows
 * [32 rows][4] (tanh of the output layer; columns past the net's outputs are 0), 7 the gradient on them [32 rows][4] as the backward chain's seed read it
 * (the loss kernels' rows plus, on the mapping nets, the atlas chain's input gradient), 8 the net's input rows [32 rows][4] as the batch preparation
 * wrote them ((x, y, t, 0); AF_EINVAL for the atlas net, whose input is the mapping nets' output) -- all three row-major, read-only copies.  nt_stride = row tiles per
 * plane of that step (ceil(rows of the net's batch / 32)); `ntiles` tiles from `tile0` go to out.  What tests/test_gpu_gemm_error.py measures the
 * per-layer error of each arithmetic on: one layer's product recomputed in fp64 from the kernel's OWN inputs against the kernel's output. */
int af_debug_tiles(af_handle* h, int net, int which, int layer, int nt_stride, int tile0, int ntiles, float* out);
/* The launch plan of the single-atlas step for a chip of `ncu` compute units (pure arithmetic, no GPU needed):
 * out3 = {T1, T2, NT}: mapping row tiles [0,T1) form launch 1, [T1,T2) lead and [T2,NT) trail the atlas part of
 * launch 2 (DESIGN.md §2.1 "Packed launches"). */
int af_debug_plan(int ncu, int rows_map, int rows_atlas, int dep_rows, int out3[3]);
/* Balance diagnostics of k_dw: enable != 0 makes every later k_dw launch record s_memrealtime (100 MHz) at the start and
 * end of each workgroup; out (nullable) receives [min(cap_wg, #CUs)][2] values of the most recent launch.  Returns #CUs. */
int af_debug_dw_clocks(af_handle* h, int enable, uint64_t* out, int cap_wg);
/* The clock each hot kernel runs at INSIDE the training step: enable != 0 makes the five hot launches of every later step (forward 1, 2,
 * backward 1, 2 of the chains in any mlp_mode, k_dw) record per workgroup {s_memrealtime, s_memtime} at its start and at its end; out
 * (nullable) receives [5][min(cap_wg, 4096)][4] uint64 of the most recent step (zeros for workgroups a launch did not have) and the
 * buffer is cleared.  Only the first 4096 workgroups of a launch are stamped (samples_batch 100 000 launches ~7 000 - 18 000; the rest
 * are skipped, nothing is written past a launch's region).  Ticks over the 100 MHz span = the shader clock under that launch's load
 * (tools/step_clock.py).  Returns 4096 (the cap, not a grid size). */
int af_debug_step_clocks(af_handle* h, int enable, uint64_t* out, int cap_wg);
/* The static split-K schedule of k_dw: which = 0 (9 row segments), 1 (7), 2 / 3 (pre-train of mapping1 / mapping2).
 * out (nullable) [min(cap_wg, #workgroups)][16][4] int32 = {job shape 0..4 (8x8, 8x2, 8x1, 1x8, 1x2; -1 ends a list), first row tile,
 * one past the last, job index}.  Returns the number of workgroups.  Used by tools/dw_fit.py to fit the schedule's cost model. */
int af_debug_dw_schedule(af_handle* h, int which, int32_t* out, int cap_wg);
/* Read back n 64-byte pixel records of the packed table: out [n][16] = rgb(3), d/dx rgb(3), d/dy rgb(3), fwd flow(2),
 * bwd flow(2), fwd mask, bwd mask, fg mask, for pixel-frame indices inds[n] (the k of get_tuples' column k). */
int af_debug_records(af_handle* h, const int64_t* inds, int n, float* out);
/* Arithmetic of the weight-gradient GEMMs (k_dw), for the loop AND for pre_train_mapping's dW: 1 (default) = fp32-faithful
 * "bf16x6" — each fp32 operand split in registers into three bf16 values, the six leading partial products accumulated in
 * fp32 on the bf16 matrix pipe (dropped terms <= 2^-23 relative: tests/test_split_precision.py).  2 (opt-in) = "bf16x3" —
 * two bf16 values per operand (16 mantissa bits), three partial products: NARROWER than the reference's fp32, faster,
 * measured within 3x of torch-fp32's own gradient error against an fp64 twin at full size (tests/test_gpu_fullsize.py);
 * never the default and never bench.py's headline value.  0 = the fp32 matrix pipe (v_mfma_f32_32x32x2_f32).  The three
 * are held against each other in tests/test_gpu_dw_modes.py.  The library reads no environment: the Python mirror maps
 * AF_DW_MODE=<m> / AF_DW_FP32=1 onto this call for the A/B tools.
 * A switch re-cuts all split-K schedules (their tile costs belong to the arithmetic). */
int af_set_dw_mode(af_handle* h, int mode);
/* Experiments and the partition-sensitivity tests: replace the per-shape tile costs k_dw's static split-K schedule is cut with
 * (cost5 = 8x8, 8x2, 8x1, 1x8, 1x2 tiles; every value finite and > 0, ratios <= 1000:1; seg_cost <= 0 keeps the shipped per-segment
 * cost) and re-cut all schedules; cost5 == NULL returns to the shipped row of the current arithmetic.  Another row = another
 * partition of the row batch over workgroups = another summation ORDER of the same partial products, nothing else; results stay
 * bit-reproducible for a given row.  AF_EINVAL (handle unchanged) for a row that is not valid or cannot be scheduled. */
int af_debug_set_dw_cost(af_handle* h, const double* cost5, double seg_cost);
/* The same choice for the 256x256 hidden-layer products of the forward / backward chains: 3 (default since round 6) = "f16x3" (mlphf.hip): every
 * operand as two fp16 terms of its scaled value, three products on v_mfma_f32_32x32x16_f16, a power-of-two scale per ROW and layer on the activations /
 * gradients and a fixed 2^12 on the weights — measured from the kernels' own tiles, its per-layer error against fp64 is below an fp32 fmaf chain's
 * (tests/test_gpu_gemm_error.py); af_train_steps / af_pretrain return AF_ERANGE once a hidden-layer weight reaches |w| >= 8 (the images stay finite up
 * to 16; mode 1 has no such limit).  1 = bf16x6 (mlpbf.hip: three bf16 terms, six products; the default of rounds 2-5), 0 = fp32 matrix pipe (mlp.hip),
 * 2 = bf16x6 forward with the backward chain (dX = W^T dZ) on three products of two-bf16 operands — a measured experiment, narrower than fp32.
 * k_adam maintains the 16-bit weight streams of the mode in force only; a switch between the stream families re-emits them (synchronises the stream).
 * (Python mirror: AF_EXPERIMENT=1 AF_MLP_MODE=<m> maps onto this call; AF_MLP_FP32=1 selects 0.)
 * pre_train_mapping's MLP chains run the f16x3 32-row chains in mode 3 (mlphf.hip) and the fp32 16-row kernels (mlp16.hip) in modes 0-2; its
 * weight-gradient GEMM follows af_set_dw_mode. */
int af_set_mlp_mode(af_handle* h, int mode);
/* The arithmetic modes in force (either pointer may be NULL): what the host side records next to its results. */
int af_get_modes(const af_handle* h, int* mlp_mode, int* dw_mode);
/* After af_train_steps / af_pretrain with debug enabled: reduced gradient of the last step, flat order. */
int af_set_debug(af_handle* h, int enable);
int af_get_last_grads(af_handle* h, int net, float* flat, size_t n);
/* Time the most recent launches: accumulated HIP-event milliseconds, launch counts and algorithmic FLOPs per
 * launch class since the last reset: [0]=prep [1]=fwd_1 [2]=fwd_2 [3]=loss [4]=bwd_1 [5]=bwd_2 [6]=dw [7]=adam.
 * A step has two forward and two backward MLP launches: fwd_1 = the mapping batch's whole rounds (two_layer:
 * alpha + both mappings), fwd_2 = atlas + the remainder; bwd_1 = atlas + remainder, bwd_2 = the rest.
 * ms16[16], counts16[16], flops16[16] (any may be NULL).
 * Bits 16..23 of class_mask: sample period P (0 or 1 = every step) - only the launches of every P-th step of an af_train_steps call
 * (its first step, its (P+1)-th, ...) carry events: a HIP event costs ~5 us in-stream, so timing two launches of every step of a
 * 1.1 ms step slows it by ~1.8 %; counts16 / flops16 cover exactly the launches that were timed. */
int af_set_timing(af_handle* h, int class_mask);   /* bit i (0..15) enables HIP-event timing of launch class i */
int af_get_timing(af_handle* h, double* ms16, int64_t* counts16, double* flops16, int reset);
/* Algorithmic work of ONE train step at the given iteration: MLP rows per net (indexed by af_net) and the
 * fwd+bwd FLOPs of the step. */
int af_step_work(const af_handle* h, int iter, int64_t rows4[4], double* flops);

#ifdef __cplusplus
}
#endif
#endif
