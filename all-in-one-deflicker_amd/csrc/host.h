// host.h — what the three host units of libatlasfit.so share: the fit handle and its parts, the error macros, the timing classes and the
// few functions that cross from the training side (host.hip) to the renders and measurements of a fitted handle (host_render.hip) and to
// the handle-free utilities (host_util.hip).  Nothing here is part of the ABI (include/atlasfit.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/atlasfit.h"
#include "af_dev.h"
#include "elem.h"

// A net's weight streams for one 16-bit chain family (bf16x6: mlpbf.hip, f16x3: mlphf.hip): byte offsets of its forward / backward stream in
// the family's stream buffers and, per layer, of its 256x256 block (-1: none) and of its fp32 block (layer 0 / skip columns / output layer; -1: none)
struct StreamPlan {
  size_t f_base = 0, b_base = 0;
  long long f_hid[AF_MAX_LAYERS], f_fp[AF_MAX_LAYERS], b_hid[AF_MAX_LAYERS], b_fp[AF_MAX_LAYERS];
};

struct NetDesc {
  int kern = -1;                                        // kernel kind (af_dev.h): the net id, or AF_KIND_MAP_PE for a mapping net with positional encoding
  int id = -1, NL = 0, in_kind = 0, in_feat0 = 0, out = 0, pe_feats = 0, pe_kind = 0;
  unsigned skip = 0; bool dx0 = false; bool used = false;
  int in_feat[AF_MAX_LAYERS], out_feat[AF_MAX_LAYERS];
  size_t w_off[AF_MAX_LAYERS], b_off[AF_MAX_LAYERS];   // within the net's flat params
  size_t nparams = 0, p_base = 0;                       // p_base: offset in the global flat buffer
  // Hidden width of the net as configured (number_of_channels_*).  The chains, tiles and split-K jobs are built around AF_HID = 256 units;
  // a narrower net runs EXACTLY inside them: units hid..255 carry zero weights and biases, so they output relu(0) = 0, receive the gradient
  // W^T dZ = 0, produce dW rows / columns of exact zeros, and Adam moves a zero-gradient, zero-moment parameter by lr * 0 / (0 + eps) = 0 —
  // they stay zero for ever.  Only the ABI's flat parameter order differs: lmap[i] = physical index of logical parameter i (state_dict
  // order of the hid-wide IMLP, implicit_neural_networks.py:43-51); empty when hid == AF_HID.
  int hid = AF_HID; size_t nlogical = 0; std::vector<uint32_t> lmap;
  // images (float offsets into the global image buffers)
  size_t f_off[AF_MAX_LAYERS]; int f_mpad[AF_MAX_LAYERS], f_groups[AF_MAX_LAYERS];
  long long b_off_img[AF_MAX_LAYERS]; int b_mpad[AF_MAX_LAYERS];
  size_t f_base = 0, b_base = 0, bias_base = 0;        // float offsets of this net's region (chunk offsets are relative to these)
  std::vector<AfChunk> fchunks, bchunks;               // the planned chunk sequences (checked against the kernels' ChunkBytes)
  StreamPlan bf, hf;                                    // weight streams of the bf16x6 and the f16x3 chains
  // activations
  int nt_cap = 0;
  float *coords = nullptr, *x0_tile = nullptr;         // input rows [rows_pad][4] (+ T-layout copy for the layer-0 dW of xyt nets)
  float *acts = nullptr, *dz = nullptr, *dz_last = nullptr, *pe_tile = nullptr, *out_buf = nullptr, *dout = nullptr;
  uint32_t* masks = nullptr;
};

struct Sched {
  std::vector<DwJob> jobs; std::vector<AdamJob> ajobs; std::vector<DwSeg> segs;
  int nwg = 0; size_t partial_floats = 0;
  DwJob* d_jobs = nullptr; AdamJob* d_ajobs = nullptr; DwSeg* d_segs = nullptr;
};

struct TimedEv { int cls; hipEvent_t a, b; };

// An edit session (include/atlasfit.h af_edit_create): textures, windows and usage masks in device memory of its own; the nets are the
// handle's at each call.  h == nullptr: the handle was destroyed, the device memory went with it and only the host struct is left.
struct af_edit {
  af_handle* h = nullptr;
  int res = 0; bool track = false;
  bool have_win[2] = {false, false}; float win[2][3] = {{0, 0, 0}, {0, 0, 0}};
  float* tex[2] = {nullptr, nullptr};      // (res, res, 3) or nullptr
  float* use[2] = {nullptr, nullptr};      // (res, res) or nullptr
};

struct af_handle {
  af_config cfg;
  bool seg = false;                   // two_layer: four nets (stage1_neural_atlas_seg.py), else two
  int device = 0; hipStream_t stream = nullptr; int ncu = 256;
  std::string err;
  NetDesc nets[AF_MAX_NETS];
  size_t total_params = 0, img_f_floats = 0, img_b_floats = 0, bias_floats = 0, sf_bytes = 0, sb_bytes = 0;
  char *img_sf = nullptr, *img_sb = nullptr;   // bf16x6 chain streams
  char *img_hf = nullptr, *img_hb = nullptr; size_t hf_bytes = 0, hb_bytes = 0;   // f16x3 chain streams (mlphf.hip)
  int mlp_mode = 3;                            // MLP chains: 3 = f16x3, the default since round 6: hidden layers on the fp16 matrix pipe, two-term fp16 split with a scale
                                               // per row, three products, both directions (mlphf.hip); 1 = bf16x6 on the bf16 pipe (mlpbf.hip, the default of rounds 2-5);
                                               // 2 = as 1 with the backward chain on three bf16 products (experiment); 0 = fp32 MFMA (mlp.hip)
  float *params = nullptr, *adam_m = nullptr, *adam_v = nullptr, *pre_m = nullptr, *pre_v = nullptr, *grads = nullptr;
  float *img_f = nullptr, *img_b = nullptr, *bias_img = nullptr;
  long long adam_step = 0;
  // video
  float* table = nullptr; bool have_video = false;
  // batch
  int N = 0;
  float *samples = nullptr, *loss_part = nullptr, *loss_log = nullptr;
  int* counts = nullptr; int loss_nblk_cap = 0; size_t loss_log_cap = 0;
  int* nan_flag = nullptr;                    // sticky, set on the device by k_adam: a non-finite parameter, a NaN loss term or an empty flow-match set
  int cur_nseg = 0;
  // compaction of the flow-match rows (k_prep): per-sample ranks, look-back scan slots, live match count, launch epoch
  int* flow_rank = nullptr; unsigned long long* scan = nullptr; int* live = nullptr; uint32_t prep_epoch = 0; unsigned long long prep_tickets = 0;
  unsigned long long* nvalid = nullptr; double p_valid[2] = {1.0, 1.0};     // share of the video's pixels with a valid fwd / bwd match
  int plan_flow_rows = 0;                                                   // flow-match rows the launches and the dW schedule are balanced for
  // schedules: 0 = 9 segments, 1 = 7 segments, 2 = pretrain mapping1, 3 = pretrain mapping2
  Sched sched[4]; float* partial = nullptr; size_t partial_cap = 0;
  unsigned long long* dw_clock = nullptr;     // af_debug_dw_clocks: per-workgroup start/end times of the last k_dw launch
  unsigned long long* step_stamp = nullptr;   // af_debug_step_clocks: [5 launches: fwd_1, fwd_2, bwd_1, bwd_2, dw][AF_STAMP_WG][4] of the last step
  // render
  int render_rows_cap = 0; float *r_coords = nullptr, *r_uv = nullptr, *r_uv2 = nullptr, *r_al = nullptr, *r_t = nullptr, *r_rgb = nullptr; double* r_sse = nullptr;
  unsigned char* r_at = nullptr;      // the frame renders' staging of one band's host u8_out and ref_u8 ([2][resy*resx][3]), allocated on first use
  std::vector<double> frame_sse; std::vector<char> frame_sse_valid;
  float* l_buf = nullptr; size_t l_cap = 0;   // layer outputs / edit scratch (af_render_layers, af_mapping_area, af_render_edit; one band's host staging of the _at calls): grows on demand
  std::vector<af_edit*> sessions;             // live edit sessions (af_edit_create): af_destroy frees their device memory and marks them dead
  bool debug = false; unsigned timing = 0, timing_every = 1; bool timing_live = true;   // timing_every: af_set_timing's sample period; timing_live: this step of af_train_steps is a sampled one
  double flop_fwd[AF_MAX_NETS] = {0}, flop_dx[AF_MAX_NETS] = {0};     // algorithmic FLOPs per MLP row of each net as built (forward == dW; dX chain), BASELINE.md 3
  bool dw_cost_set = false; double dw_cost[5] = {0}, dw_seg_cost = 0;      // af_debug_set_dw_cost: an explicit tile-cost row for build_sched (validated there: finite, > 0)
  int dw_mode = 1;                            // k_dw arithmetic (dw.hip): 1 = bf16x6 (fp32-faithful, the default), 2 = bf16x3 (hi + mid bf16 per operand, three products; opt-in), 0 = fp32 MFMA
  std::vector<TimedEv> evs; double t_ms[16] = {0}, t_flops[16] = {0}; long long t_cnt[16] = {0};

  int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    err = buf;
    return code;
  }
};

#define HCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return h->fail(AF_EHIP, #x, e_); } while (0)
#define AF_TEX_MAX 16384      // largest texture side af_render_atlas_texture / af_render_edit accept
#define LCHK(x) do { int r_ = (x); if (r_ != 0) return h->fail(AF_EHIP, #x, (hipError_t)r_); } while (0)

// timing classes (include/atlasfit.h: af_get_timing): the two forward and the two backward launches of a step
enum { T_PREP = 0, T_FWD_1 = 1, T_FWD_2 = 2, T_LOSS = 3, T_BWD_1 = 4, T_BWD_2 = 5, T_DW = 6, T_ADAM = 7 };

template <class T> hipError_t dalloc(T** p, size_t n) { return hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)); }
inline int tiles_of(int rows) { return (rows + 31) / 32; }

struct FwdPart { int net; FwdArgs a; int rows_total; };

// host.hip
FwdArgs fwd_args(af_handle* h, NetDesc& n, const float* in, float* out, int NT, bool train);
int launch_fwd(af_handle* h, int cls, std::initializer_list<FwdPart> parts, bool train);
extern "C" void af_set_thread_error(const char* m);     // the message af_last_error(NULL) reports on this thread
// host_render.hip
int ensure_render(af_handle* h, int rows);
void edit_release(af_edit* e);
// host_util.hip
double warp_error_of(const double* part, int nblk, int npix);
