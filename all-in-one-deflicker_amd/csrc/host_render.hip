// host_render.hip — what a fitted handle renders and measures (include/atlasfit.h): frames, layers, atlas textures, texture edits and edit
// sessions, loss maps, the warping error and the PSNR.  Forward only: the chains run through fwd_args / launch_fwd of the training side
// (host.hip, host.h) on the handle's stream, in the handle's render buffers; no training state moves.
#include <string.h>
#include <cmath>

#include "host.h"

namespace {

// The forward chains over the first `n` rows of r_coords (evaluate.py:302-337 / :640-661): mapping1 -> r_uv, atlas -> r_t; two_layer:
// alpha -> r_al, mapping2 -> r_uv2, atlas rows of the fg layer then, NT*32 rows later, of the bg layer (NT = tiles_of(n)).  The caller
// has filled the rows (zero up to the tile padding) and sized the buffers (ensure_render).
int chains_over(af_handle* h, int n) {
  int rc;
  const int NT = tiles_of(n);
  FwdArgs fm = fwd_args(h, h->nets[AF_NET_MAP1], h->r_coords, h->r_uv, NT, false);
  if (!h->seg) {
    if ((rc = launch_fwd(h, T_FWD_1, {{AF_NET_MAP1, fm, n}}, false)) != 0) return rc;
    FwdArgs fa = fwd_args(h, h->nets[AF_NET_ATLAS], h->r_uv, h->r_t, NT, false);
    if ((rc = launch_fwd(h, T_FWD_2, {{AF_NET_ATLAS, fa, n}}, false)) != 0) return rc;
  } else {   // evaluate.py:302-337
    FwdArgs f2 = fwd_args(h, h->nets[AF_NET_MAP2], h->r_coords, h->r_uv2, NT, false);
    FwdArgs fl = fwd_args(h, h->nets[AF_NET_ALPHA], h->r_coords, h->r_al, NT, false);
    if ((rc = launch_fwd(h, T_FWD_1, {{AF_NET_ALPHA, fl, n}, {AF_NET_MAP1, fm, n}, {AF_NET_MAP2, f2, n}}, false)) != 0) return rc;
    FwdArgs fa = fwd_args(h, h->nets[AF_NET_ATLAS], h->r_uv, h->r_t, 2 * NT, false);
    fa.in1 = h->r_uv2; fa.split_row = NT * 32;
    if ((rc = launch_fwd(h, T_FWD_2, {{AF_NET_ATLAS, fa, 2 * NT * 32}}, false)) != 0) return rc;
  }
  return 0;
}

float frame_time(const af_handle* h, int frame) {
  return (float)((double)frame / (h->cfg.number_of_frames / 2.0) - 1.0);     // evaluate.py:656 / :313 compute t in Python floats
}

// k_frame_coords_at's rows of the pixels [r0, r0 + n) of an oh x ow grid at time t into r_coords, zero up to the tile padding.
int fill_rows(af_handle* h, float t, int oh, int ow, long long r0, int n) {
  CoordsAtArgs ca{};
  ca.coords = h->r_coords; ca.resx = h->cfg.resx; ca.resy = h->cfg.resy; ca.oh = oh; ca.ow = ow;
  ca.half_main = (float)(std::max(h->cfg.resx, h->cfg.resy) / 2.0); ca.t = t; ca.r0 = r0; ca.n = n; ca.n_pad = tiles_of(n) * 32;
  LCHK(af_launch_frame_coords_at(&ca, h->stream));
  return 0;
}

// The band loop of everything a handle renders of a frame: the rows of each band of at most resx*resy pixels of the oh x ow grid at time
// t through chains_over, then finish(r0, n, NT) on the band's chain outputs (r_uv, r_uv2, r_al, r_t), so the activation buffers are the
// ones a stage-1 frame uses; a band may start and end inside a line.  The lattice (oh == resy, ow == resx) is one band.  The caller has
// checked oh and ow.  Not synchronised.
template <class Finish>
int bands_over(af_handle* h, float t, int oh, int ow, Finish&& finish) {
  const int band = h->cfg.resx * h->cfg.resy;
  int rc = ensure_render(h, band); if (rc) return rc;
  const long long total = (long long)oh * ow;
  for (long long r0 = 0; r0 < total; r0 += band) {
    const int n = (int)std::min<long long>(band, total - r0);
    if ((rc = fill_rows(h, t, oh, ow, r0, n)) != 0) return rc;
    if ((rc = chains_over(h, n)) != 0) return rc;
    if ((rc = finish(r0, n, tiles_of(n))) != 0) return rc;
  }
  return 0;
}

// The reconstruction of a frame on an oh x ow grid, enqueued: k_frame_finish_at on each band, into device pointers (on_device) or through
// r_rgb / r_at to the host.  The error is measured against a uint8 image (ref_u8), against the record table from record rec0 on (rec0 >= 0:
// the lattice frame of an uploaded video, which is also rendered into r_rgb when no rgb_out asks for it) or not at all; with `part`, the
// block partials arrive there in band and block order once the stream is synchronised.
int frame_bands(af_handle* h, float t, int oh, int ow, float* rgb_out, uint8_t* u8_out, const uint8_t* ref_u8, long long rec0, int on_device,
                       std::vector<double>* part) {
  const int band = h->cfg.resx * h->cfg.resy;
  if (!on_device && (u8_out || ref_u8) && !h->r_at) HCHK(dalloc(&h->r_at, (size_t)band * 6));
  if (part) part->assign((size_t)(((long long)oh * ow + band - 1) / band) * ((band + 255) / 256), 0.0);
  size_t blk0 = 0;
  int rc = bands_over(h, t, oh, ow, [&](long long r0, int n, int NT) -> int {
    const size_t off = (size_t)r0 * 3;
    FinishAtArgs fa{};
    fa.out_atlas = h->r_t; fa.out_alpha = h->seg ? h->r_al : nullptr; fa.row2 = (size_t)NT * 32; fa.n = n;
    if (on_device) {
      fa.rgb_out = rgb_out ? rgb_out + off : nullptr; fa.u8_out = u8_out ? u8_out + off : nullptr; fa.ref = ref_u8 ? ref_u8 + off : nullptr;
    } else {
      fa.rgb_out = rgb_out ? h->r_rgb : nullptr; fa.u8_out = u8_out ? h->r_at : nullptr;
      if (ref_u8) {
        HCHK(hipMemcpyAsync(h->r_at + (size_t)band * 3, ref_u8 + off, (size_t)n * 3, hipMemcpyHostToDevice, h->stream));
        fa.ref = h->r_at + (size_t)band * 3;
      }
    }
    if (rec0 >= 0) { fa.table = h->table; fa.rec0 = (size_t)(rec0 + r0); if (!fa.rgb_out) fa.rgb_out = h->r_rgb; }
    fa.sse_part = part ? h->r_sse : nullptr;
    LCHK(af_launch_frame_finish_at(&fa, h->stream));
    if (part) { HCHK(hipMemcpyAsync(part->data() + blk0, h->r_sse, (size_t)((n + 255) / 256) * 8, hipMemcpyDeviceToHost, h->stream)); blk0 += (n + 255) / 256; }
    if (!on_device && rgb_out) HCHK(hipMemcpyAsync(rgb_out + off, h->r_rgb, (size_t)n * 12, hipMemcpyDeviceToHost, h->stream));
    if (!on_device && u8_out) HCHK(hipMemcpyAsync(u8_out + off, h->r_at, (size_t)n * 3, hipMemcpyDeviceToHost, h->stream));
    return 0;
  });
  if (part) part->resize(blk0);
  return rc;
}

// frame_bands, synchronised, with the partials summed on the host: the core of af_render_frame, af_render_frame_u8 and af_render_frame_at.
int render_frame_core(af_handle* h, int frame, int oh, int ow, float* rgb_out, uint8_t* u8_out, const uint8_t* ref_u8, long long rec0,
                             int on_device, double* sse_out) {
  std::vector<double> part;
  int rc = frame_bands(h, frame_time(h, frame), oh, ow, rgb_out, u8_out, ref_u8, rec0, on_device, sse_out ? &part : nullptr); if (rc) return rc;
  HCHK(hipStreamSynchronize(h->stream));
  if (sse_out) { double sse = 0; for (double v : part) sse += v; *sse_out = sse; }
  return AF_OK;
}

// af_render_frame and af_render_frame_u8: the lattice frame of an uploaded video, its error against the record table cached for af_psnr.
// `what` names the caller in the error messages.
int render_lattice_frame(af_handle* h, int frame, float* rgb_out, unsigned char* u8_out, int on_device, double* sse_out, const char* what) {
  if (!h) return AF_EINVAL;
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, (std::string(what) + ": frame index").c_str());
  if (!h->have_video) return h->fail(AF_ESTATE, (std::string(what) + ": no video uploaded").c_str());
  HCHK(hipSetDevice(h->device));
  double sse = 0;
  int rc = render_frame_core(h, frame, h->cfg.resy, h->cfg.resx, rgb_out, u8_out, nullptr, (long long)frame * h->cfg.resx * h->cfg.resy, on_device, &sse);
  if (rc) return rc;
  h->frame_sse[frame] = sse; h->frame_sse_valid[frame] = 1;
  if (sse_out) *sse_out = sse;
  return AF_OK;
}

int ensure_layers(af_handle* h, size_t floats) {
  if (floats <= h->l_cap) return 0;
  (void)hipFree(h->l_buf); h->l_buf = nullptr; h->l_cap = 0;
  HCHK(dalloc(&h->l_buf, floats));
  h->l_cap = floats;
  return 0;
}

// The layer products {uv1, uv2, alpha, rgb1, rgb2} of a frame on an oh x ow grid: k_layer_finish on each band.  Host outputs are staged one
// band at a time in l_buf ([11][band] floats, then the band's alpha bytes); device outputs are written in place.  Synchronised.
int layers_core(af_handle* h, int frame, int oh, int ow, float* const o[5], uint8_t* alpha_u8, int on_device) {
  const size_t band = (size_t)h->cfg.resx * h->cfg.resy;
  int rc;
  if (!on_device && (rc = ensure_layers(h, band * 11 + (band + 3) / 4)) != 0) return rc;
  const size_t w[5] = {2, 2, 1, 3, 3}, s0[5] = {0, 2, 4, 5, 8};
  rc = bands_over(h, frame_time(h, frame), oh, ow, [&](long long r0, int n, int NT) -> int {
    float* d[5]; unsigned char* d8 = nullptr;
    for (int k = 0; k < 5; ++k) d[k] = !o[k] ? nullptr : on_device ? o[k] + (size_t)r0 * w[k] : h->l_buf + s0[k] * band;
    if (alpha_u8) d8 = on_device ? alpha_u8 + r0 : (unsigned char*)(h->l_buf + 11 * band);
    LCHK(af_launch_layer_finish(h->r_uv, h->r_uv2, h->r_t, (size_t)NT * 32, h->seg ? h->r_al : nullptr, n, d[0], d[1], d[2], d[3], d[4], d8, h->stream));
    if (!on_device) {
      for (int k = 0; k < 5; ++k) if (o[k]) HCHK(hipMemcpyAsync(o[k] + (size_t)r0 * w[k], d[k], (size_t)n * w[k] * 4, hipMemcpyDeviceToHost, h->stream));
      if (alpha_u8) HCHK(hipMemcpyAsync(alpha_u8 + r0, d8, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    }
    return 0;
  });
  if (rc) return rc;
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

// Layer L of an edit takes part, on the window win = (minx, miny, edge).  get_colors (evaluate.py:60-64): pixel_size = res / (max - min)
// with max = min + edge, everything fp32.  a.res is set.
void edit_window(EditArgs& a, int L, const float win[3]) {
  const float mx = win[0] + win[2];
  a.active[L] = 1; a.minx[L] = win[0]; a.miny[L] = win[1]; a.pixel_size[L] = (float)a.res / (mx - win[0]);
}

// Floats of the staging of one band's host outputs of an edit: edit, edit_fg, edit_bg ([3][band][3]), then the band's edit_u8 bytes.
size_t edit_stage_floats(size_t band) { return band * 9 + (band * 3 + 3) / 4; }

// Texture-edit propagation of a frame on an oh x ow grid, enqueued: k_edit on each band with the windows, textures and usage masks of `a`
// (device pointers).  o = {edit, edit_fg, edit_bg} and edit_u8 are device pointers written in place when `stage` is NULL, else host
// pointers filled one band at a time through `stage` (edit_stage_floats(resx * resy) floats of device memory).
int edit_bands(af_handle* h, const EditArgs& a, int frame, int oh, int ow, float* const o[3], uint8_t* edit_u8, float* stage) {
  const size_t band = (size_t)h->cfg.resx * h->cfg.resy;
  return bands_over(h, frame_time(h, frame), oh, ow, [&](long long r0, int n, int) -> int {
    float* d[3];
    for (int k = 0; k < 3; ++k) d[k] = !o[k] ? nullptr : stage ? stage + (size_t)k * band * 3 : o[k] + (size_t)r0 * 3;
    unsigned char* d8 = !edit_u8 ? nullptr : stage ? (unsigned char*)(stage + 9 * band) : edit_u8 + (size_t)r0 * 3;
    EditArgs b = a;
    b.uv1 = h->r_uv; b.uv2 = h->r_uv2; b.out_alpha = h->r_al;         // read here: bands_over's ensure_render allocates them on a handle's first render
    b.npix = n; b.edit = d[0]; b.edit_layer[0] = d[1]; b.edit_layer[1] = d[2]; b.edit_u8 = d8;
    LCHK(af_launch_edit(&b, h->stream));
    if (stage) {
      for (int k = 0; k < 3; ++k) if (o[k]) HCHK(hipMemcpyAsync(o[k] + (size_t)r0 * 3, d[k], (size_t)n * 12, hipMemcpyDeviceToHost, h->stream));
      if (edit_u8) HCHK(hipMemcpyAsync(edit_u8 + (size_t)r0 * 3, d8, (size_t)n * 3, hipMemcpyDeviceToHost, h->stream));
    }
    return 0;
  });
}

int edit_dead(const char* what) {
  af_set_thread_error((std::string(what) + ": the session's handle has been destroyed").c_str());
  return AF_ESTATE;
}

}  // namespace

// ---- what the training side calls as well (host.h): af_debug_forward sizes the render buffers, af_destroy releases the live sessions ----
int ensure_render(af_handle* h, int rows) {
  if (rows <= h->render_rows_cap) return 0;
  (void)hipFree(h->r_coords); (void)hipFree(h->r_uv); (void)hipFree(h->r_uv2); (void)hipFree(h->r_al); (void)hipFree(h->r_t); (void)hipFree(h->r_rgb); (void)hipFree(h->r_sse);
  h->r_coords = h->r_uv = h->r_uv2 = h->r_al = h->r_t = h->r_rgb = nullptr; h->r_sse = nullptr; h->render_rows_cap = 0;
  const size_t rp = (size_t)tiles_of(rows) * 32;
  HCHK(dalloc(&h->r_coords, rp * 4)); HCHK(dalloc(&h->r_uv, rp * 4)); HCHK(dalloc(&h->r_t, rp * 4 * (h->seg ? 2 : 1)));
  if (h->seg) { HCHK(dalloc(&h->r_uv2, rp * 4)); HCHK(dalloc(&h->r_al, rp * 4)); }
  HCHK(dalloc(&h->r_rgb, rp * 3)); HCHK(dalloc(&h->r_sse, (rp + 255) / 256));
  h->render_rows_cap = rows;
  return 0;
}

void edit_release(af_edit* e) {     // the session's device memory; the host struct stays for af_edit_destroy
  for (int L = 0; L < 2; ++L) { (void)hipFree(e->tex[L]); (void)hipFree(e->use[L]); e->tex[L] = nullptr; e->use[L] = nullptr; }
  e->h = nullptr;
}

extern "C" {

int af_render_frame(af_handle* h, int frame, float* rgb_out, double* sse_out) {
  return render_lattice_frame(h, frame, rgb_out, nullptr, 0, sse_out, "af_render_frame");
}

int af_render_frame_u8(af_handle* h, int frame, float* rgb_out, uint8_t* u8_out, int on_device, double* sse_out) {
  return render_lattice_frame(h, frame, rgb_out, u8_out, on_device, sse_out, "af_render_frame_u8");
}

// The reconstruction of one frame on an oh x ow grid (include/atlasfit.h).  Touches neither the training state nor af_psnr's cache, and
// reads no record.
int af_render_frame_at(af_handle* h, int frame, int oh, int ow, float* rgb_out, uint8_t* u8_out, const uint8_t* ref_u8, double* sse_out, int on_device) {
  if (!h) return AF_EINVAL;
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, "af_render_frame_at: frame index");
  if (oh < 1 || oh > AF_TEX_MAX || ow < 1 || ow > AF_TEX_MAX) return h->fail(AF_EINVAL, "af_render_frame_at: oh and ow must be 1..16384");
  if (!rgb_out && !u8_out && !ref_u8) return h->fail(AF_EINVAL, "af_render_frame_at: rgb_out, u8_out and ref_u8 are all NULL");
  if (sse_out && !ref_u8) return h->fail(AF_EINVAL, "af_render_frame_at: sse_out needs ref_u8");
  if (ref_u8 && !sse_out) return h->fail(AF_EINVAL, "af_render_frame_at: ref_u8 needs sse_out");
  HCHK(hipSetDevice(h->device));
  return render_frame_core(h, frame, oh, ow, rgb_out, u8_out, ref_u8, -1, on_device, sse_out);
}

int af_render_layers(af_handle* h, int frame, float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2) {
  if (!h) return AF_EINVAL;
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, "af_render_layers: frame index");
  if (!h->seg && (uv2 || rgb2)) return h->fail(AF_EINVAL, "af_render_layers: uv2 / rgb2 need a two_layer handle");
  HCHK(hipSetDevice(h->device));
  float* const o[5] = {uv1, uv2, alpha, rgb1, rgb2};
  return layers_core(h, frame, h->cfg.resy, h->cfg.resx, o, nullptr, 0);
}

int af_mapping_area(af_handle* h, int which, float out5[5]) {
  if (!h) return AF_EINVAL;
  if (which != 0 && which != 1) return h->fail(AF_EINVAL, "af_mapping_area: which must be 0 (fg) or 1 (bg)");
  if (!out5) return h->fail(AF_EINVAL, "af_mapping_area: out5 is NULL");
  if (!h->seg) return h->fail(AF_ESTATE, "af_mapping_area: needs a two_layer handle");
  if (!h->have_video) return h->fail(AF_ESTATE, "af_mapping_area: no video uploaded");
  HCHK(hipSetDevice(h->device));
  const int npix = h->cfg.resx * h->cfg.resy, F = h->cfg.number_of_frames, NT = tiles_of(npix), nblk = (npix + 255) / 256;
  int rc = ensure_render(h, npix); if (rc) return rc;
  if ((rc = ensure_layers(h, (size_t)F * nblk * 4)) != 0) return rc;
  const int mnet = which == 0 ? AF_NET_MAP1 : AF_NET_MAP2;
  NetDesc& M = h->nets[mnet];
  float* uv = which == 0 ? h->r_uv : h->r_uv2;
  const float half_f = (float)(F / 2.0);
  for (int f = 0; f < F; ++f) {
    // evaluate.py:160-162: integer index tensors divided in fp32 (t = float(f) / float(F/2) - 1, unlike the render's Python-float t)
    const float t = (float)f / half_f - 1.f;
    if ((rc = fill_rows(h, t, h->cfg.resy, h->cfg.resx, 0, npix)) != 0) return rc;
    FwdArgs fm = fwd_args(h, M, h->r_coords, uv, NT, false);
    FwdArgs fl = fwd_args(h, h->nets[AF_NET_ALPHA], h->r_coords, h->r_al, NT, false);
    if ((rc = launch_fwd(h, T_FWD_1, {{AF_NET_ALPHA, fl, npix}, {mnet, fm, npix}}, false)) != 0) return rc;
    LCHK(af_launch_area_reduce(uv, h->r_al, h->table, (size_t)f * npix, npix, which, h->l_buf + (size_t)f * nblk * 4, h->stream));
  }
  std::vector<float> part((size_t)F * nblk * 4);
  HCHK(hipMemcpyAsync(part.data(), h->l_buf, part.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HCHK(hipStreamSynchronize(h->stream));
  // evaluate.py:153-190: start from min = 1, max = -1 (the values an empty selection returns), then clamp to [-1, 1]; edge may be negative
  float minx = 1.f, miny = 1.f, maxx = -1.f, maxy = -1.f;
  for (size_t b = 0; b < part.size(); b += 4) {
    minx = std::min(minx, part[b]); miny = std::min(miny, part[b + 1]); maxx = std::max(maxx, part[b + 2]); maxy = std::max(maxy, part[b + 3]);
  }
  maxx = std::min(maxx, 1.f); maxy = std::min(maxy, 1.f); minx = std::max(minx, -1.f); miny = std::max(miny, -1.f);
  out5[0] = maxx; out5[1] = minx; out5[2] = maxy; out5[3] = miny; out5[4] = std::max(maxx - minx, maxy - miny);
  return AF_OK;
}

int af_render_atlas_texture(af_handle* h, int res, float minx, float miny, float edge, float* out) {
  if (!h) return AF_EINVAL;
  if (res <= 0 || res > AF_TEX_MAX) return h->fail(AF_EINVAL, "af_render_atlas_texture: res must be 1..16384");
  if (!out) return AF_OK;
  HCHK(hipSetDevice(h->device));
  const int cap = std::max(h->cfg.resx * h->cfg.resy, res);
  int rc = ensure_render(h, cap); if (rc) return rc;
  const int rows_tex = std::max(1, h->render_rows_cap / res);
  const float maxx = minx + edge, maxy = miny + edge;        // evaluate.py:248-257 pass (min, min + edge) in fp32
  for (int row0 = 0; row0 < res; row0 += rows_tex) {
    const int nr = std::min(rows_tex, res - row0), rows = nr * res, NT = tiles_of(rows);
    LCHK(af_launch_tex_coords(h->r_coords, res, row0, nr, minx, maxx, miny, maxy, NT * 32, h->stream));
    FwdArgs fa = fwd_args(h, h->nets[AF_NET_ATLAS], h->r_coords, h->r_t, NT, false);
    fa.in_scale = 1.f; fa.in_shift0 = 0.f; fa.in_shift1 = 0.f;     // the grid is the atlas input itself (no uv*0.5 +- 0.5)
    if ((rc = launch_fwd(h, T_FWD_2, {{AF_NET_ATLAS, fa, rows}}, false)) != 0) return rc;
    LCHK(af_launch_tex_finish(h->r_t, rows, h->r_rgb, h->stream));
    HCHK(hipMemcpyAsync(out + (size_t)row0 * res * 3, h->r_rgb, (size_t)rows * 12, hipMemcpyDeviceToHost, h->stream));
  }
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

int af_render_edit(af_handle* h, int frame, int res, const float* tex_fg, const float win_fg[3], const float* tex_bg, const float win_bg[3],
                   float* edit, float* edit_fg, float* edit_bg, float* use_fg, float* use_bg) {
  if (!h) return AF_EINVAL;
  if (!h->seg) return h->fail(AF_ESTATE, "af_render_edit: needs a two_layer handle");
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, "af_render_edit: frame index");
  if (res <= 0 || res > AF_TEX_MAX) return h->fail(AF_EINVAL, "af_render_edit: res must be 1..16384");
  const float* tex[2] = {tex_fg, tex_bg}; const float* win[2] = {win_fg, win_bg};
  float* eo[2] = {edit_fg, edit_bg}; float* use[2] = {use_fg, use_bg};
  for (int L = 0; L < 2; ++L) {
    if (!win[L] && (tex[L] || eo[L] || use[L])) return h->fail(AF_EINVAL, "af_render_edit: a layer's texture / outputs without its window");
    if (win[L] && !tex[L] && eo[L]) return h->fail(AF_EINVAL, "af_render_edit: edit_fg / edit_bg need that layer's texture");
  }
  if (edit && ((win_fg && !tex_fg) || (win_bg && !tex_bg))) return h->fail(AF_EINVAL, "af_render_edit: edit needs the texture of every layer with a window");
  HCHK(hipSetDevice(h->device));
  const size_t npix = (size_t)h->cfg.resx * h->cfg.resy, R2 = (size_t)res * res;
  int rc = ensure_layers(h, 2 * R2 * 4 + edit_stage_floats(npix)); if (rc) return rc;
  float* d_tex[2] = {h->l_buf, h->l_buf + R2 * 3};
  float* d_use[2] = {h->l_buf + 2 * R2 * 3, h->l_buf + 2 * R2 * 3 + R2};
  EditArgs a{};
  a.res = res;
  for (int L = 0; L < 2; ++L) {
    if (!win[L]) continue;
    edit_window(a, L, win[L]);
    if (tex[L]) { HCHK(hipMemcpyAsync(d_tex[L], tex[L], R2 * 12, hipMemcpyHostToDevice, h->stream)); a.tex[L] = d_tex[L]; }
    if (use[L]) { HCHK(hipMemcpyAsync(d_use[L], use[L], R2 * 4, hipMemcpyHostToDevice, h->stream)); a.use[L] = d_use[L]; }
  }
  float* const o[3] = {edit, edit_fg, edit_bg};
  if ((rc = edit_bands(h, a, frame, h->cfg.resy, h->cfg.resx, o, nullptr, h->l_buf + 2 * R2 * 4)) != 0) return rc;
  for (int L = 0; L < 2; ++L)
    if (use[L]) HCHK(hipMemcpyAsync(use[L], d_use[L], R2 * 4, hipMemcpyDeviceToHost, h->stream));
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

// af_render_layers on an oh x ow grid (include/atlasfit.h).
int af_render_layers_at(af_handle* h, int frame, int oh, int ow, float* uv1, float* uv2, float* alpha, float* rgb1, float* rgb2,
                        uint8_t* alpha_u8, int on_device) {
  if (!h) return AF_EINVAL;
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, "af_render_layers_at: frame index");
  if (oh < 1 || oh > AF_TEX_MAX || ow < 1 || ow > AF_TEX_MAX) return h->fail(AF_EINVAL, "af_render_layers_at: oh and ow must be 1..16384");
  if (!uv1 && !uv2 && !alpha && !rgb1 && !rgb2 && !alpha_u8) return h->fail(AF_EINVAL, "af_render_layers_at: every output pointer is NULL");
  if (!h->seg && (uv2 || rgb2)) return h->fail(AF_EINVAL, "af_render_layers_at: uv2 / rgb2 need a two_layer handle");
  HCHK(hipSetDevice(h->device));
  float* const o[5] = {uv1, uv2, alpha, rgb1, rgb2};
  return layers_core(h, frame, oh, ow, o, alpha_u8, on_device);
}

// ---- edit sessions (include/atlasfit.h): af_render_edit's propagation with the textures and usage masks resident on the device ----
int af_edit_create(af_handle* h, int res, const float* tex_fg, const float win_fg[3], const float* tex_bg, const float win_bg[3], int track_usage, af_edit** out) {
  if (!h) return AF_EINVAL;
  if (!out) return h->fail(AF_EINVAL, "af_edit_create: out is NULL");
  *out = nullptr;
  if (!h->seg) return h->fail(AF_ESTATE, "af_edit_create: needs a two_layer handle");
  if (res <= 0 || res > AF_TEX_MAX) return h->fail(AF_EINVAL, "af_edit_create: res must be 1..16384");
  const float* tex[2] = {tex_fg, tex_bg}; const float* win[2] = {win_fg, win_bg};
  for (int L = 0; L < 2; ++L)
    if (!win[L] && tex[L]) return h->fail(AF_EINVAL, "af_edit_create: a layer's texture without its window");
  if (!win_fg && !win_bg) return h->fail(AF_EINVAL, "af_edit_create: no layer has a window");
  HCHK(hipSetDevice(h->device));
  af_edit* e = new af_edit();
  e->h = h; e->res = res; e->track = track_usage != 0;
  const size_t R2 = (size_t)res * res;
  hipError_t err = hipSuccess;
  for (int L = 0; L < 2 && err == hipSuccess; ++L) {
    if (!win[L]) continue;
    e->have_win[L] = true;
    for (int k = 0; k < 3; ++k) e->win[L][k] = win[L][k];
    if (tex[L]) {
      if ((err = dalloc(&e->tex[L], R2 * 3)) != hipSuccess) break;
      if ((err = hipMemcpyAsync(e->tex[L], tex[L], R2 * 12, hipMemcpyHostToDevice, h->stream)) != hipSuccess) break;
    }
    if (e->track) {
      if ((err = dalloc(&e->use[L], R2)) != hipSuccess) break;
      err = hipMemsetAsync(e->use[L], 0, R2 * 4, h->stream);
    }
  }
  if (err == hipSuccess) err = hipStreamSynchronize(h->stream);      // the caller's textures are free again when this returns
  if (err != hipSuccess) { edit_release(e); delete e; return h->fail(AF_EHIP, "af_edit_create: device memory for the textures / usage masks", err); }
  h->sessions.push_back(e);
  *out = e;
  return AF_OK;
}

int af_edit_frame(af_edit* e, int frame, int oh, int ow, float* edit, float* edit_fg, float* edit_bg, uint8_t* edit_u8, int on_device) {
  if (!e) return AF_EINVAL;
  af_handle* h = e->h;
  if (!h) return edit_dead("af_edit_frame");
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, "af_edit_frame: frame index");
  if (oh < 1 || oh > AF_TEX_MAX || ow < 1 || ow > AF_TEX_MAX) return h->fail(AF_EINVAL, "af_edit_frame: oh and ow must be 1..16384");
  float* eo[2] = {edit_fg, edit_bg};
  for (int L = 0; L < 2; ++L)
    if (eo[L] && !e->tex[L]) return h->fail(AF_EINVAL, "af_edit_frame: edit_fg / edit_bg need that layer's texture");
  if ((edit || edit_u8) && ((e->have_win[0] && !e->tex[0]) || (e->have_win[1] && !e->tex[1])))
    return h->fail(AF_EINVAL, "af_edit_frame: edit / edit_u8 need the texture of every layer with a window");
  if (!edit && !edit_fg && !edit_bg && !edit_u8 && !e->track) return h->fail(AF_EINVAL, "af_edit_frame: no output asked for and no usage tracked");
  HCHK(hipSetDevice(h->device));
  const size_t band = (size_t)h->cfg.resx * h->cfg.resy;
  int rc;
  if (!on_device && (rc = ensure_layers(h, edit_stage_floats(band))) != 0) return rc;
  EditArgs a{};
  a.res = e->res;
  for (int L = 0; L < 2; ++L) {
    if (!e->have_win[L]) continue;
    edit_window(a, L, e->win[L]);
    a.tex[L] = e->tex[L]; a.use[L] = e->use[L];
  }
  float* const o[3] = {edit, edit_fg, edit_bg};
  if ((rc = edit_bands(h, a, frame, oh, ow, o, edit_u8, on_device ? nullptr : h->l_buf)) != 0) return rc;
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

int af_edit_usage(af_edit* e, float* use_fg, float* use_bg) {
  if (!e) return AF_EINVAL;
  af_handle* h = e->h;
  if (!h) return edit_dead("af_edit_usage");
  if (!e->track) return h->fail(AF_ESTATE, "af_edit_usage: the session does not track usage");
  HCHK(hipSetDevice(h->device));
  float* use[2] = {use_fg, use_bg};
  const size_t R2 = (size_t)e->res * e->res;
  for (int L = 0; L < 2; ++L) {
    if (!use[L]) continue;
    if (e->use[L]) HCHK(hipMemcpyAsync(use[L], e->use[L], R2 * 4, hipMemcpyDeviceToHost, h->stream));
    else memset(use[L], 0, R2 * 4);        // a layer without a window uses no texel
  }
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

int af_edit_reset_usage(af_edit* e) {
  if (!e) return AF_EINVAL;
  af_handle* h = e->h;
  if (!h) return edit_dead("af_edit_reset_usage");
  if (!e->track) return h->fail(AF_ESTATE, "af_edit_reset_usage: the session does not track usage");
  HCHK(hipSetDevice(h->device));
  for (int L = 0; L < 2; ++L)
    if (e->use[L]) HCHK(hipMemsetAsync(e->use[L], 0, (size_t)e->res * e->res * 4, h->stream));
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

void af_edit_destroy(af_edit* e) {
  if (!e) return;
  if (af_handle* h = e->h) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->sessions.erase(std::remove(h->sessions.begin(), h->sessions.end(), e), h->sessions.end());
    edit_release(e);
  }
  delete e;
}

// Per-pixel loss maps (evaluate.py:338-384 / :650-705).  Input rows in segments of P = NT*32 rows, ordered [y-d, x-d | centre | flow
// target] so that the mapping nets read one contiguous range [0, nseg_map) (without the target on the last frame) and the alpha net
// another, [centre, centre + 1 or 2).  Segments no requested map needs are not built.  Two chain launches as in chains_over:
// {alpha, mapping1, mapping2}, then the atlas on the centre uv of both mappings (only for rgb_err / residual).
int af_render_loss_maps(af_handle* h, int frame, float* rigidity1, float* rigidity2, float* flow1, float* flow2, float* flow_alpha,
                        float* rgb_err, float* residual) {
  if (!h) return AF_EINVAL;
  if (frame < 0 || frame >= h->cfg.number_of_frames) return h->fail(AF_EINVAL, "af_render_loss_maps: frame index");
  if (!h->have_video) return h->fail(AF_EINVAL, "af_render_loss_maps: no video uploaded");
  if (!h->seg && (rigidity2 || flow2 || flow_alpha)) return h->fail(AF_EINVAL, "af_render_loss_maps: rigidity2 / flow2 / flow_alpha need a two_layer handle");
  HCHK(hipSetDevice(h->device));
  const int F = h->cfg.number_of_frames, npix = h->cfg.resx * h->cfg.resy, NT = tiles_of(npix);
  const size_t P = (size_t)NT * 32;
  const bool rig = rigidity1 || rigidity2, rgb = rgb_err || residual;
  const bool flow_map = (flow1 || flow2) && frame < F - 1;          // the last frame's flow maps are 0 (evaluate.py:374-376, :692)
  const bool need_t = flow_map || flow_alpha != nullptr;
  const bool run_m1 = rigidity1 || flow1 || rgb, run_m2 = h->seg && (rigidity2 || flow2 || rgb);
  const bool run_al = h->seg && (flow_map || flow_alpha || rgb);
  LossMapArgs a{};
  a.seg_ym = rig ? 0 : -1; a.seg_xm = rig ? 1 : -1; a.seg_c = rig ? 2 : 0; a.seg_t = need_t ? a.seg_c + 1 : -1;
  const int nseg = a.seg_c + 1 + (need_t ? 1 : 0), nseg_map = a.seg_c + 1 + (flow_map ? 1 : 0), nseg_al = flow_alpha ? 2 : 1;
  const size_t need = P * 4 * (nseg + (size_t)nseg_map * ((run_m1 ? 1 : 0) + (run_m2 ? 1 : 0)) + (run_al ? nseg_al : 0) + (rgb ? (h->seg ? 2 : 1) : 0))
                      + (size_t)npix * 9;
  int rc = ensure_layers(h, need); if (rc) return rc;
  float* p = h->l_buf;
  auto take = [&p](size_t n) { float* q = p; p += n; return q; };
  a.coords = take(P * 4 * nseg);
  float* out_m1 = run_m1 ? take(P * 4 * nseg_map) : nullptr;
  float* out_m2 = run_m2 ? take(P * 4 * nseg_map) : nullptr;
  float* out_al = run_al ? take(P * 4 * nseg_al) : nullptr;
  float* out_at = rgb ? take(P * 4 * (h->seg ? 2 : 1)) : nullptr;
  float* const host[7] = {rigidity1, rigidity2, flow1, flow2, flow_alpha, rgb_err, residual};
  float* dev[7];
  for (int k = 0; k < 7; ++k) dev[k] = host[k] ? take((size_t)npix * (k == 6 ? 3 : 1)) : nullptr;
  a.table = h->table; a.rec0 = (size_t)frame * npix;
  a.resx = h->cfg.resx; a.resy = h->cfg.resy; a.rows_pad = (int)P; a.frame = frame; a.d = h->cfg.derivative_amount;
  a.half_main = (float)(std::max(h->cfg.resx, h->cfg.resy) / 2.0); a.half_frames = (float)(F / 2.0); a.t_centre = frame_time(h, frame);
  LCHK(af_launch_lossmap_rows(&a, h->stream));
  const int NT_map = NT * nseg_map;
  FwdArgs f1 = fwd_args(h, h->nets[AF_NET_MAP1], a.coords, out_m1, run_m1 ? NT_map : 0, false);
  FwdArgs f2 = h->seg ? fwd_args(h, h->nets[AF_NET_MAP2], a.coords, out_m2, run_m2 ? NT_map : 0, false) : f1;
  FwdArgs fl = h->seg ? fwd_args(h, h->nets[AF_NET_ALPHA], a.coords + (size_t)a.seg_c * P * 4, out_al, run_al ? NT * nseg_al : 0, false) : f1;
  if (!h->seg) rc = launch_fwd(h, T_FWD_1, {{AF_NET_MAP1, f1, (int)P * nseg_map}}, false);
  else         rc = launch_fwd(h, T_FWD_1, {{AF_NET_ALPHA, fl, (int)P * nseg_al}, {AF_NET_MAP1, f1, (int)P * nseg_map}, {AF_NET_MAP2, f2, (int)P * nseg_map}}, false);
  if (rc) return rc;
  if (rgb) {
    FwdArgs fa = fwd_args(h, h->nets[AF_NET_ATLAS], out_m1 + (size_t)a.seg_c * P * 4, out_at, h->seg ? 2 * NT : NT, false);
    if (h->seg) { fa.in1 = out_m2 + (size_t)a.seg_c * P * 4; fa.split_row = (int)P; }
    if ((rc = launch_fwd(h, T_FWD_2, {{AF_NET_ATLAS, fa, (int)P * (h->seg ? 2 : 1)}}, false)) != 0) return rc;
  }
  a.out_m1 = out_m1; a.out_m2 = out_m2; a.out_alpha = out_al; a.out_atlas = out_at; a.flow_map = flow_map ? 1 : 0;
  a.L = (float)std::max(h->cfg.resx, h->cfg.resy); a.uv_scale = h->cfg.uv_mapping_scale;
  a.rigidity1 = dev[0]; a.rigidity2 = dev[1]; a.flow1 = dev[2]; a.flow2 = dev[3]; a.flow_alpha = dev[4]; a.rgb_err = dev[5]; a.residual = dev[6];
  LCHK(af_launch_lossmap_finish(&a, h->stream));
  for (int k = 0; k < 7; ++k) if (host[k]) HCHK(hipMemcpyAsync(host[k], dev[k], (size_t)npix * (k == 6 ? 3 : 1) * 4, hipMemcpyDeviceToHost, h->stream));
  HCHK(hipStreamSynchronize(h->stream));
  return AF_OK;
}

// Warping error of the uploaded video (which 0: one launch over all F-1 pairs, straight from the record table) or of the reconstruction
// (which 1: af_render_frame's rgb, rendered frame by frame through frame_bands into two ping-pong buffers; pair t-1 runs as soon as frame t is rendered).
// Flows: the uploaded ones (REC_FF of frame t, REC_FB of frame t+1).  Forward-only: the frame-error cache of af_psnr is not written.
int af_warp_error(af_handle* h, int which, int align_corners, double* per_pair, double* mean) {
  if (!h) return AF_EINVAL;
  if (which != 0 && which != 1) return h->fail(AF_EINVAL, "af_warp_error: which must be 0 (input) or 1 (reconstruction)");
  if (align_corners != 0 && align_corners != 1) return h->fail(AF_EINVAL, "af_warp_error: align_corners must be 0 or 1");
  const int F = h->cfg.number_of_frames;
  if (F < 2) return h->fail(AF_EINVAL, "af_warp_error: needs at least two frames");
  if (!h->have_video) return h->fail(AF_ESTATE, "af_warp_error: no video uploaded");
  HCHK(hipSetDevice(h->device));
  const int npix = h->cfg.resx * h->cfg.resy, nblk = (npix + 255) / 256;
  const size_t rec = (size_t)npix * AF_REC_F, npart = (size_t)(F - 1) * nblk * 2;
  const size_t img = ((size_t)npix * 3 + 63) / 64 * 64;                 // ping-pong frames (which 1), 256-byte aligned
  int rc = ensure_layers(h, npart * 2 + (which ? 2 * img : 0)); if (rc) return rc;
  double* part = (double*)h->l_buf;
  float* buf[2] = {h->l_buf + npart * 2, h->l_buf + npart * 2 + img};
  WarpErrArgs a{};
  a.h = h->cfg.resy; a.w = h->cfg.resx; a.align_corners = align_corners;
  if (which == 0) {
    a.img1 = h->table + REC_RGB; a.img2 = h->table + rec + REC_RGB; a.flow12 = h->table + REC_FF; a.flow21 = h->table + rec + REC_FB;
    a.img_pair_stride = a.flow_pair_stride = rec; a.part = part;
    LCHK(af_launch_warp_error(&a, 0, F - 1, h->stream));
  } else {
    for (int f = 0; f < F; ++f) {
      if ((rc = frame_bands(h, frame_time(h, f), h->cfg.resy, h->cfg.resx, buf[f & 1], nullptr, nullptr, -1, 1, nullptr)) != 0) return rc;
      if (f == 0) continue;
      a.img1 = buf[(f - 1) & 1]; a.img2 = buf[f & 1];
      a.flow12 = h->table + (size_t)(f - 1) * rec + REC_FF; a.flow21 = h->table + (size_t)f * rec + REC_FB;
      a.part = part + (size_t)(f - 1) * nblk * 2;
      LCHK(af_launch_warp_error(&a, 1, 1, h->stream));
    }
  }
  std::vector<double> hp(npart);
  HCHK(hipMemcpyAsync(hp.data(), part, npart * 8, hipMemcpyDeviceToHost, h->stream));
  HCHK(hipStreamSynchronize(h->stream));
  double acc = 0.0;
  for (int t = 0; t < F - 1; ++t) {
    const double e = warp_error_of(hp.data() + (size_t)t * nblk * 2, nblk, npix);
    if (per_pair) per_pair[t] = e;
    acc += e;
  }
  if (mean) *mean = acc / (F - 1);
  return AF_OK;
}

int af_psnr(af_handle* h, double* mean_psnr, double* per_frame) {
  if (!h) return AF_EINVAL;
  const int F = h->cfg.number_of_frames; const double cnt = (double)h->cfg.resx * h->cfg.resy * 3.0;
  double acc = 0;
  for (int f = 0; f < F; ++f) {
    if (!h->frame_sse_valid[f]) { int rc = af_render_frame(h, f, nullptr, nullptr); if (rc) return rc; }
    const double mse = h->frame_sse[f] / cnt;
    const double p = 10.0 * log10(1.0 / mse);
    if (per_frame) per_frame[f] = p;
    acc += p;
  }
  if (mean_psnr) *mean_psnr = acc / F;
  return AF_OK;
}

}  // extern "C"
