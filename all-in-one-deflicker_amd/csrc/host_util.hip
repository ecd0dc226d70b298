// host_util.hip — the handle-free utilities of libatlasfit.so (include/atlasfit.h): the input builders (resizes, flow consistency, luminance
// grids), the YUV4MPEG2 conversions, the mask propagation steps, the guided transfer, the fidelity metrics and the warping error of one pair.  Stateless; each call runs one kernel on
// the default stream of the device it names and reports through af_last_error(NULL).
#include <float.h>
#include <string.h>
#include <cmath>
#include <type_traits>

#include "fidelity.h"
#include "host.h"

namespace {

int refuse(const std::string& m) { af_set_thread_error(m.c_str()); return AF_EINVAL; }

// The device side of one call.  Constructing it selects the device.  in / out hand out the device pointer of a buffer of the caller's: the
// caller's own pointer when the call is on_device, else a device copy that lives as long as the call (inputs uploaded at once, outputs
// copied back by finish).  upload / fetch do the same for a buffer that is on the host whatever on_device says (tables, partial sums),
// scratch is device memory nobody reads back.  finish takes the launch's result, synchronises the default stream and copies the host
// outputs back.  The first HIP error is kept and nothing touches the device after it: status() is then AF_EHIP with "<what>: <HIP's
// text>" as the thread's message, so a caller checks once after staging (a launch must not see the null pointers of a failed staging).
struct UtilCall {
  struct Back { void* host; void* dev; size_t bytes; };
  const bool on_device; hipError_t e; const char* what = "hipSetDevice";
  std::vector<void*> owned; std::vector<Back> back;
  UtilCall(int device_ordinal, int on_device_) : on_device(on_device_ != 0), e(hipSetDevice(device_ordinal)) {}
  UtilCall(const UtilCall&) = delete;
  ~UtilCall() { for (void* p : owned) (void)hipFree(p); }
  bool ok() const { return e == hipSuccess; }
  int status() const {
    if (ok()) return AF_OK;
    af_set_thread_error((std::string(what) + ": " + hipGetErrorString(e)).c_str());
    return AF_EHIP;
  }
  void step(const char* w, hipError_t r) { if (ok() && r != hipSuccess) { e = r; what = w; } }
  void* scratch(size_t bytes, const char* w = "scratch buffer") {
    void* d = nullptr;
    if (ok()) step(w, hipMalloc(&d, std::max<size_t>(bytes, 1)));
    if (d) owned.push_back(d);
    return d;
  }
  template <class T> const T* upload(const T* p, size_t bytes) {
    void* d = scratch(bytes, "stage input");
    if (ok()) step("stage input", hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
    return (const T*)d;
  }
  template <class T> T* fetch(T* p, size_t bytes) {
    void* d = scratch(bytes, "stage output");
    if (ok()) back.push_back({p, d, bytes});
    return (T*)d;
  }
  template <class T> const T* in(const T* p, size_t bytes) { return on_device ? p : upload(p, bytes); }
  template <class T> T* out(T* p, size_t bytes) { return on_device ? p : fetch(p, bytes); }
  int finish(const char* kernel, int launch_result) {
    step(kernel, (hipError_t)launch_result);
    if (ok()) step(kernel, hipStreamSynchronize(nullptr));
    for (const Back& b : back) if (ok()) step("copy back", hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    return status();
  }
};

// The coverage table of one axis for INTER_AREA (computeResizeAreaTab): in fp64, the weights stored as float; the entries of
// destination d are ofs[d] .. ofs[d + 1] - 1, in the order OpenCV emits them.
void area_table(int ssize, int dsize, double scale, std::vector<int>& ofs, std::vector<int>& idx, std::vector<float>& w) {
  for (int d = 0; d < dsize; ++d) {
    const double f1 = d * scale, f2 = f1 + scale, cell = std::min(scale, ssize - f1);
    int s1 = (int)std::ceil(f1);
    const int s2 = std::min((int)std::floor(f2), ssize - 1);
    s1 = std::min(s1, s2);
    ofs.push_back((int)idx.size());
    if (s1 - f1 > 1e-3) { idx.push_back(s1 - 1); w.push_back((float)((s1 - f1) / cell)); }
    for (int s = s1; s < s2; ++s) { idx.push_back(s); w.push_back((float)(1.0 / cell)); }
    if (f2 - s2 > 1e-3) { idx.push_back(s2); w.push_back((float)(std::min(std::min(f2 - s2, 1.0), cell) / cell)); }
  }
  ofs.push_back((int)idx.size());
}

// YCbCr <-> RGB of a YUV4MPEG2 frame payload (yuv_core.h through yuv.hip and yuv16.hip), one body over the sample
// type.  The coefficient tables are built here in fp64 at D = bits bits per sample and rounded to Q = D + 6 fraction bits, with the scales
// of a D-bit code range, sy = 219 2^(D-8) / M and sc = 224 2^(D-8) / M; the rows of the RGB -> YCbCr matrix are then adjusted at their
// largest entry so that the luma row sums exactly to its scale and each chroma row exactly to 0: a grey pixel has chroma exactly C and, in
// full range, Y = v.  The 8-bit entries pass bits = 8 (Q = 14, the table yuv.hip's constants expect) and check neither bits nor parity.
bool yuv_plane_sizes(int h, int w, int layout, int* ch, int* cw, int* hmode, int* vmode) {
  switch (layout) {
    case AF_YUV_444: *hmode = YUV_AXIS_FULL; *vmode = YUV_AXIS_FULL; break;
    case AF_YUV_422: *hmode = YUV_AXIS_COSITED; *vmode = YUV_AXIS_FULL; break;
    case AF_YUV_420JPEG: *hmode = YUV_AXIS_CENTRED; *vmode = YUV_AXIS_CENTRED; break;
    case AF_YUV_420MPEG2: *hmode = YUV_AXIS_COSITED; *vmode = YUV_AXIS_CENTRED; break;
    case AF_YUV_MONO: *hmode = YUV_AXIS_FULL; *vmode = YUV_AXIS_FULL; *ch = 0; *cw = 0; return true;
    default: return false;
  }
  *cw = *hmode == YUV_AXIS_FULL ? w : (w + 1) / 2;
  *ch = *vmode == YUV_AXIS_FULL ? h : (h + 1) / 2;
  return true;
}
void yuv_fix_row(int (&row)[3], int target) {      // the largest entry takes what rounding left over
  int big = 0;
  for (int k = 1; k < 3; ++k) if (std::abs(row[k]) > std::abs(row[big])) big = k;
  row[big] += target - (row[0] + row[1] + row[2]);
}
const char* bits_error(int bits) { return bits < 8 || bits > 16 ? "bits must be 8..16" : nullptr; }
bool odd_pointer(const void* p) { return (uintptr_t)p % 2 != 0; }
template <class S>
int yuv_convert(const char* name, bool to_rgb, int device_ordinal, const S* src, int h, int w, int layout, int matrix, int full_range, int bits,
                S* dst, int on_device) {
  constexpr bool deep = sizeof(S) == 2;
  const std::string who(name);
  if (!src || !dst) return refuse(who + ": null pointer");
  if (h < 1 || h > 16384) return refuse(who + ": h must be 1..16384");
  if (w < 1 || w > 16384) return refuse(who + ": w must be 1..16384");
  typename std::conditional<deep, Yuv16Args, YuvArgs>::type a{};
  if (!yuv_plane_sizes(h, w, layout, &a.ch, &a.cw, &a.hmode, &a.vmode)) return refuse(who + ": unknown layout");
  if (matrix != AF_YUV_BT601 && matrix != AF_YUV_BT709) return refuse(who + ": unknown matrix");
  if constexpr (deep) {
    if (const char* m = bits_error(bits)) return refuse(who + ": " + m);
    if (odd_pointer(src) || odd_pointer(dst)) return refuse(who + ": uint16 pointers must be 2-byte aligned");
  }
  UtilCall c(device_ordinal, on_device);
  const int Q = bits + 6;
  const auto q = [Q](double v) { return (int)std::nearbyint(v * std::ldexp(1.0, Q)); };
  const double M = (double)((1 << bits) - 1), up = std::ldexp(1.0, bits - 8);
  const double kr = matrix == AF_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == AF_YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
  const double sy = full_range ? 1.0 : 219.0 * up / M, sc = full_range ? 1.0 : 224.0 * up / M;      // RGB -> YCbCr scales; the way back divides
  a.h = h; a.w = w; a.mono = layout == AF_YUV_MONO; a.y0 = full_range ? 0 : 16 << (bits - 8);
  if constexpr (deep) { a.q = Q; a.maxv = (1 << bits) - 1; a.c16 = 1 << (bits + 3); }
  a.cy = q(1.0 / sy);
  a.crv = q(2.0 * (1.0 - kr) / sc);
  a.cgu = q(-2.0 * (1.0 - kb) * kb / kg / sc);
  a.cgv = q(-2.0 * (1.0 - kr) * kr / kg / sc);
  a.cbu = q(2.0 * (1.0 - kb) / sc);
  a.ky[0] = q(kr * sy); a.ky[1] = q(kg * sy); a.ky[2] = q(kb * sy);
  a.ku[0] = q(-kr / (2.0 * (1.0 - kb)) * sc); a.ku[1] = q(-kg / (2.0 * (1.0 - kb)) * sc); a.ku[2] = q(0.5 * sc);
  a.kv[0] = q(0.5 * sc); a.kv[1] = q(-kg / (2.0 * (1.0 - kr)) * sc); a.kv[2] = q(-kb / (2.0 * (1.0 - kr)) * sc);
  yuv_fix_row(a.ky, q(sy)); yuv_fix_row(a.ku, 0); yuv_fix_row(a.kv, 0);
  const size_t ybytes = sizeof(S) * ((size_t)h * w + 2 * (size_t)a.ch * a.cw), rbytes = sizeof(S) * (size_t)h * w * 3;
  a.src = c.in(src, to_rgb ? ybytes : rbytes); a.dst = c.out(dst, to_rgb ? rbytes : ybytes);
  if (!c.ok()) return c.status();
  if constexpr (deep) return to_rgb ? c.finish("k_yuv_to_rgb16", af_launch_yuv_to_rgb16(&a, nullptr)) : c.finish("k_rgb_to_yuv16", af_launch_rgb_to_yuv16(&a, nullptr));
  else return to_rgb ? c.finish("k_yuv_to_rgb", af_launch_yuv_to_rgb(&a, nullptr)) : c.finish("k_rgb_to_yuv", af_launch_rgb_to_yuv(&a, nullptr));
}

// Mask propagation along the flows (maskprop.hip): one step s -> t, and the blend of a forward and a backward result.
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
const char* mask_size_error(int h, int w) {
  if (h < 1 || h > 16384) return "h must be 1..16384";
  if (w < 1 || w > 16384) return "w must be 1..16384";
  return nullptr;
}

// The full-size apply of the guided transfer (guided.hip), one body over the sample type; `name` carries the entry's
// "af_...: " prefix.  The refusals come before the device is touched; the 8-bit entry passes bits = 8 and checks neither bits nor parity.
// `colour`: a is the nine-channel plane A of the colour guide and the launch the colour kernel's.
template <class S>
int guided_apply(const char* name, int device_ordinal, const S* full, int H, int W, int bits, const float* a, const float* b, int h, int w, S* out,
                 int on_device, bool colour = false) {
  constexpr bool deep = sizeof(S) == 2;
  const std::string who(name);
  if (!full || !a || !b || !out) return refuse(who + "null pointer");
  if (H < 1 || H > 16384) return refuse(who + "H must be 1..16384");
  if (W < 1 || W > 16384) return refuse(who + "W must be 1..16384");
  if (const char* m = mask_size_error(h, w)) return refuse(who + m);
  if (h > H || w > W) return refuse(who + "the proxy is larger than the full frame");
  if constexpr (deep) {
    if (const char* m = bits_error(bits)) return refuse(who + m);
    if (odd_pointer(full) || odd_pointer(out)) return refuse(who + "uint16 pointers must be 2-byte aligned");
  }
  const size_t fb = sizeof(S) * (size_t)H * W * 3, pb = (size_t)h * w * 12, ab = colour ? 3 * pb : pb;
  if (ranges_overlap(out, fb, full, fb) || ranges_overlap(out, fb, a, ab) || ranges_overlap(out, fb, b, pb)) return refuse(who + "the output aliases an input");
  UtilCall c(device_ordinal, on_device);
  const S* df = c.in(full, fb);
  const float *da = c.in(a, ab), *db = c.in(b, pb);
  S* o = c.out(out, fb);
  if (!c.ok()) return c.status();
  const double sx = (double)w / (double)W, sy = (double)h / (double)H;
  if constexpr (deep) {
    const int maxv = (1 << bits) - 1;
    const GuidedApply16Args g{df, H, W, da, db, h, w, sx, sy, maxv, (float)((double)maxv / 255.0), o};
    if (colour) return c.finish("k_guided_apply_colour16", af_launch_guided_apply_colour16(&g, nullptr));
    return c.finish("k_guided_apply16", af_launch_guided_apply16(&g, nullptr));
  } else {
    const GuidedApplyArgs g{df, H, W, da, db, h, w, sx, sy, o};
    if (colour) return c.finish("k_guided_apply_colour", af_launch_guided_apply_colour(&g, nullptr));
    return c.finish("k_guided_apply", af_launch_guided_apply(&g, nullptr));
  }
}

}  // namespace

// E_t of one pair from the fp64 block partials [nblk][2], summed in block order; N = 3 * sum noc, or 3 * h * w when no pixel is
// unoccluded (the error is then 0).
double warp_error_of(const double* part, int nblk, int npix) {
  double sse = 0.0, cnt = 0.0;
  for (int b = 0; b < nblk; ++b) { sse += part[2 * b]; cnt += part[2 * b + 1]; }
  return sse / (3.0 * (cnt > 0.0 ? cnt : (double)npix));
}

extern "C" {

int af_resize_bilinear(int device_ordinal, const void* src, int src_u8, int sh, int sw, int ch, float* dst, int dh, int dw,
                       int64_t pix_stride, int64_t ch_stride, int64_t offset, double scale0, double scale1, int on_device) {
  if (!src || !dst || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || ch <= 0 || pix_stride <= 0) return refuse("af_resize_bilinear: arguments");
  UtilCall c(device_ordinal, on_device);
  if (!c.ok()) return c.status();
  if (!on_device && (pix_stride != ch || ch_stride != 1 || offset != 0)) return refuse("af_resize_bilinear: host destinations must be HWC contiguous");
  const void* s = c.in(src, (size_t)sh * sw * ch * (src_u8 ? 1 : 4));
  float* d = c.out(dst, (size_t)dh * dw * ch * 4);
  if (!c.ok()) return c.status();
  ResizeArgs a{s, src_u8, sh, sw, ch, d, dh, dw, pix_stride, ch_stride, offset, scale0, scale1};
  return c.finish("k_resize_bilinear", af_launch_resize(&a, nullptr));
}

int af_resize_area(int device_ordinal, const uint8_t* src, int sh, int sw, int ch, uint8_t* dst, int dh, int dw, int on_device) {
  if (!src || !dst) return refuse("af_resize_area: null pointer");
  if (ch < 1 || ch > 4) return refuse("af_resize_area: ch must be 1..4");
  if (dh < 1) return refuse("af_resize_area: dh < 1");
  if (dw < 1) return refuse("af_resize_area: dw < 1");
  if (dh > sh) return refuse("af_resize_area: dh > sh (INTER_AREA is implemented for shrinking only)");
  if (dw > sw) return refuse("af_resize_area: dw > sw (INTER_AREA is implemented for shrinking only)");
  if (dh == sh && dw == sw) return refuse("af_resize_area: dh == sh && dw == sw (nothing to resize)");
  if ((int64_t)dh * dw > ((int64_t)1 << 38)) return refuse("af_resize_area: image too large");
  UtilCall c(device_ordinal, on_device);
  if (!c.ok()) return c.status();
  AreaArgs a{};
  a.sh = sh; a.sw = sw; a.ch = ch; a.dh = dh; a.dw = dw;
  const double scale_x = 1.0 / ((double)dw / sw), scale_y = 1.0 / ((double)dh / sh);
  const int isx = (int)std::nearbyint(scale_x), isy = (int)std::nearbyint(scale_y);
  const bool fast = std::fabs(scale_x - isx) < DBL_EPSILON && std::fabs(scale_y - isy) < DBL_EPSILON &&
                    (int64_t)isx * dw == sw && (int64_t)isy * dh == sh;      // the products: the block reads stay inside the source
  if (fast) {
    a.mode = (isx == 2 && isy == 2 && ch != 2) ? AREA_2X2 : AREA_BLOCK;
    a.isx = isx; a.isy = isy; a.inv_area = (float)(1.f / (float)((int64_t)isx * isy));
  } else {
    std::vector<int> xofs, yofs, xidx, yidx; std::vector<float> xa, ya;
    area_table(sw, dw, scale_x, xofs, xidx, xa);
    area_table(sh, dh, scale_y, yofs, yidx, ya);
    for (int v : xidx) if (v < 0 || v >= sw) return refuse("af_resize_area: x table out of range");
    for (int v : yidx) if (v < 0 || v >= sh) return refuse("af_resize_area: y table out of range");
    const size_t o_yofs = xofs.size(), o_xidx = o_yofs + yofs.size(), o_yidx = o_xidx + xidx.size(), o_xa = o_yidx + yidx.size(), o_ya = o_xa + xa.size();
    std::vector<int> tab(o_ya + ya.size());       // xofs | yofs | xidx | yidx | xa | ya (floats as bits), one upload
    std::copy(xofs.begin(), xofs.end(), tab.begin()); std::copy(yofs.begin(), yofs.end(), tab.begin() + o_yofs);
    std::copy(xidx.begin(), xidx.end(), tab.begin() + o_xidx); std::copy(yidx.begin(), yidx.end(), tab.begin() + o_yidx);
    if (!xa.empty()) memcpy(tab.data() + o_xa, xa.data(), xa.size() * 4);
    if (!ya.empty()) memcpy(tab.data() + o_ya, ya.data(), ya.size() * 4);
    const int* base = c.upload(tab.data(), tab.size() * 4);
    a.mode = AREA_GENERAL;
    a.xofs = base; a.yofs = base + o_yofs; a.xidx = base + o_xidx; a.yidx = base + o_yidx;
    a.xa = (const float*)(base + o_xa); a.ya = (const float*)(base + o_ya);
  }
  a.src = c.in(src, (size_t)sh * sw * ch); a.dst = c.out(dst, (size_t)dh * dw * ch);
  if (!c.ok()) return c.status();
  return c.finish("k_resize_area", af_launch_resize_area(&a, nullptr));
}

// Luminance grids for the cut detector (shots.hip): the kernel leaves one 64-bit sum per strip of a cell, the strips are added here.
int af_luma_grid(int device_ordinal, const uint8_t* src, int n, int h, int w, int gh, int gw, uint64_t* sums_out, int on_device) {
  if (!src || !sums_out) return refuse("af_luma_grid: null pointer");
  if (n < 1) return refuse("af_luma_grid: n < 1");
  if (h < 1) return refuse("af_luma_grid: h < 1");
  if (w < 1) return refuse("af_luma_grid: w < 1");
  if (gh < 1 || gh > 64) return refuse("af_luma_grid: gh must be 1..64");
  if (gw < 1 || gw > 64) return refuse("af_luma_grid: gw must be 1..64");
  if (h > (1 << 24) || w > (1 << 24)) return refuse("af_luma_grid: image too large");
  UtilCall c(device_ordinal, on_device);
  LumaArgs a{};
  a.n = n; a.h = h; a.w = w; a.gh = std::min(gh, h); a.gw = std::min(gw, w);
  const int cw = (w + a.gw - 1) / a.gw, chh = (h + a.gh - 1) / a.gh;      // the largest cell
  a.strip_rows = std::max(4, (4096 + cw - 1) / cw);                       // ~4096 pixels per workgroup, a row for each of its four waves
  a.strips = (chh + a.strip_rows - 1) / a.strip_rows;
  const size_t cells = (size_t)a.gh * a.gw, nparts = (size_t)n * cells * a.strips;
  std::vector<unsigned long long> part(nparts);
  a.src = c.in(src, (size_t)n * h * w * 3); a.part = c.fetch(part.data(), nparts * 8);
  if (!c.ok()) return c.status();
  if (int rc = c.finish("k_luma_grid", af_launch_luma_grid(&a, nullptr))) return rc;
  for (size_t i = 0; i < (size_t)n * cells; ++i) {
    uint64_t t = 0;
    for (int k = 0; k < a.strips; ++k) t += part[i * a.strips + k];
    sums_out[i] = t;
  }
  return AF_OK;
}

int64_t af_yuv_frame_bytes(int h, int w, int layout) {
  int ch, cw, hm, vm;
  if (h < 1 || h > 16384 || w < 1 || w > 16384 || !yuv_plane_sizes(h, w, layout, &ch, &cw, &hm, &vm)) return 0;
  return (int64_t)h * w + 2 * (int64_t)ch * cw;
}

int af_yuv_to_rgb(int device_ordinal, const uint8_t* yuv, int h, int w, int layout, int matrix, int full_range, uint8_t* rgb, int on_device) {
  return yuv_convert("af_yuv_to_rgb", true, device_ordinal, yuv, h, w, layout, matrix, full_range, 8, rgb, on_device);
}

int af_rgb_to_yuv(int device_ordinal, const uint8_t* rgb, int h, int w, int layout, int matrix, int full_range, uint8_t* yuv, int on_device) {
  return yuv_convert("af_rgb_to_yuv", false, device_ordinal, rgb, h, w, layout, matrix, full_range, 8, yuv, on_device);
}

int af_mask_step(int device_ordinal, const float* m_s, const float* c_s, const float* f_ts, const float* f_st, int h, int w, float thresh,
                 float* m_t, float* c_t, int on_device) {
  const std::string who("af_mask_step: ");
  if (!m_s || !c_s || !f_ts || !f_st || !m_t || !c_t) return refuse(who + "null pointer");
  if (const char* m = mask_size_error(h, w)) return refuse(who + m);
  if (!std::isfinite(thresh) || thresh <= 0.f) return refuse(who + "thresh must be finite and > 0");
  const size_t pb = (size_t)h * w * 4, fb = 2 * pb;
  const void* ins[4] = {m_s, c_s, f_ts, f_st}; const size_t inb[4] = {pb, pb, fb, fb};
  for (int k = 0; k < 4; ++k)
    if (ranges_overlap(m_t, pb, ins[k], inb[k]) || ranges_overlap(c_t, pb, ins[k], inb[k])) return refuse(who + "an output aliases an input");
  if (ranges_overlap(m_t, pb, c_t, pb)) return refuse(who + "m_t aliases c_t");
  UtilCall c(device_ordinal, on_device);
  const float *dm = c.in(m_s, pb), *dc = c.in(c_s, pb), *dts = c.in(f_ts, fb), *dst = c.in(f_st, fb);
  float *om = c.out(m_t, pb), *oc = c.out(c_t, pb);
  if (!c.ok()) return c.status();
  MaskStepArgs a{dm, dc, dts, dst, h, w, (float)(thresh * thresh), om, oc};
  return c.finish("k_mask_step", af_launch_mask_step(&a, nullptr));
}

int af_mask_blend(int device_ordinal, const float* m_f, const float* c_f, const float* m_b, const float* c_b, int h, int w, int a, int t, int b,
                  float* out, int on_device) {
  const std::string who("af_mask_blend: ");
  if (!m_f || !c_f || !m_b || !c_b || !out) return refuse(who + "null pointer");
  if (const char* m = mask_size_error(h, w)) return refuse(who + m);
  if (!(a < t && t < b)) return refuse(who + "frames must satisfy a < t < b");
  const size_t pb = (size_t)h * w * 4;
  const float* ins[4] = {m_f, c_f, m_b, c_b};
  for (int k = 0; k < 4; ++k)
    if (ranges_overlap(out, pb, ins[k], pb)) return refuse(who + "the output aliases an input");
  UtilCall c(device_ordinal, on_device);
  const float* s[4];
  for (int k = 0; k < 4; ++k) s[k] = c.in(ins[k], pb);
  float* o = c.out(out, pb);
  if (!c.ok()) return c.status();
  MaskBlendArgs g{s[0], s[1], s[2], s[3], h, w, (float)((int64_t)b - t), (float)((int64_t)t - a), (float)((int64_t)b - a), o};
  return c.finish("k_mask_blend", af_launch_mask_blend(&g, nullptr));
}

// Residual guided transfer (guided.hip).  The refusals come before the device is touched.
int af_guided_coeffs(int device_ordinal, const uint8_t* proxy_in, const uint8_t* proxy_out, int h, int w, int r, float eps,
                     float* a_out, float* b_out, float* work, int on_device) {
  const std::string who("af_guided_coeffs: ");
  if (!proxy_in || !proxy_out || !a_out || !b_out) return refuse(who + "null pointer");
  if (r < 1 || r > 32) return refuse(who + "r must be 1..32");
  if (!std::isfinite(eps) || eps <= 0.f) return refuse(who + "eps must be finite and > 0");
  if (const char* m = mask_size_error(h, w)) return refuse(who + m);
  if (work && !on_device) return refuse(who + "work is device memory: host pointers take none");
  const size_t ib = (size_t)h * w * 3, pb = ib * 4;
  if (ranges_overlap(a_out, pb, b_out, pb)) return refuse(who + "a_out aliases b_out");
  if (work && (ranges_overlap(work, 2 * pb, a_out, pb) || ranges_overlap(work, 2 * pb, b_out, pb))) return refuse(who + "work aliases an output");
  UtilCall c(device_ordinal, on_device);
  const uint8_t *di = c.in(proxy_in, ib), *dp = c.in(proxy_out, ib);
  float *oa = c.out(a_out, pb), *ob = c.out(b_out, pb);
  float* raw = work ? work : (float*)c.scratch(2 * pb);      // the unsmoothed planes: a, then b
  if (!c.ok()) return c.status();
  GuidedCoeffArgs g{di, dp, h, w, r, eps, raw, raw + ib};
  c.step("k_guided_coeffs", (hipError_t)af_launch_guided_coeffs(&g, nullptr));
  if (!c.ok()) return c.status();
  GuidedSmoothArgs m{raw, raw + ib, h, w, r, oa, ob};
  return c.finish("k_guided_smooth", af_launch_guided_smooth(&m, nullptr));
}

int af_guided_apply(int device_ordinal, const uint8_t* full, int H, int W, const float* a, const float* b, int h, int w, uint8_t* out,
                    int on_device) {
  return guided_apply("af_guided_apply: ", device_ordinal, full, H, W, 8, a, b, h, w, out, on_device);
}

// The colour guide (guided.hip): three launches, the window sums, the fp64 solve and the box means of the 12 planes.  work is
// 33 * h * w four-byte words: the 21 int32 planes of sums, then the unsmoothed A (h, w, 9) and b (h, w, 3).
int af_guided_coeffs_colour(int device_ordinal, const uint8_t* proxy_in, const uint8_t* proxy_out, int h, int w, int r, float eps,
                            float* A_out, float* b_out, float* work, int on_device) {
  const std::string who("af_guided_coeffs_colour: ");
  if (!proxy_in || !proxy_out || !A_out || !b_out) return refuse(who + "null pointer");
  if (r < 1 || r > 32) return refuse(who + "r must be 1..32");
  if (!std::isfinite(eps) || eps < 0x1p-20f) return refuse(who + "eps must be finite and >= 2^-20");
  if (const char* m = mask_size_error(h, w)) return refuse(who + m);
  if (work && !on_device) return refuse(who + "work is device memory: host pointers take none");
  const size_t px = (size_t)h * w, ib = px * 3, Ab = px * 36, bb = px * 12, wb = px * 132;
  if (ranges_overlap(A_out, Ab, b_out, bb)) return refuse(who + "a_out aliases b_out");
  if (work && (ranges_overlap(work, wb, A_out, Ab) || ranges_overlap(work, wb, b_out, bb))) return refuse(who + "work aliases an output");
  UtilCall c(device_ordinal, on_device);
  const uint8_t *di = c.in(proxy_in, ib), *dp = c.in(proxy_out, ib);
  float *oa = c.out(A_out, Ab), *ob = c.out(b_out, bb);
  float* raw = work ? work : (float*)c.scratch(wb);
  if (!c.ok()) return c.status();
  int* sums = (int*)raw;
  float *rawA = raw + 21 * px, *rawb = rawA + 9 * px;
  GuidedMomentArgs g{di, dp, h, w, r, sums};
  c.step("k_guided_moments", (hipError_t)af_launch_guided_moments(&g, nullptr));
  if (!c.ok()) return c.status();
  GuidedSolveArgs v{sums, h, w, r, eps, rawA, rawb};
  c.step("k_guided_solve", (hipError_t)af_launch_guided_solve(&v, nullptr));
  if (!c.ok()) return c.status();
  GuidedSmoothArgs m{rawA, rawb, h, w, r, oa, ob};
  return c.finish("k_guided_smooth", af_launch_guided_smooth_colour(&m, nullptr));
}

int af_guided_apply_colour(int device_ordinal, const uint8_t* full, int H, int W, const float* A, const float* b, int h, int w, uint8_t* out,
                           int on_device) {
  return guided_apply("af_guided_apply_colour: ", device_ordinal, full, H, W, 8, A, b, h, w, out, on_device, true);
}

int af_guided_apply_colour16(int device_ordinal, const uint16_t* full, int H, int W, int bits, const float* A, const float* b, int h, int w,
                             uint16_t* out, int on_device) {
  return guided_apply("af_guided_apply_colour16: ", device_ordinal, full, H, W, bits, A, b, h, w, out, on_device, true);
}

// Frames of more than 8 bits per sample: the bodies above at uint16 samples, and the depth reduction (yuv16.hip).
int af_yuv_to_rgb16(int device_ordinal, const uint16_t* yuv, int h, int w, int layout, int matrix, int full_range, int bits, uint16_t* rgb,
                    int on_device) {
  return yuv_convert("af_yuv_to_rgb16", true, device_ordinal, yuv, h, w, layout, matrix, full_range, bits, rgb, on_device);
}

int af_rgb_to_yuv16(int device_ordinal, const uint16_t* rgb, int h, int w, int layout, int matrix, int full_range, int bits, uint16_t* yuv,
                    int on_device) {
  return yuv_convert("af_rgb_to_yuv16", false, device_ordinal, rgb, h, w, layout, matrix, full_range, bits, yuv, on_device);
}

int af_depth_reduce(int device_ordinal, const uint16_t* src, int64_t count, int bits, uint8_t* dst, int on_device) {
  const std::string who("af_depth_reduce: ");
  if (!src || !dst) return refuse(who + "null pointer");
  if (count < 1 || count > ((int64_t)1 << 32)) return refuse(who + "count must be 1..2^32");
  if (const char* m = bits_error(bits)) return refuse(who + m);
  if (odd_pointer(src)) return refuse(who + "uint16 pointers must be 2-byte aligned");
  if (ranges_overlap(dst, (size_t)count, src, 2 * (size_t)count)) return refuse(who + "the output aliases the input");
  UtilCall c(device_ordinal, on_device);
  DepthReduceArgs a{};
  a.count = count; a.maxv = (1 << bits) - 1;
  a.src = c.in(src, 2 * (size_t)count); a.dst = c.out(dst, (size_t)count);
  if (!c.ok()) return c.status();
  return c.finish("k_depth_reduce", af_launch_depth_reduce(&a, nullptr));
}

int af_guided_apply16(int device_ordinal, const uint16_t* full, int H, int W, int bits, const float* a, const float* b, int h, int w,
                      uint16_t* out, int on_device) {
  return guided_apply("af_guided_apply16: ", device_ordinal, full, H, W, bits, a, b, h, w, out, on_device);
}

// PSNR / SSIM between two sequences (fidelity.hip).  The refusals come before the device is touched; the per-frame sums are
// host memory whatever on_device says, the partials of the workgroups are added here in block order.
int af_fidelity(int device_ordinal, const uint8_t* a, const uint8_t* b, int n, int h, int w, int win, uint64_t* sse_out, double* ssim_out,
                double* ssim_map, int on_device) {
  const std::string who("af_fidelity: ");
  if (!a || !b) return refuse(who + "null pointer");
  if (!sse_out && !ssim_out && !ssim_map) return refuse(who + "no output asked for");
  if (ssim_map && !ssim_out) return refuse(who + "ssim_map needs ssim_out");
  if (n < 1) return refuse(who + "n < 1");
  if (win < 3 || win > 15 || win % 2 == 0) return refuse(who + "win must be odd and 3..15");
  if (h < win || h > 16384) return refuse(who + "h must be win..16384");
  if (w < win || w > 16384) return refuse(who + "w must be win..16384");
  UtilCall c(device_ordinal, on_device);
  const size_t fb = (size_t)n * h * w * 3, oh = (size_t)(h - win + 1), ow = (size_t)(w - win + 1);
  const double N = (double)(win * win), k1 = 0.01 * 255.0, k2 = 0.03 * 255.0;
  FidelityArgs g{};
  g.n = n; g.h = h; g.w = w; g.win = win;
  g.c1 = (k1 * k1) * (N * N); g.c2 = (k2 * k2) * (N * (N - 1.0));
  g.a = c.in(a, fb); g.b = c.in(b, fb);
  const size_t nblk = ssim_out ? ((3 * ow + 3 * AF_FID_TILE_X - 1) / (3 * AF_FID_TILE_X)) * ((oh + AF_FID_TILE_Y - 1) / AF_FID_TILE_Y)
                               : ((size_t)h * w * 3 + AF_FID_SSE_BYTES - 1) / AF_FID_SSE_BYTES;
  std::vector<unsigned long long> sse_part(sse_out ? (size_t)n * nblk * 3 : 0);
  std::vector<double> ssim_part(ssim_out ? (size_t)n * nblk * 3 : 0);
  if (sse_out) g.sse_part = c.fetch(sse_part.data(), sse_part.size() * 8);
  if (ssim_out) g.ssim_part = c.fetch(ssim_part.data(), ssim_part.size() * 8);
  if (ssim_map) g.map = c.out(ssim_map, (size_t)n * oh * ow * 3 * 8);
  if (!c.ok()) return c.status();
  if (int rc = ssim_out ? c.finish("k_fidelity_ssim", af_launch_fidelity_ssim(&g, nullptr)) : c.finish("k_fidelity_sse", af_launch_fidelity_sse(&g, nullptr))) return rc;
  for (size_t i = 0; i < (size_t)n * 3; ++i) {      // i = frame * 3 + channel
    const size_t f = i / 3, ch = i % 3;
    if (sse_out) {
      uint64_t t = 0;
      for (size_t k = 0; k < nblk; ++k) t += sse_part[(f * nblk + k) * 3 + ch];
      sse_out[i] = t;
    }
    if (ssim_out) {
      double t = 0.0;
      for (size_t k = 0; k < nblk; ++k) t += ssim_part[(f * nblk + k) * 3 + ch];
      ssim_out[i] = t / (double)(oh * ow);
    }
  }
  return AF_OK;
}

int af_flow_consistency(int device_ordinal, const float* f12, const float* f21, int h, int w, float* out,
                        int64_t pix_stride, int64_t offset, float thresh, int on_device) {
  if (!f12 || !f21 || !out || h <= 0 || w <= 0 || pix_stride <= 0) return refuse("af_flow_consistency: arguments");
  UtilCall c(device_ordinal, on_device);
  if (!c.ok()) return c.status();
  if (!on_device && (pix_stride != 1 || offset != 0)) return refuse("af_flow_consistency: host destinations must be contiguous");
  const size_t fb = (size_t)h * w * 8;
  const float *d12 = c.in(f12, fb), *d21 = c.in(f21, fb);
  float* o = c.out(out, (size_t)h * w * 4);
  if (!c.ok()) return c.status();
  ConsistencyArgs a{d12, d21, h, w, o, pix_stride, offset, thresh};
  return c.finish("k_flow_consistency", af_launch_consistency(&a, nullptr));
}

int af_warp_error_pair(int device_ordinal, const float* img1, const float* img2, const float* flow12, const float* flow21, int h, int w,
                       int align_corners, double* err, float* noc, float* warped, int on_device) {
  if (!img1 || !img2 || !flow12 || !flow21 || !err || h < 2 || w < 2 || (align_corners != 0 && align_corners != 1))
    return refuse("af_warp_error_pair: arguments");
  if ((int64_t)h * w > INT32_MAX / 4) return refuse("af_warp_error_pair: image too large");
  UtilCall c(device_ordinal, on_device);
  const int npix = h * w, nblk = (npix + 255) / 256;
  const size_t ib = (size_t)npix * 12, fb = (size_t)npix * 8;
  std::vector<double> part((size_t)nblk * 2);
  const float *d1 = c.in(img1, ib), *d2 = c.in(img2, ib), *d12 = c.in(flow12, fb), *d21 = c.in(flow21, fb);
  float* dn = noc ? c.out(noc, (size_t)npix * 4) : nullptr;
  float* dw = warped ? c.out(warped, ib) : nullptr;
  double* dp = c.fetch(part.data(), (size_t)nblk * 16);
  if (!c.ok()) return c.status();
  WarpErrArgs a{d1, d2, d12, d21, 0, 0, h, w, align_corners, dn, dw, dp};
  if (int rc = c.finish("k_warp_error", af_launch_warp_error(&a, 2, 1, nullptr))) return rc;
  *err = warp_error_of(part.data(), nblk, npix);
  return AF_OK;
}

}  // extern "C"
