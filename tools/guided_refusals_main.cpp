// guided_refusals_main.cpp — the argument checks of af_guided_coeffs / af_guided_apply and their colour-guide siblings (csrc/host_util.hip) in a stand-alone program, for a
// host sanitizer.  Every call here is refused before the wrapper touches the device, so the program needs no GPU.  Build and run
// (tools/README.md): host_util.hip compiled with -Xarch_host -fsanitize=address,undefined, linked with the library's other objects.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/atlasfit.h"

static int failures = 0;

static void expect(int rc, const char* msg) {
  const char* got = af_last_error(nullptr);
  if (rc != AF_EINVAL || std::strcmp(got, msg) != 0) {
    std::printf("FAIL: rc %d, message \"%s\", expected \"%s\"\n", rc, got, msg);
    ++failures;
  }
}

int main() {
  const int h = 4, w = 6, H = 8, W = 12;
  std::vector<uint8_t> pin(h * w * 3), pout(h * w * 3), full(H * W * 3), out(H * W * 3);
  std::vector<float> a(h * w * 3), b(h * w * 3);
  expect(af_guided_coeffs(0, nullptr, pout.data(), h, w, 8, 64.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: null pointer");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, 64.f, a.data(), nullptr, nullptr, 0), "af_guided_coeffs: null pointer");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 0, 64.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: r must be 1..32");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 33, 64.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: r must be 1..32");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, 0.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: eps must be finite and > 0");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, -1.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: eps must be finite and > 0");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, NAN, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: eps must be finite and > 0");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, INFINITY, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: eps must be finite and > 0");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), 0, w, 8, 64.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: h must be 1..16384");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, 16385, 8, 64.f, a.data(), b.data(), nullptr, 0), "af_guided_coeffs: w must be 1..16384");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, 64.f, a.data(), b.data(), a.data(), 0), "af_guided_coeffs: work is device memory: host pointers take none");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, 64.f, a.data(), a.data(), nullptr, 0), "af_guided_coeffs: a_out aliases b_out");
  expect(af_guided_coeffs(0, pin.data(), pout.data(), h, w, 8, 64.f, a.data(), b.data(), a.data(), 1), "af_guided_coeffs: work aliases an output");
  expect(af_guided_apply(0, nullptr, H, W, a.data(), b.data(), h, w, out.data(), 0), "af_guided_apply: null pointer");
  expect(af_guided_apply(0, full.data(), 0, W, a.data(), b.data(), h, w, out.data(), 0), "af_guided_apply: H must be 1..16384");
  expect(af_guided_apply(0, full.data(), H, 16385, a.data(), b.data(), h, w, out.data(), 0), "af_guided_apply: W must be 1..16384");
  expect(af_guided_apply(0, full.data(), H, W, a.data(), b.data(), 0, w, out.data(), 0), "af_guided_apply: h must be 1..16384");
  expect(af_guided_apply(0, full.data(), H, W, a.data(), b.data(), h, 16385, out.data(), 0), "af_guided_apply: w must be 1..16384");
  expect(af_guided_apply(0, full.data(), 3, W, a.data(), b.data(), h, w, out.data(), 0), "af_guided_apply: the proxy is larger than the full frame");
  expect(af_guided_apply(0, full.data(), H, 5, a.data(), b.data(), h, w, out.data(), 0), "af_guided_apply: the proxy is larger than the full frame");
  expect(af_guided_apply(0, full.data(), H, W, a.data(), b.data(), h, w, full.data(), 0), "af_guided_apply: the output aliases an input");
  // the colour guide: A of 9 h w floats, the siblings' refusals and the eps floor
  std::vector<float> A(h * w * 9);
  std::vector<uint16_t> full16(H * W * 3), out16(H * W * 3);
  expect(af_guided_coeffs_colour(0, nullptr, pout.data(), h, w, 8, 64.f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: null pointer");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, 64.f, nullptr, b.data(), nullptr, 0), "af_guided_coeffs_colour: null pointer");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 0, 64.f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: r must be 1..32");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 33, 64.f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: r must be 1..32");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, 0.f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: eps must be finite and >= 2^-20");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, 0x1p-21f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: eps must be finite and >= 2^-20");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, NAN, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: eps must be finite and >= 2^-20");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, INFINITY, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: eps must be finite and >= 2^-20");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), 0, w, 8, 64.f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: h must be 1..16384");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, 16385, 8, 64.f, A.data(), b.data(), nullptr, 0), "af_guided_coeffs_colour: w must be 1..16384");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, 64.f, A.data(), b.data(), A.data(), 0), "af_guided_coeffs_colour: work is device memory: host pointers take none");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, 64.f, A.data(), A.data() + 8 * h * w, nullptr, 0), "af_guided_coeffs_colour: a_out aliases b_out");
  expect(af_guided_coeffs_colour(0, pin.data(), pout.data(), h, w, 8, 64.f, A.data(), b.data(), A.data(), 1), "af_guided_coeffs_colour: work aliases an output");
  expect(af_guided_apply_colour(0, nullptr, H, W, A.data(), b.data(), h, w, out.data(), 0), "af_guided_apply_colour: null pointer");
  expect(af_guided_apply_colour(0, full.data(), 0, W, A.data(), b.data(), h, w, out.data(), 0), "af_guided_apply_colour: H must be 1..16384");
  expect(af_guided_apply_colour(0, full.data(), H, W, A.data(), b.data(), h, 16385, out.data(), 0), "af_guided_apply_colour: w must be 1..16384");
  expect(af_guided_apply_colour(0, full.data(), 3, W, A.data(), b.data(), h, w, out.data(), 0), "af_guided_apply_colour: the proxy is larger than the full frame");
  expect(af_guided_apply_colour(0, full.data(), H, W, A.data(), b.data(), h, w, full.data(), 0), "af_guided_apply_colour: the output aliases an input");
  expect(af_guided_apply_colour16(0, full16.data(), H, W, 7, A.data(), b.data(), h, w, out16.data(), 0), "af_guided_apply_colour16: bits must be 8..16");
  expect(af_guided_apply_colour16(0, (const uint16_t*)((const char*)full16.data() + 1), H, W, 10, A.data(), b.data(), h, w, out16.data(), 0),
         "af_guided_apply_colour16: uint16 pointers must be 2-byte aligned");
  expect(af_guided_apply_colour16(0, full16.data(), H, W, 10, A.data(), b.data(), h, w, full16.data(), 0), "af_guided_apply_colour16: the output aliases an input");
  std::printf(failures ? "%d refusals failed\n" : "all refusals as named (%d failed)\n", failures);
  return failures ? 1 : 0;
}
