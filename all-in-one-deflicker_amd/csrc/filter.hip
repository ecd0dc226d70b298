// filter.hip — stage 2 of the pipeline (reference: src/neural_filter_and_refinement.py:44-130): the neural filter UNet
// (src/models/network_filter.py) and the local refinement TransformNet (src/models/network_local.py) in eval mode, one frame per call.
//
// Activations are NHWC fp32.  Every convolution of both nets is k_conv: the implicit-GEMM core of conv_gemm.h (shared with raft.hip's
// k_rconv; fp32-input matrix pipe, M = output pixels, N = output channels, K = (ky, kx, ci)) instantiated with reflection padding and
// without the batch index.  k_conv's epilogue applies none / ReLU / LeakyReLU(0.2) / tanh to sum + bias, adds an optional residual and
// stores into a channel slice of a wider buffer (pixel stride ldy), so every torch.cat of the nets is free: the producers write into the
// slices of one buffer.  The glue kernels are replicate pad, maxpool 2x2, bilinear x2 (align_corners=True, ATen's source-index
// arithmetic), nearest x2, the ConvLSTM finish with zero state and final = p2 + Y.  The host side (net tables, handle, frame graph) is
// at the end of this file; the layer record, the weight repack and the launch dispatch are conv_gemm.h's.
//
// Precision mode AF_FILTER_FP16 (af_filter_set_precision; both nets as the reference's modules compute them under fp16 autocast):
// every convolution runs as k_conv_h on conv_tile_h (conv_gemm_h.h, v_mfma_f32_32x32x16_f16): operands rounded to fp16 as they are
// gathered, exact products, an fp32 sum, y = fp16(sum + bias16), the activation in fp32 on y rounded once, then fp16(v + residual).
// The bilinear upsampling, the LSTM finish and final = pred + Y round where autocast would hold an fp16 tensor (their `half` flag);
// the kernels that only move values are shared.  The buffers stay NHWC fp32 and hold fp16-representable values.
#include <math.h>
#include <string.h>

#include "conv_gemm_h.h"

namespace {

struct ConvArgs {
  ConvGeom g;
  int act;                                // 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 tanh
  const float* res; long long ldr;        // residual added after the activation, or null
  float* y; long long ldy;                // output (Ho, Wo, Cout) at pixel stride ldy
  float* y2; long long ldy2;              // optional second copy of the output (a tensor that feeds two concatenations)
};

// conv_tile without the batch index, with reflection padding; the epilogue: activation, residual, store into one or two channel slices
template <int BN>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
  conv_tile<BN, false, true>(a.g, [=](int m, int co, float v) {
    if (a.act == 1) v = v > 0.f ? v : 0.f;
    else if (a.act == 2) v = v > 0.f ? v : v * 0.2f;
    else if (a.act == 3) v = tanhf(v);
    if (a.res) v = v + a.res[(size_t)m * a.ldr + co];
    a.y[(size_t)m * a.ldy + co] = v;
    if (a.y2) a.y2[(size_t)m * a.ldy2 + co] = v;
  });
}

// The fp16 mode's convolution: conv_tile_h hands y = fp16(sum + bias16); the activation is evaluated in fp32 on y and rounded to fp16
// once, the residual is added after that and the sum rounded once more; both stores write the same value.
template <int BN>
__global__ __launch_bounds__(256) void k_conv_h(ConvArgs a) {
  conv_tile_h<BN, false, true>(a.g, [=](int m, int co, float v) {
#pragma clang fp contract(off)
    if (a.act == 1) v = v > 0.f ? v : 0.f;
    else if (a.act == 2) v = round_h(v > 0.f ? v : v * 0.2f);
    else if (a.act == 3) v = round_h(tanhf(v));
    if (a.res) v = round_h(v + a.res[(size_t)m * a.ldr + co]);
    a.y[(size_t)m * a.ldy + co] = v;
    if (a.y2) a.y2[(size_t)m * a.ldy2 + co] = v;
  });
}

// InputPadder mode 'other' with F.pad(mode='replicate'): dst (Hp, Wp) at pixel stride ldd, channels [0, C) of src (h, w, C) from offset doff;
// `left` columns on the left, the rest on the right, all rows of the height pad at the bottom.
__global__ void k_pad_replicate(const float* src, int h, int w, int C, float* dst, int Hp, int Wp, int ldd, int doff, int left) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Hp * Wp * C) return;
  const int c = (int)(i % C); const long long p = i / C;
  const int y = (int)(p / Wp), x = (int)(p - (long long)y * Wp);
  const int sy = min(y, h - 1), sx = min(max(x - left, 0), w - 1);
  dst[p * ldd + doff + c] = src[((size_t)sy * w + sx) * C + c];
}

// The TransformNet input cat(p2, o1, p2, p1): (P, 12) from three (P, 3) tensors.
__global__ void k_pack12(const float* p2, const float* o1, const float* p1, float* x, long long P) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * 12) return;
  const long long p = i / 12; const int c = (int)(i - p * 12), g = c / 3, k = c - 3 * g;
  const float* s = g == 1 ? o1 : (g == 3 ? p1 : p2);
  x[i] = s[p * 3 + k];
}

// MaxPool2d(2, 2): x (H, W, C) at pixel stride ldx -> y (H/2, W/2, C) contiguous.
__global__ void k_maxpool2(const float* x, long long ldx, int H, int W, int C, float* y) {
  const int Ho = H / 2, Wo = W / 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Ho * Wo * C) return;
  const int c = (int)(i % C); const long long p = i / C;
  const int oy = (int)(p / Wo), ox = (int)(p - (long long)oy * Wo);
  const float* b = x + ((size_t)(2 * oy) * W + 2 * ox) * ldx + c;
  float v = b[0];
  const float v1 = b[ldx], v2 = b[(size_t)W * ldx], v3 = b[(size_t)(W + 1) * ldx];
  v = v1 > v ? v1 : v; v = v2 > v ? v2 : v; v = v3 > v ? v3 : v;
  y[i] = v;
}

// nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) as ATen's upsample_bilinear2d computes it: scale (in - 1) / (out - 1)
// in fp32, source index scale * dst, i1 = (int) src, lambda = src - i1, neighbour i1 + (i1 < in - 1).
// half: the fp32 result is rounded to fp16 once at the store (the fp16 mode: the same expression on fp16 values).
__global__ void k_up_bilinear2(const float* x, int H, int W, int C, float* y, int half) {
#pragma clang fp contract(off)
  const int Ho = 2 * H, Wo = 2 * W;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Ho * Wo * C) return;
  const int c = (int)(i % C); const long long p = i / C;
  const int oy = (int)(p / Wo), ox = (int)(p - (long long)oy * Wo);
  const float rh = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, rw = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
  const float hr = rh * (float)oy, wr = rw * (float)ox;
  const int h1 = (int)hr, w1 = (int)wr;
  const int hp = h1 < H - 1 ? 1 : 0, wp = w1 < W - 1 ? 1 : 0;
  const float l1h = hr - (float)h1, l0h = 1.f - l1h, l1w = wr - (float)w1, l0w = 1.f - l1w;
  const float* b = x + ((size_t)h1 * W + w1) * C + c;
  const float t = l0w * b[0] + l1w * b[(size_t)wp * C];
  const float u = l0w * b[(size_t)hp * W * C] + l1w * b[((size_t)hp * W + wp) * C];
  const float v = l0h * t + l1h * u;
  y[i] = half ? round_h(v) : v;
}

// nn.Upsample(scale_factor=2, mode='nearest'): source index floor(dst / 2).
__global__ void k_up_nearest2(const float* x, int H, int W, int C, float* y) {
  const int Wo = 2 * W;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)4 * H * W * C) return;
  const int c = (int)(i % C); const long long p = i / C;
  const int oy = (int)(p / Wo), ox = (int)(p - (long long)oy * Wo);
  y[i] = x[((size_t)(oy >> 1) * W + (ox >> 1)) * C + c];
}

// ConvLSTM with prev_state None (neural_filter_and_refinement.py:106): gates (P, 4 hc) chunked (in, remember, out, cell);
// cell = sigmoid(remember) * 0 + sigmoid(in) * tanh(cell_gate) = sigmoid(in) * tanh(cell_gate), hidden = sigmoid(out) * tanh(cell).
// half (the fp16 mode): every step rounds, i = fp16(sigmoid(in)), o = fp16(sigmoid(out)), g = fp16(tanh(cell_gate)), cell = fp16(i g),
// hidden = fp16(o tanh(cell)).  Autocast keeps cell and hidden in fp32 (prev_state is an fp32 zero tensor), but hidden's only consumer
// is a convolution that rounds as it gathers: rounding at the store gives that convolution the same operand bits.
__global__ void k_lstm_zero_state(const float* g, long long P, int hc, float* hidden, int half) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * hc) return;
  const long long p = i / hc; const int c = (int)(i - p * hc);
  const float* r = g + p * 4 * hc;
  const float gi = 1.f / (1.f + expf(-r[c])), go = 1.f / (1.f + expf(-r[2 * hc + c])), gc = tanhf(r[3 * hc + c]);
  if (half) {
#pragma clang fp contract(off)
    const float cell = round_h(round_h(gi) * round_h(gc));
    hidden[i] = round_h(round_h(go) * tanhf(cell));
    return;
  }
  hidden[i] = go * tanhf(gi * gc);
}

// half: the sum is rounded to fp16 (the fp16 mode)
__global__ void k_add(const float* a, const float* b, float* y, long long n, int half) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = a[i] + b[i];
  y[i] = half ? round_h(v) : v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

struct LayerDesc { int cout, cin, k, stride, bias, reflect, cin_used; };

// state_dict order of UNet(6, 3, 32) (network_filter.py:9-57): encoder1..4, bottleneck, (upconvN.1, decoderN) for N = 4..1, conv
const std::vector<LayerDesc>& unet_layers() {
  static const std::vector<LayerDesc> L = [] {
    std::vector<LayerDesc> v;
    int c = 6;
    for (int f : {32, 64, 128, 256, 512}) { v.push_back({f, c, 3, 1, 0, 0, c}); v.push_back({f, f, 3, 1, 0, 0, f}); c = f; }
    for (int f : {256, 128, 64, 32}) { v.push_back({f, 2 * f, 3, 1, 1, 0, 2 * f}); v.push_back({f, 2 * f, 3, 1, 0, 0, 2 * f}); v.push_back({f, f, 3, 1, 0, 0, f}); }
    v.push_back({3, 32, 1, 1, 1, 0, 32});
    return v;
  }();
  return L;
}

// state_dict order of TransformNet(nf 32, blocks 5, nc_in 12, nc_out 3) without the InstanceNorm buffers (network_local.py:60-86):
// conv1a, conv1b, conv2a, conv2b, conv3, ResBlocks.{0..4}.conv{1,2}, convlstm.Gates, deconv1, deconv2, deconv3.  The Gates conv reads
// cat(RB, hidden) with hidden = 0 on every frame: only its first 128 input channels are used (the rest multiply exact zeros).
const std::vector<LayerDesc>& local_layers() {
  static const std::vector<LayerDesc> L = [] {
    std::vector<LayerDesc> v;
    v.push_back({32, 6, 7, 1, 1, 1, 6}); v.push_back({32, 6, 7, 1, 1, 1, 6});
    v.push_back({64, 32, 3, 2, 1, 1, 32}); v.push_back({64, 32, 3, 2, 1, 1, 32});
    v.push_back({128, 128, 3, 2, 1, 1, 128});
    for (int b = 0; b < 10; ++b) v.push_back({128, 128, 3, 1, 1, 1, 128});
    v.push_back({512, 256, 3, 1, 1, 0, 128});
    v.push_back({64, 128, 3, 1, 1, 1, 128}); v.push_back({32, 128, 3, 1, 1, 1, 128}); v.push_back({3, 64, 7, 1, 1, 1, 64});
    return v;
  }();
  return L;
}

size_t layer_params(const LayerDesc& d) { return (size_t)d.cout * d.cin * d.k * d.k + (d.bias ? d.cout : 0); }

// prec picks the kernel family and the weight image: AF_FILTER_FP16 needs L's fp16 image (upload_layer_h)
hipError_t launch_conv(int prec, const ConvLayer& L, const float* x, long long ldx, int H, int W, float* y, long long ldy, int act,
                       const float* res, long long ldr, float* y2, long long ldy2, hipStream_t s) {
  if (prec == AF_FILTER_FP16) {
    const ConvArgs a{conv_geom_h(L, x, ldx, 1, H, W), act, res, ldr, y, ldy, y2, ldy2};
    return launch_conv_family(k_conv_h<32>, k_conv_h<64>, k_conv_h<128>, a, s);
  }
  const ConvArgs a{conv_geom(L, x, ldx, 1, H, W), act, res, ldr, y, ldy, y2, ldy2};
  return launch_conv_family(k_conv<32>, k_conv<64>, k_conv<128>, a, s);
}

}  // namespace

struct af_filter : DevPool {
  int device = 0, h = 0, w = 0, Hp = 0, Wp = 0, left = 0;
  hipStream_t stream = nullptr;
  std::vector<ConvLayer> net[2];
  bool loaded[2] = {false, false};
  int prec = AF_FILTER_FP32;      // af_filter_set_precision
  int frame = 0;                  // frames since create / reset: 0 -> the frame-0 rule
  bool local_ran = false;         // the last frame ran the TransformNet (its named activations are valid)
  // buffers (NHWC fp32); P = Hp * Wp, freed by the pool
  float *in_c = nullptr, *in_s = nullptr;                     // staging of host inputs (h, w, 3)
  float *x0, *cat1, *cat2, *cat3, *cat4, *pool, *tmp, *bott, *dec4, *dec3, *dec2, *dec1, *up, *pred;
  float *xt, *c1, *e1b, *c2, *e3in, *e3, *rbt, *rb[2], *gates, *hidden, *y, *o1, *p1, *fin;
  float* rb_last = nullptr;

  ~af_filter() {
    for (auto& n : net) for (auto& L : n) free_layer(L);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

// A named intermediate of the last frame: base pointer, pyramid level (size Hp >> lvl, Wp >> lvl), channels, pixel stride.
struct Named { const char* name; float* af_filter::*buf; int off, lvl, C, ld, local; };
const Named kNamed[] = {
  {"input", &af_filter::x0, 0, 0, 6, 6, 0},
  {"enc1", &af_filter::cat1, 32, 0, 32, 64, 0}, {"enc2", &af_filter::cat2, 64, 1, 64, 128, 0},
  {"enc3", &af_filter::cat3, 128, 2, 128, 256, 0}, {"enc4", &af_filter::cat4, 256, 3, 256, 512, 0},
  {"bottleneck", &af_filter::bott, 0, 4, 512, 512, 0},
  {"dec4", &af_filter::dec4, 0, 3, 256, 256, 0}, {"dec3", &af_filter::dec3, 0, 2, 128, 128, 0},
  {"dec2", &af_filter::dec2, 0, 1, 64, 64, 0}, {"dec1", &af_filter::dec1, 0, 0, 32, 32, 0},
  {"pred", &af_filter::pred, 0, 0, 3, 3, 0},
  {"E1a", &af_filter::c1, 32, 0, 32, 64, 1}, {"E1b", &af_filter::e1b, 0, 0, 32, 32, 1},
  {"E2a", &af_filter::c2, 64, 1, 64, 128, 1}, {"E2b", &af_filter::e3in, 64, 1, 64, 128, 1},
  {"E3", &af_filter::e3, 0, 2, 128, 128, 1}, {"RB", nullptr, 0, 2, 128, 128, 1},
  {"hidden", &af_filter::hidden, 0, 2, 128, 128, 1},
  {"D2", &af_filter::c2, 0, 1, 64, 128, 1}, {"D1", &af_filter::c1, 0, 0, 32, 64, 1},
  {"Y", &af_filter::y, 0, 0, 3, 3, 1}, {"final", &af_filter::fin, 0, 0, 3, 3, 0},
};

int pad_to_32(int n) { return n + ((((n / 32) + 1) * 32 - n) % 32); }

hipError_t run_unet(af_filter* f) {
  const auto& L = f->net[0];
  const int H = f->Hp, W = f->Wp, half = f->prec == AF_FILTER_FP16;
  hipStream_t s = f->stream;
  hipError_t e;
#define FCHK(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
  // encoders: conv, ReLU, conv, ReLU; the block output lands in its decoder's concatenation buffer behind the upconv half
  float* cats[4] = {f->cat1, f->cat2, f->cat3, f->cat4};
  const float* in = f->x0; long long ldin = 6;
  int h = H, w = W;
  for (int lv = 0; lv < 4; ++lv) {
    const int c = 32 << lv;
    FCHK(launch_conv(f->prec, L[2 * lv], in, ldin, h, w, f->tmp, c, 1, nullptr, 0, nullptr, 0, s));
    FCHK(launch_conv(f->prec, L[2 * lv + 1], f->tmp, c, h, w, cats[lv] + c, 2 * c, 1, nullptr, 0, nullptr, 0, s));
    hipLaunchKernelGGL(k_maxpool2, dim3(nblk((long long)(h / 2) * (w / 2) * c)), dim3(256), 0, s, cats[lv] + c, (long long)2 * c, h, w, c, f->pool);
    FCHK(hipGetLastError());
    in = f->pool; ldin = c; h /= 2; w /= 2;
  }
  FCHK(launch_conv(f->prec, L[8], f->pool, 256, h, w, f->tmp, 512, 1, nullptr, 0, nullptr, 0, s));
  FCHK(launch_conv(f->prec, L[9], f->tmp, 512, h, w, f->bott, 512, 1, nullptr, 0, nullptr, 0, s));
  // decoders: upconv = bilinear x2 then conv3x3 + bias into the first half of the concatenation, then the block
  float* decs[4] = {f->dec4, f->dec3, f->dec2, f->dec1};
  const float* cur = f->bott; int cc = 512;
  for (int i = 0; i < 4; ++i) {
    const int lv = 3 - i, c = 32 << lv;
    hipLaunchKernelGGL(k_up_bilinear2, dim3(nblk((long long)4 * h * w * cc)), dim3(256), 0, s, cur, h, w, cc, f->up, half);
    FCHK(hipGetLastError());
    h *= 2; w *= 2;
    FCHK(launch_conv(f->prec, L[10 + 3 * i], f->up, cc, h, w, cats[lv], 2 * c, 0, nullptr, 0, nullptr, 0, s));
    FCHK(launch_conv(f->prec, L[11 + 3 * i], cats[lv], 2 * c, h, w, f->tmp, c, 1, nullptr, 0, nullptr, 0, s));
    FCHK(launch_conv(f->prec, L[12 + 3 * i], f->tmp, c, h, w, decs[i], c, 1, nullptr, 0, nullptr, 0, s));
    cur = decs[i]; cc = c;
  }
  FCHK(launch_conv(f->prec, L[22], f->dec1, 32, H, W, f->pred, 3, 0, nullptr, 0, nullptr, 0, s));
  return hipSuccess;
}

hipError_t run_local(af_filter* f) {
  const auto& L = f->net[1];
  const int H = f->Hp, W = f->Wp;
  const long long P = (long long)H * W;
  hipStream_t s = f->stream;
  hipError_t e;
  hipLaunchKernelGGL(k_pack12, dim3(nblk(P * 12)), dim3(256), 0, s, f->pred, f->o1, f->p1, f->xt, P);
  FCHK(hipGetLastError());
  FCHK(launch_conv(f->prec, L[0], f->xt, 12, H, W, f->c1 + 32, 64, 2, nullptr, 0, nullptr, 0, s));           // E1a = leaky(conv1a(p2, o1))
  FCHK(launch_conv(f->prec, L[1], f->xt + 6, 12, H, W, f->e1b, 32, 2, nullptr, 0, nullptr, 0, s));          // E1b = leaky(conv1b(p2, p1))
  FCHK(launch_conv(f->prec, L[2], f->c1 + 32, 64, H, W, f->c2 + 64, 128, 2, nullptr, 0, f->e3in, 128, s));  // E2a into cat(D2, E2a) and cat(E2a, E2b)
  FCHK(launch_conv(f->prec, L[3], f->e1b, 32, H, W, f->e3in + 64, 128, 2, nullptr, 0, nullptr, 0, s));      // E2b
  const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4;
  FCHK(launch_conv(f->prec, L[4], f->e3in, 128, h2, w2, f->e3, 128, 2, nullptr, 0, nullptr, 0, s));         // E3
  const float* cur = f->e3;
  for (int b = 0; b < 5; ++b) {       // ResidualBlock: conv1, leaky, conv2, + x
    FCHK(launch_conv(f->prec, L[5 + 2 * b], cur, 128, h4, w4, f->rbt, 128, 2, nullptr, 0, nullptr, 0, s));
    FCHK(launch_conv(f->prec, L[6 + 2 * b], f->rbt, 128, h4, w4, f->rb[b & 1], 128, 0, cur, 128, nullptr, 0, s));
    cur = f->rb[b & 1];
  }
  f->rb_last = const_cast<float*>(cur);
  FCHK(launch_conv(f->prec, L[15], cur, 128, h4, w4, f->gates, 512, 0, nullptr, 0, nullptr, 0, s));
  hipLaunchKernelGGL(k_lstm_zero_state, dim3(nblk((long long)h4 * w4 * 128)), dim3(256), 0, s, f->gates, (long long)h4 * w4, 128, f->hidden, (int)(f->prec == AF_FILTER_FP16));
  FCHK(hipGetLastError());
  hipLaunchKernelGGL(k_up_nearest2, dim3(nblk((long long)4 * h4 * w4 * 128)), dim3(256), 0, s, f->hidden, h4, w4, 128, f->up);
  FCHK(hipGetLastError());
  FCHK(launch_conv(f->prec, L[16], f->up, 128, h2, w2, f->c2, 128, 2, nullptr, 0, nullptr, 0, s));          // D2 = leaky(deconv1(hidden))
  hipLaunchKernelGGL(k_up_nearest2, dim3(nblk((long long)4 * h2 * w2 * 128)), dim3(256), 0, s, f->c2, h2, w2, 128, f->up);
  FCHK(hipGetLastError());
  FCHK(launch_conv(f->prec, L[17], f->up, 128, H, W, f->c1, 64, 2, nullptr, 0, nullptr, 0, s));             // D1 = leaky(deconv2(cat(D2, E2a)))
  FCHK(launch_conv(f->prec, L[18], f->c1, 64, H, W, f->y, 3, 3, nullptr, 0, nullptr, 0, s));                // Y = tanh(deconv3(cat(D1, E1a)))
  return hipSuccess;
#undef FCHK
}

}  // namespace

extern "C" {

int af_filter_create(int device_ordinal, int h, int w, af_filter** out) {
  if (!out) return fail(AF_EINVAL, "af_filter_create: null argument");
  *out = nullptr;
  // the deepest TransformNet level is (Hp / 4, Wp / 4) and reflection-pads by 1: at least 2 rows / columns there
  if (h <= 0 || w <= 0 || h > 16384 || w > 16384) return fail(AF_EINVAL, "af_filter_create: h and w must be 1..16384");
  hipError_t e = hipSetDevice(device_ordinal);
  if (e != hipSuccess) return hfail("af_filter_create: hipSetDevice", e);
  af_filter* f = new af_filter();
  f->device = device_ordinal; f->h = h; f->w = w;
  f->Hp = pad_to_32(h); f->Wp = pad_to_32(w); f->left = (f->Wp - w) / 2;
  const size_t P = (size_t)f->Hp * f->Wp;
  e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
  f->in_c = f->alloc((size_t)h * w * 3, e); f->in_s = f->alloc((size_t)h * w * 3, e);
  f->x0 = f->alloc(P * 6, e); f->cat1 = f->alloc(P * 64, e); f->cat2 = f->alloc(P * 32, e); f->cat3 = f->alloc(P * 16, e);
  f->cat4 = f->alloc(P * 8, e); f->pool = f->alloc(P * 8, e); f->tmp = f->alloc(P * 32, e); f->bott = f->alloc(P * 2, e);
  f->dec4 = f->alloc(P * 4, e); f->dec3 = f->alloc(P * 8, e); f->dec2 = f->alloc(P * 16, e); f->dec1 = f->alloc(P * 32, e);
  f->up = f->alloc(P * 128, e); f->pred = f->alloc(P * 3, e);
  f->xt = f->alloc(P * 12, e); f->c1 = f->alloc(P * 64, e); f->e1b = f->alloc(P * 32, e); f->c2 = f->alloc(P * 32, e);
  f->e3in = f->alloc(P * 32, e); f->e3 = f->alloc(P * 8, e); f->rbt = f->alloc(P * 8, e); f->rb[0] = f->alloc(P * 8, e);
  f->rb[1] = f->alloc(P * 8, e); f->gates = f->alloc(P * 32, e); f->hidden = f->alloc(P * 8, e); f->y = f->alloc(P * 3, e);
  f->o1 = f->alloc(P * 3, e); f->p1 = f->alloc(P * 3, e); f->fin = f->alloc(P * 3, e);
  if (e != hipSuccess) { delete f; return hfail("af_filter_create", e); }
  *out = f;
  return AF_OK;
}

void af_filter_destroy(af_filter* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  (void)hipStreamSynchronize(f->stream);
  delete f;
}

size_t af_filter_param_count(const af_filter* f, int net) {
  if (!f || (net != 0 && net != 1)) return 0;
  size_t n = 0;
  for (const auto& d : net == 0 ? unet_layers() : local_layers()) n += layer_params(d);
  return n;
}

int af_filter_set_params(af_filter* f, int net, const float* flat, size_t n) {
  if (!f || !flat || (net != 0 && net != 1)) return fail(AF_EINVAL, "af_filter_set_params: arguments");
  if (n != af_filter_param_count(f, net)) return fail(AF_EINVAL, "af_filter_set_params: expected " + std::to_string(af_filter_param_count(f, net)) + " parameters, got " + std::to_string(n));
  hipError_t e = hipSetDevice(f->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  if ((e = hipStreamSynchronize(f->stream)) != hipSuccess) return hfail("af_filter_set_params", e);
  auto& v = f->net[net];
  for (auto& L : v) free_layer(L);
  v.clear(); f->loaded[net] = false;
  size_t off = 0;
  for (const auto& d : net == 0 ? unet_layers() : local_layers()) {
    ConvLayer L;
    const float* w = flat + off; off += (size_t)d.cout * d.cin * d.k * d.k;
    const float* b = d.bias ? flat + off : nullptr; off += d.bias ? d.cout : 0;
    e = upload_layer(L, d.cin, d.cin_used, d.k, d.k, d.stride, d.reflect, {w}, {b}, d.cout);
    if (e == hipSuccess) e = upload_layer_h(L, d.cin, {w}, {b}, d.cout);      // both images stay resident: the precision switches at any time
    if (e != hipSuccess) { free_layer(L); return hfail("af_filter_set_params", e); }
    v.push_back(L);
  }
  f->loaded[net] = true;
  return AF_OK;
}

int af_filter_reset(af_filter* f) {
  if (!f) return fail(AF_EINVAL, "af_filter_reset: null handle");
  f->frame = 0; f->local_ran = false;
  return AF_OK;
}

int af_filter_set_precision(af_filter* f, int precision) {
  if (!f) return fail(AF_EINVAL, "af_filter_set_precision: null handle");
  if (precision != AF_FILTER_FP32 && precision != AF_FILTER_FP16)
    return fail(AF_EINVAL, "af_filter_set_precision: precision must be AF_FILTER_FP32 (0) or AF_FILTER_FP16 (1), got " + std::to_string(precision));
  hipError_t e = hipSetDevice(f->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  if ((e = hipStreamSynchronize(f->stream)) != hipSuccess) return hfail("af_filter_set_precision", e);
  f->prec = precision;
  return af_filter_reset(f);      // the recurrent state (o1, p1) belongs to the arithmetic that wrote it
}

int af_filter_get_precision(const af_filter* f, int* precision) {
  if (!f || !precision) return fail(AF_EINVAL, "af_filter_get_precision: null argument");
  *precision = f->prec;
  return AF_OK;
}

int af_filter_frame(af_filter* f, const float* content, const float* style, float* pred_out, float* final_out, int on_device) {
  if (!f || !content || !style) return fail(AF_EINVAL, "af_filter_frame: arguments");
  if (!f->loaded[0] || !f->loaded[1]) return fail(AF_ESTATE, "af_filter_frame: parameters of both nets must be set first");
  hipError_t e = hipSetDevice(f->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
  const size_t ib = (size_t)f->h * f->w * 3 * sizeof(float), ob = (size_t)f->Hp * f->Wp * 3 * sizeof(float);
  const long long P = (long long)f->Hp * f->Wp;
  hipStream_t s = f->stream;
  const float *c = content, *st = style;
  if (!on_device) {
    if ((e = hipMemcpyAsync(f->in_c, content, ib, hipMemcpyHostToDevice, s)) != hipSuccess) return hfail("upload content", e);
    if ((e = hipMemcpyAsync(f->in_s, style, ib, hipMemcpyHostToDevice, s)) != hipSuccess) return hfail("upload style", e);
    c = f->in_c; st = f->in_s;
  } else if ((e = hipDeviceSynchronize()) != hipSuccess) {       // device inputs may come from another stream of this device
    return hfail("af_filter_frame", e);
  }
  hipLaunchKernelGGL(k_pad_replicate, dim3(nblk(P * 3)), dim3(256), 0, s, c, f->h, f->w, 3, f->x0, f->Hp, f->Wp, 6, 0, f->left);
  hipLaunchKernelGGL(k_pad_replicate, dim3(nblk(P * 3)), dim3(256), 0, s, st, f->h, f->w, 3, f->x0, f->Hp, f->Wp, 6, 3, f->left);
  if ((e = hipGetLastError()) != hipSuccess) return hfail("k_pad_replicate", e);
  if ((e = run_unet(f)) != hipSuccess) return hfail("filter net", e);
  if (f->frame == 0) {
    // frame 0: o1 = p1 = pred, final = pred
    for (float* d : {f->o1, f->p1, f->fin})
      if ((e = hipMemcpyAsync(d, f->pred, ob, hipMemcpyDeviceToDevice, s)) != hipSuccess) return hfail("frame 0 state", e);
    f->local_ran = false;
  } else {
    if ((e = run_local(f)) != hipSuccess) return hfail("refinement net", e);
    hipLaunchKernelGGL(k_add, dim3(nblk(P * 3)), dim3(256), 0, s, f->pred, f->y, f->fin, P * 3, (int)(f->prec == AF_FILTER_FP16));     // final = p2 + Y
    if ((e = hipGetLastError()) != hipSuccess) return hfail("k_add", e);
    if ((e = hipMemcpyAsync(f->p1, f->pred, ob, hipMemcpyDeviceToDevice, s)) != hipSuccess) return hfail("state", e);
    if ((e = hipMemcpyAsync(f->o1, f->fin, ob, hipMemcpyDeviceToDevice, s)) != hipSuccess) return hfail("state", e);
    f->local_ran = true;
  }
  ++f->frame;
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (pred_out && (e = hipMemcpyAsync(pred_out, f->pred, ob, k, s)) != hipSuccess) return hfail("copy pred", e);
  if (final_out && (e = hipMemcpyAsync(final_out, f->fin, ob, k, s)) != hipSuccess) return hfail("copy final", e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hfail("af_filter_frame", e);
  return AF_OK;
}

int af_filter_debug_activation(af_filter* f, const char* name, float* out, size_t n) {
  if (!f || !name || !out) return fail(AF_EINVAL, "af_filter_debug_activation: arguments");
  for (const Named& d : kNamed) {
    if (strcmp(d.name, name) != 0) continue;
    if (f->frame == 0) return fail(AF_ESTATE, "af_filter_debug_activation: no frame has run");
    if (d.local && !f->local_ran) return fail(AF_ESTATE, std::string("af_filter_debug_activation: the refinement net did not run on the last frame (") + name + ")");
    const size_t hh = (size_t)(f->Hp >> d.lvl), ww = (size_t)(f->Wp >> d.lvl);
    if (n != hh * ww * d.C) return fail(AF_EINVAL, std::string("af_filter_debug_activation: ") + name + " has " + std::to_string(hh * ww * d.C) + " values");
    const float* src = (d.buf ? f->*(d.buf) : f->rb_last) + d.off;
    hipError_t e = hipSetDevice(f->device); if (e != hipSuccess) return hfail("hipSetDevice", e);
    if ((e = hipStreamSynchronize(f->stream)) != hipSuccess) return hfail("af_filter_debug_activation", e);
    if ((e = hipMemcpy2D(out, (size_t)d.C * 4, src, (size_t)d.ld * 4, (size_t)d.C * 4, hh * ww, hipMemcpyDeviceToHost)) != hipSuccess)
      return hfail("af_filter_debug_activation", e);
    return AF_OK;
  }
  return fail(AF_EINVAL, std::string("af_filter_debug_activation: unknown name ") + name);
}

static int conv2d_impl(const std::string& who, int prec, int device_ordinal, const float* x, int h, int w, int cin, const float* weight, const float* bias,
                       int cout, int k, int stride, int pad_mode, int act, const float* residual, float* y, int on_device) {
  if (prec != AF_FILTER_FP32 && prec != AF_FILTER_FP16)
    return fail(AF_EINVAL, who + ": precision must be AF_FILTER_FP32 (0) or AF_FILTER_FP16 (1), got " + std::to_string(prec));
  if (!x || !weight || !y || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || (k != 1 && k != 3 && k != 7) || (stride != 1 && stride != 2) ||
      (pad_mode != 0 && pad_mode != 1) || act < 0 || act > 3)
    return fail(AF_EINVAL, who + ": arguments");
  if (pad_mode == 1 && (h <= k / 2 || w <= k / 2)) return fail(AF_EINVAL, who + ": reflection padding needs h, w > k / 2");
  if ((long long)h * w * std::max(cin, cout) > (1LL << 31)) return fail(AF_EINVAL, who + ": tensor too large");
  if (prec == AF_FILTER_FP16 && (h > 16384 || w > 16384)) return fail(AF_EINVAL, who + ": the fp16 tile packs a pixel's row and column into 16 bits each: h and w at most 16384");
  hipError_t e = hipSetDevice(device_ordinal); if (e != hipSuccess) return hfail("hipSetDevice", e);
  const int ho = (h + 2 * (k / 2) - k) / stride + 1, wo = (w + 2 * (k / 2) - k) / stride + 1;
  const float *hwp = weight, *hbp = bias;
  std::vector<float> hw, hb;
  // the weights are repacked on the host: fetch them if they live on the device
  if (on_device) {
    hw.resize((size_t)cout * cin * k * k); hb.resize(bias ? cout : 0);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hfail(who.c_str(), e);
    if ((e = hipMemcpy(hw.data(), weight, hw.size() * 4, hipMemcpyDeviceToHost)) != hipSuccess) return hfail((who + " weights").c_str(), e);
    if (bias && (e = hipMemcpy(hb.data(), bias, hb.size() * 4, hipMemcpyDeviceToHost)) != hipSuccess) return hfail((who + " bias").c_str(), e);
    hwp = hw.data(); hbp = bias ? hb.data() : nullptr;
  }
  ConvLayer L;
  e = upload_layer(L, cin, cin, k, k, stride, pad_mode, {hwp}, {hbp}, cout);
  if (e == hipSuccess && prec == AF_FILTER_FP16) e = upload_layer_h(L, cin, {hwp}, {hbp}, cout);
  if (e != hipSuccess) { free_layer(L); return hfail(who.c_str(), e); }
  const size_t xb = (size_t)h * w * cin * 4, yb = (size_t)ho * wo * cout * 4;
  float *dx = nullptr, *dr = nullptr, *dy = nullptr;
  std::vector<void*> own;
  auto cleanup = [&]() { free_layer(L); for (void* p : own) (void)hipFree(p); };
  auto dalloc = [&](void** p, size_t b) { hipError_t r = hipMalloc(p, std::max<size_t>(b, 4)); if (r == hipSuccess) own.push_back(*p); return r; };
  if (on_device) { dx = const_cast<float*>(x); dr = const_cast<float*>(residual); dy = y; }
  else {
    if ((e = dalloc((void**)&dx, xb)) != hipSuccess || (e = dalloc((void**)&dy, yb)) != hipSuccess) { cleanup(); return hfail(who.c_str(), e); }
    if ((e = hipMemcpy(dx, x, xb, hipMemcpyHostToDevice)) != hipSuccess) { cleanup(); return hfail(who.c_str(), e); }
    if (residual) {
      if ((e = dalloc((void**)&dr, yb)) != hipSuccess || (e = hipMemcpy(dr, residual, yb, hipMemcpyHostToDevice)) != hipSuccess) { cleanup(); return hfail(who.c_str(), e); }
    }
  }
  e = launch_conv(prec, L, dx, cin, h, w, dy, cout, act, dr, cout, nullptr, 0, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess && !on_device) e = hipMemcpy(y, dy, yb, hipMemcpyDeviceToHost);
  cleanup();
  return e == hipSuccess ? AF_OK : hfail(who.c_str(), e);
}

int af_conv2d(int device_ordinal, const float* x, int h, int w, int cin, const float* weight, const float* bias, int cout, int k, int stride,
              int pad_mode, int act, const float* residual, float* y, int on_device) {
  return conv2d_impl("af_conv2d", AF_FILTER_FP32, device_ordinal, x, h, w, cin, weight, bias, cout, k, stride, pad_mode, act, residual, y, on_device);
}

int af_conv2d_prec(int precision, int device_ordinal, const float* x, int h, int w, int cin, const float* weight, const float* bias, int cout, int k,
                   int stride, int pad_mode, int act, const float* residual, float* y, int on_device) {
  return conv2d_impl("af_conv2d_prec", precision, device_ordinal, x, h, w, cin, weight, bias, cout, k, stride, pad_mode, act, residual, y, on_device);
}

}  // extern "C"
