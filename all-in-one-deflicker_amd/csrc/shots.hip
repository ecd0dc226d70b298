// shots.hip — exact luminance grids of uint8 RGB frames, the device side of the cut detector (shots.py).
// Cell (i, j) of a gh x gw grid over an h x w frame covers rows [i*h/gh, (i+1)*h/gh) and columns [j*w/gw, (j+1)*w/gw); its value
// is the integer sum of 77 R + 150 G + 29 B over the cell.  Integer arithmetic only: the result does not depend on the order of the
// sums, so the host may demand equality with numpy.  One workgroup per (strip of a cell, frame): a wave walks rows, its lanes walk
// the pixels of a row (a cell's row is 3 * cw consecutive bytes, aligned to nothing: 197 * 3 = 591 bytes per row), 64-bit
// accumulators throughout (a pixel is worth up to 65280, a 300 x 300 cell of white 5 875 200 000), wave reduction by shuffles, four
// values through LDS, one 64-bit vector store per workgroup.  The strips of a cell are added on the host (host_util.hip af_luma_grid).
#include "af_dev.h"
#include "elem.h"

namespace {

__global__ __launch_bounds__(256) void k_luma_grid(LumaArgs a, int f0) {
  __shared__ unsigned long long red[4];
  const int cells = a.gh * a.gw;
  const int cell = blockIdx.x / a.strips, strip = blockIdx.x - cell * a.strips;
  const int ci = cell / a.gw, cj = cell - ci * a.gw;
  const int f = f0 + (int)blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long acc = 0;
  if (cell < cells && f < a.n) {
    const int rc0 = (int)((long long)ci * a.h / a.gh), rc1 = (int)((long long)(ci + 1) * a.h / a.gh);
    const int c0 = (int)((long long)cj * a.w / a.gw), c1 = (int)((long long)(cj + 1) * a.w / a.gw);
    const long long rs = (long long)rc0 + (long long)strip * a.strip_rows;
    const int r0 = (int)(rs < rc1 ? rs : rc1), r1 = (int)(rs + a.strip_rows < rc1 ? rs + a.strip_rows : rc1);      // an empty strip writes 0
    const unsigned char* frame = a.src + (size_t)f * (size_t)a.h * (size_t)a.w * 3;      // 64-bit offsets: 16384^2 * 3 * n passes 2^32
    for (int r = r0 + wave; r < r1; r += 4) {
      const unsigned char* row = frame + ((size_t)r * (size_t)a.w + (size_t)c0) * 3;
#pragma unroll 4
      for (int x = lane; x < c1 - c0; x += 64) {
        const unsigned char* p = row + (size_t)x * 3;
        acc += 77u * p[0] + 150u * p[1] + 29u * p[2];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0 && cell < cells && f < a.n)
    a.part[((size_t)f * cells + cell) * a.strips + strip] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

extern "C" {
// Grid (gh * gw * strips, frames); a launch takes at most 65535 frames (gridDim.y), so a longer block goes in several.
int af_launch_luma_grid(const LumaArgs* a, hipStream_t s) {
  const unsigned gx = (unsigned)((long long)a->gh * a->gw * a->strips);
  for (int f0 = 0; f0 < a->n; f0 += 65535) {
    const int nf = a->n - f0 < 65535 ? a->n - f0 : 65535;
    hipLaunchKernelGGL(k_luma_grid, dim3(gx, (unsigned)nf), dim3(256), 0, s, *a, f0);
    const int e = (int)hipGetLastError();
    if (e) return e;
  }
  return 0;
}
}
