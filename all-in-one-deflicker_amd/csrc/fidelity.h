// fidelity.h — the tile of the SSIM kernel (fidelity.hip), shared with the host entry (host_util.hip af_fidelity), which sizes the partial
// sums by it, and read by the tests, which place their shapes around its edges.  One workgroup of 256 threads serves the windows whose
// top-left pixel lies in a tile of AF_FID_TILE_X pixels (three channels each) by AF_FID_TILE_Y rows.
#pragma once
#define AF_FID_TILE_X 32
#define AF_FID_TILE_Y 16
#define AF_FID_SSE_BYTES 24576      // bytes of a frame one workgroup of the SSE-only kernel reads: 256 threads x 8 rounds x 12 bytes
