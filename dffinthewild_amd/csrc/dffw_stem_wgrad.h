// Weight gradient of the stem, the dilated 1x9x9 conv of the image stack: the launch contract between dffw_stem_wgrad.hip
// (kernels) and dffw_grad.cpp (C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

namespace stemw {
constexpr int CO = 8, CI = 3, K = 9, DIL = 2, PAD = 8;   // Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2))
constexpr int TY = 16, TX = 32;                          // a unit: TY x TX pixels of one slice of one sample = 16 chunks of 32 pixels (2 rows x 16 columns)
constexpr int FY = TY + 2 * PAD, FX = TX + 2 * PAD;      // its footprint in x: 32 x 48 pixels per input plane
constexpr int COLS = CI * K * K;                         // 243 filter elements per output channel: the MFMA columns, (ci, ky, kx) row-major
constexpr int TILES = (COLS + 15) / 16;                  // 16 column tiles, 4 per wave; the last one has 13 dead columns
constexpr int BLOCK = CO * COLS;                         // values of a workgroup's partial filter block, in PyTorch order (8,3,1,9,9)
constexpr int FLUSH_UNITS = 32;                          // units a workgroup's fp32 accumulators sum before they are flushed: 16 384 pixels
constexpr int DEFAULT_WGS = 512;                         // workgroups of a launch (two per CU: the split-bf16 image takes 72 KB of LDS)
}  // namespace stemw

// dW[co][ci][0][ky][kx] = sum over (b, n, y, x) of g[b, n, y, x, co] * x[b, ci, n, y + 2 ky - 8, x + 2 kx - 8]   (zero outside the image)
struct StemWgradArgs {
    const uint16_t *g;   // activation records (B, N, H, W, 8): [pixel][part][channel]
    const float *x;      // fp32 planes (B, 3, N, H, W)
    double *partial;     // [grid.x][8][243]: every workgroup's partial filter block
    int B, N, H, W;
    int tiles_y, tiles_x, total_units;
    int flush_units;     // 1 .. FLUSH_UNITS
};

const char *stem_wgrad_kernel_name(int prec);              // nullptr: no such precision
unsigned stem_wgrad_grid_x(const StemWgradArgs &a, int wgs);   // persistent grid of a launch that wants `wgs` workgroups (0: the default)
// stem_wgrad_kernel on the persistent grid, then stem_wgrad_finish_kernel: dw receives (8, 3, 1, 9, 9) fp32
hipError_t launch_stem_wgrad(int prec, const StemWgradArgs &a, unsigned grid_x, float *dw, hipStream_t s);

// dffw_grad.cpp: DFFW_OK, or the error with its message set
int stem_backward_check(int precision, int B, int N, int H, int W);

}  // namespace dffw
