// Weight gradient of the aggregation network's convs: the launch contract between dffw_conv_wgrad.hip (kernels) and dffw_grad.cpp (C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

namespace wgrad {
constexpr int TY = 4, TX = 16;      // a unit: TY x TX points of the grid-side tensor's plane (one slice of one sample) = two 32-deep MFMA chunks
constexpr int CO_T = 16;            // grid-side channels of a workgroup (one MFMA row tile)
constexpr int CI_G = 32;            // footprint-side channels of a workgroup (two MFMA column tiles)
constexpr int BLOCK = CO_T * CI_G * 9;   // values of a workgroup's partial filter block
constexpr int FLUSH_UNITS = 256;    // units (of TY * TX = 64 points) a workgroup's fp32 accumulators sum before they are flushed: 16 384 points
constexpr int DEFAULT_WGS = 512;    // workgroups of a launch over grid.x * grid.y (two per CU)
}  // namespace wgrad

// dW[co][ci][kz][ky][kx] = sum over (b, n, y, x) of g[b, n, y, x, co] * f[b, n + kz - pz, S*y + ky - 1, S*x + kx - 1, ci]   (zero outside f)
// g is the tensor on the conv's output grid (dy of a conv; x of the transposed conv), f the one its footprints lie in (x of a conv; dy of the transposed conv).
struct WgradArgs {
    const uint16_t *g;   // activation records (B, N, Hg, Wg, Cg)
    const uint16_t *f;   // activation records (B, N, S*Hg, S*Wg, Cf)
    double *partial;     // [grid.y][grid.x][CO_T][CI_G][9]: every workgroup's partial filter block
    int B, N, Hg, Wg, Cg, Cf;
    int kd, pz;          // slice taps (3 or 1) and slice padding (1 or 0)
    int tiles_y, tiles_x, total_tiles;
    int ncot, ncig;      // grid.y = kd * ncot * ncig: slice tap x CO_T-channel tile of g x CI_G-channel group of f
    int flush_units;     // 1 .. FLUSH_UNITS
};

// The same sum for the 3x3x3 stride-1 pad-1 conv whose input is the channel concatenation of two tensors of one volume: f is
// never materialised, footprint channel ci is f_a's channel ci below Ca and f_b's channel ci - Ca from there.  kd = 3, pz = 1, S = 1.
struct WgradCatArgs {
    const uint16_t *g;     // activation records (B, N, Hg, Wg, Cg): grad_y
    const uint16_t *f_a;   // activation records (B, N, Hg, Wg, Ca): the first source
    const uint16_t *f_b;   // activation records (B, N, Hg, Wg, Cb): the second source
    double *partial;       // [grid.y][grid.x][CO_T][CI_G][9], as WgradArgs::partial
    int B, N, Hg, Wg, Cg, Ca, Cb;
    int tiles_y, tiles_x, total_tiles;
    int ncot, ncig;        // grid.y = 3 * ncot * ncig; the CI_G-channel groups run over the Ca + Cb channels of the concatenation
    int flush_units;       // 1 .. FLUSH_UNITS
};

// rows of the family's table (nullptr: no such instantiation); `stride` is the in-plane stride S, 1 or 2
const char *conv_wgrad_kernel_name(int prec, int stride);
unsigned conv_wgrad_grid_x(const WgradArgs &a, int wgs);   // persistent grid of a launch that wants `wgs` workgroups in all (0: the default)
// conv_wgrad_kernel on the persistent grid, then conv_wgrad_finish: dw receives (Cg, Cf, kd, 3, 3) fp32
hipError_t launch_conv_wgrad(int prec, int stride, const WgradArgs &a, unsigned grid_x, float *dw, hipStream_t s);
// ... and of conv_wgrad_cat_kernel (one row per precision): dw receives (Cg, Ca + Cb, 3, 3, 3) fp32
const char *conv_wgrad_cat_kernel_name(int prec);
unsigned conv_wgrad_cat_grid_x(const WgradCatArgs &a, int wgs);
hipError_t launch_conv_wgrad_cat(int prec, const WgradCatArgs &a, unsigned grid_x, float *dw, hipStream_t s);

// dffw_grad.cpp: is this one of the four geometries conv backward serves, on a shape it serves?  DFFW_OK, or the error with its message set
int conv_backward_check(int precision, int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int stride[3], const int pad[3],
                        int transposed);
// ... and of the conv over a concatenation: its one geometry is in its name, so these are the shape's refusals
int conv_cat_backward_check(int precision, int B, int Ca, int Cb, int N, int H, int W, int Cout);

}  // namespace dffw
