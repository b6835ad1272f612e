// Weight gradient of the convs without in-plane taps, 3x1x1 and 1x1x1: the launch contract between dffw_conv_pw_wgrad.hip
// (kernels) and dffw_grad.cpp (C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

namespace pwgrad {
constexpr int P = 128;              // a unit: a column of P consecutive flat pixels of one sample's H*W plane (the plane's last chunk ragged), all N slices
constexpr int WAVE_PIX = 32;        // ... of which each of the 4 waves contracts 32 per step (one 32-deep MFMA chunk)
constexpr int CO_T = 16;            // channels of g (grad_y) of a workgroup (one MFMA row tile)
constexpr int CI_G = 32;            // channels of f (x) of a workgroup (two MFMA column tiles)
constexpr int FLUSH_STEPS = 512;    // steps (slices of a column: 32 pixels per accumulator) between two flushes into float64: 16 384 pixels
constexpr int DEFAULT_WGS = 512;    // workgroups of a launch over grid.x * grid.y (two per CU)
constexpr int block(int kd) { return CO_T * CI_G * kd; }   // values of one wave's partial filter block
}  // namespace pwgrad

// dW[co][ci][kz] = sum over (b, n, p) of g[b, n, p, co] * f[b, n + kz - pz, p, ci]     p: flat pixel of the plane, zero outside 0 <= n + kz - pz < N
struct PwgradArgs {
    const uint16_t *g;   // activation records (B, N, HW, Cg): grad_y
    const uint16_t *f;   // activation records (B, N, HW, Cf): x
    double *partial;     // [grid.y][grid.x][wave][CO_T][CI_G][kd]: every wave's partial filter block
    int B, N, HW, Cg, Cf;
    int chunks, total_units;   // chunks of P pixels per plane; units = B * chunks
    int ncot, ncig;      // grid.y = ncot * ncig: CO_T-channel tile of g x CI_G-channel group of f
    int flush_steps;     // 1 .. FLUSH_STEPS
};

const char *conv_pw_wgrad_kernel_name(int prec, int kd);   // nullptr: no such instantiation (kd is 1 or 3)
unsigned conv_pw_wgrad_grid_x(const PwgradArgs &a, int wgs);   // persistent grid of a launch that wants `wgs` workgroups in all (0: the default)
// conv_pw_wgrad_kernel on the persistent grid, then conv_pw_wgrad_finish_kernel: dw receives (Cg, Cf, kd, 1, 1) fp32
hipError_t launch_conv_pw_wgrad(int prec, int kd, const PwgradArgs &a, unsigned grid_x, float *dw, hipStream_t s);

// dffw_grad.cpp: is this k311 / k111 on a shape the family serves?  DFFW_OK, or the error with its message set
int conv_pw_backward_check(int precision, int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int pad[3]);

}  // namespace dffw
