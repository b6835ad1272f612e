// Backward of the attention tail y = x + relu(conv111(relu(conv311(x)))) as one kernel: the launch contract between
// dffw_att_grad.hip (kernels) and dffw_grad.cpp (C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

namespace attgrad {
constexpr int P = 128;              // a unit: a column of P consecutive flat pixels of one sample's H*W plane (the plane's last chunk ragged), all N slices
constexpr int WAVE_PIX = 32;        // ... of which each of the 4 waves owns 32 in every phase of a step (two 16-pixel MFMA tiles, one 32-deep contraction)
constexpr int FLUSH_STEPS = 512;    // steps (slices of a column: 32 pixels per accumulator) between two flushes into float64: 16 384 pixels
constexpr int DEFAULT_WGS = 512;    // workgroups of a launch (two per CU)
constexpr int block(int C) { return 4 * C * C; }   // values of one workgroup's partial block: [dW3 kz = 0, 1, 2 | dW1][co][ci]
}  // namespace attgrad

// gt = [t > 0] gy;  ga = [a > 0] W1^T gt;  gx = gy + sum_kz W3[kz]^T ga[n - kz + 1];  dW1 = sum gt a;  dW3[kz] = sum ga x[n + kz - 1]
struct AttGradArgs {
    const uint16_t *x, *a, *t, *gy;   // activation records (B, N, HW, C)
    uint16_t *gx;                     // records (B, N, HW, C), may alias gy; null: no data gradient
    const float *w3, *w1;             // device fp32 (C, C, 3, 1, 1) and (C, C, 1, 1, 1); w3 is read only with gx
    double *partial;                  // [grid.x][4][C][C]: every workgroup's partial block; null: no weight gradients
    int B, N, HW;
    int chunks, total_units;          // chunks of P pixels per plane; units = B * chunks
    int flush_steps;                  // 1 .. FLUSH_STEPS
};

const char *att_tail_bwd_kernel_name(int prec, int C);   // nullptr: no such instantiation (C is 8, 16 or 32)
unsigned att_tail_bwd_grid_x(const AttGradArgs &a, int wgs);   // persistent grid of a launch that wants `wgs` workgroups (0: the default)
// att_tail_bwd_kernel on the persistent grid, then (with a.partial) att_tail_bwd_finish_kernel: dw3 (C, C, 3, 1, 1) and dw1 (C, C, 1, 1, 1) fp32
hipError_t launch_att_tail_bwd(int prec, int C, const AttGradArgs &a, unsigned grid_x, float *dw3, float *dw1, hipStream_t s);

// dffw_grad.cpp: does the family serve this shape?  DFFW_OK, or the error with its message set
int att_tail_backward_check(int precision, int B, int C, int N, int H, int W);

}  // namespace dffw
