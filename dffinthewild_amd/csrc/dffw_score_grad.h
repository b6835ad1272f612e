// Backward of the score convs, Cin -> 1: the launch contract between dffw_score_grad.hip (kernels) and dffw_grad.cpp (C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

namespace score {
constexpr int TY = 8, TX = 8;        // k333: a unit is a TY x TX tile of one slice of one sample
constexpr int TILE_PIX = TY * TX;
constexpr int HALO = 3 * (TY + 2) * (TX + 2);   // the tile's halo of g: 3 slices x (TY + 2) x (TX + 2) fp32
constexpr int MAX_C = 128;
constexpr int DEFAULT_WGS = 512;     // workgroups of a launch (two per CU); DFFW_SCORE_WGS overrides
}  // namespace score

// One argument block for the four kernels; every launch reads the fields of its own role (the others are null).
// Records are [pixel][part][channel], C a multiple of 8 from 8 to 128; M = B*N*H*W pixels < 2^31; g is fp32 planar (B,N,H,W).
struct ScoreArgs {
    const uint16_t *x;       // wgrad: the conv's input, as the forward stored it
    const float *g;          // the score gradient
    const float *w;          // dgrad: the filter (1,C,kd,kh,kw), i.e. [c][tap]
    const uint16_t *b;       // dgrad: a second gradient of the input (null: none)
    uint16_t *out;           // dgrad: grad_x; may alias b
    double *partial;         // wgrad: [workgroup][tap][C], the workgroups' float64 sums
    int C, M, total_units;   // units: bn::UNIT_PIX pixels (k111), tiles (k333)
    int N, H, W, tiles_y, tiles_x;   // k333
};

const char *score_dgrad_kernel_name(int prec, int k, int add);   // k = 1 (k111) or 3 (k333)
const char *score_wgrad_kernel_name(int prec, int k);

int score_units(int k, int B, int N, int H, int W);              // units of a launch over the volume
unsigned score_grid(int total_units, int wgs);                   // its persistent grid when `wgs` workgroups are wanted (0: the default)
hipError_t launch_score_dgrad(int prec, int k, const ScoreArgs &a, int wgs, hipStream_t s);
// score_wgrad_kernel + score_wgrad_finish_kernel: grad_w (1,C,k,k,k) fp32
hipError_t launch_score_wgrad(int prec, int k, const ScoreArgs &a, int wgs, float *grad_w, hipStream_t s);

// dffw_grad.cpp: is this a score conv the backward serves?  DFFW_OK, or the error with its message set
int score_conv_backward_check(int precision, int B, int Cin, int N, int H, int W, const int kernel[3], const int pad[3]);

}  // namespace dffw
