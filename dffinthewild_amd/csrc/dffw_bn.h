// Train-mode BatchNorm3d on activation records: the launch contract between dffw_bn.hip (kernels) and dffw_bn.cpp (C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

namespace bn {
constexpr int UNIT_PIX = 512;       // a unit: 512 consecutive pixels of the volume (the last one ragged)
constexpr int DEFAULT_WGS = 512;    // workgroups of a launch (two per CU); DFFW_BN_WGS overrides
}  // namespace bn

// One argument block for the four streaming kernels; every launch reads the fields of its own role (the others are null).
// Records are [pixel][part][channel], C in {8, 16, 32, 64, 128}; M = B*N*H*W pixels < 2^31.
struct BnArgs {
    const uint16_t *x;       // the normalised tensor (input of the forward)
    const uint16_t *y;       // stored output of the forward: the ReLU mask of the backward kernels (null without ReLU)
    const uint16_t *in2;     // forward apply: the residual; backward kernels: grad_y
    uint16_t *out;           // forward apply: y; backward apply: grad_x
    uint16_t *out2;          // backward apply: grad_res (null without a residual)
    const float *gamma, *beta;
    const float *mean, *invstd;          // save_mean / save_invstd (C each)
    const float *dgamma, *dbeta;         // backward apply: the finished parameter gradients
    double *partial;         // [workgroup][2][C]: the workgroups' float64 sums (stats: sum x, sum x^2; backward: sum g, sum g (x - mean))
    int C, M, total_units;
};

const char *bn_stats_kernel_name(int prec);
const char *bn_apply_kernel_name(int prec, int relu, int res);
const char *bn_bwd_reduce_kernel_name(int prec, int relu);
const char *bn_bwd_apply_kernel_name(int prec, int relu, int res);

unsigned bn_grid(int M, int wgs);   // the persistent grid of every launch over M pixels that wants `wgs` workgroups (0: the default)
// bn_stats_kernel + bn_stats_finish_kernel: save_mean, save_invstd, and running_mean / running_var in place where given
hipError_t launch_bn_stats(int prec, const BnArgs &a, int wgs, double eps, double momentum, float *running_mean, float *running_var, float *save_mean,
                           float *save_invstd, hipStream_t s);
hipError_t launch_bn_apply(int prec, int relu, int res, const BnArgs &a, int wgs, hipStream_t s);
// bn_bwd_reduce_kernel + bn_bwd_finish_kernel: grad_gamma, grad_beta
hipError_t launch_bn_bwd_reduce(int prec, int relu, const BnArgs &a, int wgs, float *grad_gamma, float *grad_beta, hipStream_t s);
hipError_t launch_bn_bwd_apply(int prec, int relu, int res, const BnArgs &a, int wgs, hipStream_t s);

// out = [y > 0] a (+ b) on records of C channels (a multiple of 8), M pixels; y or b may be null, not both
struct CombineArgs {
    const uint16_t *a, *y, *b;
    uint16_t *out;           // may alias a, y or b
    int C, M, total_units;   // units of bn::UNIT_PIX pixels
};
const char *grad_combine_kernel_name(int prec, int mask, int add);   // nullptr without mask and add
hipError_t launch_grad_combine(int prec, const CombineArgs &a, int wgs, hipStream_t s);

// dffw_bn.cpp: is (B, C, N, H, W) a volume train-mode BatchNorm serves?  DFFW_OK, or the error with its message set
int bn_train_check(int precision, int B, int C, int N, int H, int W);

}  // namespace dffw
