// Backward of the pools on activation records: the launch contract between dffw_pool_grad.hip (kernels) and
// dffw_pool_grad.cpp (C ABI).  Records are [pixel][part][channel], C a multiple of 8 up to 128; H and W are those of the pools' INPUT
// (the volume the gradient is written at), M = B*N*H*W < 2^31.  Units are those of dffw_bn.h: bn::UNIT_PIX input pixels each, on bn_grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

constexpr int POOL_MAX = 0, POOL_AVG = 1;   // the modes of dffw_op_pool

// out = adjoint of the (1,k,k) pool at g (+ b).  max (k = 2): g goes to the first maximum of the STORED x in row-major window order
struct PoolGradArgs {
    const uint16_t *g;       // gradient of the pool's output, (B,N,H/k,W/k)
    const uint16_t *x;       // max: the stored input of the forward, (B,N,H,W); null for avg
    const uint16_t *b;       // a second gradient of the input, (B,N,H,W), or null
    uint16_t *out;           // (B,N,H,W); may alias b
    int C, W, M, total_units;
};
const char *pool_bwd_kernel_name(int prec, int mode, int k, int add);   // nullptr where no instantiation serves (mode, k)
hipError_t launch_pool_bwd(int prec, int mode, int k, const PoolGradArgs &a, int wgs, hipStream_t s);

// out = ((g8 / 64 + g4 / 16) + g2 / 4) (+ b): the adjoint of pool3_kernel in one pass; H and W multiples of 8
struct Pool3GradArgs {
    const uint16_t *g2, *g4, *g8;   // (B,N,H/2,W/2), (B,N,H/4,W/4), (B,N,H/8,W/8)
    const uint16_t *b;              // (B,N,H,W) or null
    uint16_t *out;                  // (B,N,H,W); may alias b
    int C, W, M, total_units;
};
const char *pool3_bwd_kernel_name(int prec, int add);
hipError_t launch_pool3_bwd(int prec, const Pool3GradArgs &a, int wgs, hipStream_t s);

// dffw_pool_grad.cpp: does the pool backward serve these arguments?  DFFW_OK, or DFFW_EINVAL with its message set; nothing touches the GPU
int pool_backward_check(int precision, int mode, int k, bool has_x, int B, int C, int N, int H, int W);
int pool3_backward_check(int precision, int B, int C, int N, int H, int W);

}  // namespace dffw
