// Backward of the pools on activation records: the C ABI of the kernels of dffw_pool_grad.hip.  The record forms enqueue one
// launch on the caller's stream and allocate nothing; the op forms (dffw_ops.cpp) convert fp32 NCDHW tensors around them.
#include "dffw_bn.h"
#include "dffw_pool_grad.h"
#include "dffw_run.h"

using namespace dffw;

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int units_of(int64_t M) { return (int)((M + bn::UNIT_PIX - 1) / bn::UNIT_PIX); }

}  // namespace

int dffw::pool_backward_check(int precision, int mode, int k, bool has_x, int B, int C, int N, int H, int W) {
    if (mode != POOL_MAX && mode != POOL_AVG) return fail(DFFW_EINVAL, "unknown pool mode %d (0 max, 1 average)", mode);
    if (mode == POOL_MAX && k != 2) return fail(DFFW_EINVAL, "the max pool backward serves (1,2,2) only, got k = %d", k);
    if (mode == POOL_AVG && k != 2 && k != 4 && k != 8) return fail(DFFW_EINVAL, "the average pool backward serves k = 2, 4, 8, got %d", k);
    if (int rc = check_volume("pool backward", precision, B, N, H, W, {C}, k, (int64_t)B * N * H * W, "pixels")) return rc;
    if (mode == POOL_MAX && !has_x) return fail(DFFW_EINVAL, "the max pool backward reads the argmax from x, the stored input of the forward");
    return DFFW_OK;
}

int dffw::pool3_backward_check(int precision, int B, int C, int N, int H, int W) {
    return check_volume("the pyramid backward", precision, B, N, H, W, {C}, 8, (int64_t)B * N * H * W, "pixels");   // H and W: the input resolution
}

extern "C" {

int dffw_pool_backward(int device, int precision, int mode, int k, const void *g, const void *x, const void *b, int B, int C, int N, int H, int W,
                       void *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = pool_backward_check(precision, mode, k, x != nullptr, B, C, N, H, W)) return rc;
    if (!g || !out) return fail(DFFW_EINVAL, "null argument");
    if (!aligned16(g) || !aligned16(x) || !aligned16(b) || !aligned16(out)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    HIPCHK(hipSetDevice(device));
    PoolGradArgs a;
    a.g = (const uint16_t *)g;
    a.x = mode == POOL_MAX ? (const uint16_t *)x : nullptr;
    a.b = (const uint16_t *)b;
    a.out = (uint16_t *)out;
    a.C = C;
    a.W = W;
    a.M = (int)((int64_t)B * N * H * W);
    a.total_units = units_of(a.M);
    HIPCHK(launch_pool_bwd(precision, mode, k, a, Switches::read().bn_wgs, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels(pool_bwd_kernel_name(precision, mode, k, b != nullptr));
    return DFFW_OK;
}

int dffw_pool3_backward(int device, int precision, const void *g2, const void *g4, const void *g8, const void *b, int B, int C, int N, int H, int W,
                        void *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = pool3_backward_check(precision, B, C, N, H, W)) return rc;
    if (!g2 || !g4 || !g8) return fail(DFFW_EINVAL, "the pyramid backward needs all of g2, g4 and g8");
    if (!out) return fail(DFFW_EINVAL, "null argument");
    if (!aligned16(g2) || !aligned16(g4) || !aligned16(g8) || !aligned16(b) || !aligned16(out)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    HIPCHK(hipSetDevice(device));
    Pool3GradArgs a;
    a.g2 = (const uint16_t *)g2;
    a.g4 = (const uint16_t *)g4;
    a.g8 = (const uint16_t *)g8;
    a.b = (const uint16_t *)b;
    a.out = (uint16_t *)out;
    a.C = C;
    a.W = W;
    a.M = (int)((int64_t)B * N * H * W);
    a.total_units = units_of(a.M);
    HIPCHK(launch_pool3_bwd(precision, a, Switches::read().bn_wgs, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels(pool3_bwd_kernel_name(precision, b != nullptr));
    return DFFW_OK;
}

}  // extern "C"
