// Train-mode BatchNorm3d and the gradient mask-and-add (§15): the C ABI of the kernels of dffw_bn.hip.  The record forms enqueue on the caller's stream into the caller's
// workspace; the op forms (dffw_ops.cpp) convert fp32 NCDHW tensors with the from_ncdhw / to_ncdhw kernels around them.
#include <string>

#include "dffw_bn.h"
#include "dffw_run.h"

using namespace dffw;

namespace {

// everything that is decided before a launch; M comes back through *Mout
int check_shape(int precision, int B, int C, int N, int H, int W, int *Mout) {
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (C != 8 && C != 16 && C != 32 && C != 64 && C != 128) return fail(DFFW_EINVAL, "train-mode BatchNorm serves 8, 16, 32, 64 or 128 channels, got %d", C);
    const int64_t M = (int64_t)B * N * H * W;
    if (M >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: %lld pixels do not fit 31 bits", (long long)M);
    if (M == 1) return fail(DFFW_EINVAL, "train-mode BatchNorm needs more than one value per channel (B*N*H*W == 1)");
    *Mout = (int)M;
    return DFFW_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int64_t workspace_bytes(int M, int C, const Switches &sw) { return (int64_t)bn_grid(M, sw.bn_wgs) * 2 * C * (int64_t)sizeof(double); }

BnArgs base_args(const void *x, int C, int M, void *workspace) {
    BnArgs a;
    memset(&a, 0, sizeof a);
    a.x = (const uint16_t *)x;
    a.partial = (double *)workspace;
    a.C = C;
    a.M = M;
    a.total_units = (int)(((int64_t)M + bn::UNIT_PIX - 1) / bn::UNIT_PIX);
    return a;
}

}  // namespace

int dffw::bn_train_check(int precision, int B, int C, int N, int H, int W) {
    int M;
    return check_shape(precision, B, C, N, H, W, &M);
}

extern "C" {

int64_t dffw_bn_train_workspace_bytes(int B, int C, int N, int H, int W) {
    int M;
    if (check_shape(0, B, C, N, H, W, &M)) return 0;
    return workspace_bytes(M, C, Switches::read());
}

int dffw_bn_train_forward(int device, int precision, const void *x, int B, int C, int N, int H, int W, const float *gamma, const float *beta, double eps,
                          double momentum, float *running_mean, float *running_var, const void *res, int relu, void *y, float *save_mean,
                          float *save_invstd, void *workspace, int64_t workspace_bytes_given, void *hip_stream) {
    dffw_set_last_op_kernels("");
    int M;
    if (int rc = check_shape(precision, B, C, N, H, W, &M)) return rc;
    if (!(eps > 0.0)) return fail(DFFW_EINVAL, "eps must be positive, got %g", eps);
    if (!x || !gamma || !beta || !save_mean || !save_invstd || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!y && (relu || res)) return fail(DFFW_EINVAL, "y may be NULL (statistics only) without ReLU and residual");
    if (!aligned16(x) || !aligned16(y) || !aligned16(res) || ((uintptr_t)workspace & 7)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    const Switches sw = Switches::read();
    const int64_t need = workspace_bytes(M, C, sw);
    if (workspace_bytes_given < need) return fail(DFFW_ENOMEM, "BatchNorm workspace too small (%lld < %lld bytes)", (long long)workspace_bytes_given, (long long)need);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    BnArgs a = base_args(x, C, M, workspace);
    HIPCHK(launch_bn_stats(precision, a, sw.bn_wgs, eps, momentum, running_mean, running_var, save_mean, save_invstd, s));
    std::string names = std::string(bn_stats_kernel_name(precision)) + ";dffw::bn_stats_finish_kernel";
    if (y) {
        a.in2 = (const uint16_t *)res;
        a.out = (uint16_t *)y;
        a.gamma = gamma;
        a.beta = beta;
        a.mean = save_mean;
        a.invstd = save_invstd;
        HIPCHK(launch_bn_apply(precision, relu, res != nullptr, a, sw.bn_wgs, s));
        names += std::string(";") + bn_apply_kernel_name(precision, relu, res != nullptr);
    }
    dffw_set_last_op_kernels(names.c_str());
    return DFFW_OK;
}

int dffw_bn_train_backward(int device, int precision, const void *x, const void *y, const void *grad_y, int B, int C, int N, int H, int W,
                           const float *gamma, const float *save_mean, const float *save_invstd, int relu, void *grad_x, void *grad_res,
                           float *grad_gamma, float *grad_beta, void *workspace, int64_t workspace_bytes_given, void *hip_stream) {
    dffw_set_last_op_kernels("");
    int M;
    if (int rc = check_shape(precision, B, C, N, H, W, &M)) return rc;
    if (!x || !grad_y || !gamma || !save_mean || !save_invstd || !grad_gamma || !grad_beta || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (relu && !y) return fail(DFFW_EINVAL, "the ReLU mask is read from y: y may be NULL only without ReLU");
    if (grad_res && !grad_x) return fail(DFFW_EINVAL, "grad_res is written with grad_x");
    if (!aligned16(x) || !aligned16(y) || !aligned16(grad_y) || !aligned16(grad_x) || !aligned16(grad_res) || ((uintptr_t)workspace & 7))
        return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    const Switches sw = Switches::read();
    const int64_t need = workspace_bytes(M, C, sw);
    if (workspace_bytes_given < need) return fail(DFFW_ENOMEM, "BatchNorm workspace too small (%lld < %lld bytes)", (long long)workspace_bytes_given, (long long)need);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    BnArgs a = base_args(x, C, M, workspace);
    a.y = relu ? (const uint16_t *)y : nullptr;
    a.in2 = (const uint16_t *)grad_y;
    a.mean = save_mean;
    a.invstd = save_invstd;
    HIPCHK(launch_bn_bwd_reduce(precision, relu, a, sw.bn_wgs, grad_gamma, grad_beta, s));
    std::string names = std::string(bn_bwd_reduce_kernel_name(precision, relu)) + ";dffw::bn_bwd_finish_kernel";
    if (grad_x) {
        a.out = (uint16_t *)grad_x;
        a.out2 = (uint16_t *)grad_res;
        a.gamma = gamma;
        a.dgamma = grad_gamma;
        a.dbeta = grad_beta;
        HIPCHK(launch_bn_bwd_apply(precision, relu, grad_res != nullptr, a, sw.bn_wgs, s));
        names += std::string(";") + bn_bwd_apply_kernel_name(precision, relu, grad_res != nullptr);
    }
    dffw_set_last_op_kernels(names.c_str());
    return DFFW_OK;
}

int dffw_grad_combine(int device, int precision, const void *a, const void *y, const void *b, int B, int C, int N, int H, int W, void *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (C < 8 || C % 8 || C > 128) return fail(DFFW_EINVAL, "grad_combine needs a multiple of 8 channels up to 128, got %d", C);
    const int64_t M = (int64_t)B * N * H * W;
    if (M >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: %lld pixels do not fit 31 bits", (long long)M);
    if (!a || !out) return fail(DFFW_EINVAL, "null argument");
    if (!y && !b) return fail(DFFW_EINVAL, "grad_combine without a mask (y) and without a second gradient (b) is a copy: not an operation");
    if (!aligned16(a) || !aligned16(y) || !aligned16(b) || !aligned16(out)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    HIPCHK(hipSetDevice(device));
    CombineArgs c;
    c.a = (const uint16_t *)a;
    c.y = (const uint16_t *)y;
    c.b = (const uint16_t *)b;
    c.out = (uint16_t *)out;
    c.C = C;
    c.M = (int)M;
    c.total_units = (int)((M + bn::UNIT_PIX - 1) / bn::UNIT_PIX);
    HIPCHK(launch_grad_combine(precision, c, Switches::read().bn_wgs, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels(grad_combine_kernel_name(precision, y != nullptr, b != nullptr));
    return DFFW_OK;
}

}  // extern "C"
