// Backward of the score convs, Cin -> 1: the C ABI of the kernels of dffw_score_grad.hip.  The record forms enqueue their launches
// on the caller's stream and allocate nothing; the op form (dffw_ops.cpp) converts fp32 NCDHW tensors around them.
#include "dffw_score_grad.h"
#include "dffw_run.h"

using namespace dffw;

namespace {

// 3 (k333), 1 (k111), or 0 with the error message set
int kernel_of(const int kernel[3], const int pad[3]) {
    if (!kernel || !pad) {
        fail(DFFW_EINVAL, "null argument");
        return 0;
    }
    const bool cube = kernel[0] == kernel[1] && kernel[1] == kernel[2] && pad[0] == pad[1] && pad[1] == pad[2];
    if (cube && kernel[0] == 3 && pad[0] == 1) return 3;
    if (cube && kernel[0] == 1 && pad[0] == 0) return 1;
    fail(DFFW_EINVAL, "the score conv backward serves 1x1x1 p0 and 3x3x3 p(1,1,1), one output channel, stride 1; got k(%d,%d,%d) p(%d,%d,%d)", kernel[0],
         kernel[1], kernel[2], pad[0], pad[1], pad[2]);
    return 0;
}

int check_shape(int precision, int B, int Cin, int N, int H, int W) {
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d h=%d w=%d", B, N, H, W);
    if (Cin < 8 || Cin % 8 || Cin > score::MAX_C) return fail(DFFW_EINVAL, "the score conv backward needs Cin a multiple of 8 up to 128, got %d", Cin);
    const int64_t M = (int64_t)B * N * H * W;
    if (M >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: %lld pixels do not fit 31 bits", (long long)M);
    return DFFW_OK;
}

bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

ScoreArgs args_of(int k, int B, int Cin, int N, int H, int W) {
    ScoreArgs a;
    memset(&a, 0, sizeof a);
    a.C = Cin;
    a.M = (int)((int64_t)B * N * H * W);
    a.N = N;
    a.H = H;
    a.W = W;
    a.tiles_y = (H + score::TY - 1) / score::TY;
    a.tiles_x = (W + score::TX - 1) / score::TX;
    a.total_units = score_units(k, B, N, H, W);
    return a;
}

int64_t workspace_bytes(int k, const ScoreArgs &a, const Switches &sw) {
    return (int64_t)score_grid(a.total_units, sw.score_wgs) * a.C * (k * k * k) * (int64_t)sizeof(double);
}

}  // namespace

int dffw::score_conv_backward_check(int precision, int B, int Cin, int N, int H, int W, const int kernel[3], const int pad[3]) {
    return kernel_of(kernel, pad) ? check_shape(precision, B, Cin, N, H, W) : DFFW_EINVAL;
}

extern "C" {

int dffw_score_conv_dgrad(int device, int precision, const float *grad_score, int B, int Cin, int N, int h, int w, const float *weight, const int kernel[3],
                          const int pad[3], const void *b, void *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    const int k = kernel_of(kernel, pad);
    if (!k) return DFFW_EINVAL;
    if (int rc = check_shape(precision, B, Cin, N, h, w)) return rc;
    if (!grad_score || !weight || !out) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(b, 16) || !aligned(out, 16)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    if (!aligned(grad_score, 4) || !aligned(weight, 4)) return fail(DFFW_EINVAL, "grad_score and weight must be 4-byte aligned");
    HIPCHK(hipSetDevice(device));
    ScoreArgs a = args_of(k, B, Cin, N, h, w);
    a.g = grad_score;
    a.w = weight;
    a.b = (const uint16_t *)b;
    a.out = (uint16_t *)out;
    HIPCHK(launch_score_dgrad(precision, k, a, Switches::read().score_wgs, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels(score_dgrad_kernel_name(precision, k, b != nullptr));
    return DFFW_OK;
}

int64_t dffw_score_conv_wgrad_workspace_bytes(int B, int Cin, int N, int h, int w, const int kernel[3], const int pad[3]) {
    const int k = kernel_of(kernel, pad);
    if (!k || check_shape(0, B, Cin, N, h, w)) return 0;
    return workspace_bytes(k, args_of(k, B, Cin, N, h, w), Switches::read());
}

int dffw_score_conv_wgrad(int device, int precision, const void *x, const float *grad_score, int B, int Cin, int N, int h, int w, const int kernel[3],
                          const int pad[3], float *grad_w, void *workspace, int64_t workspace_bytes_given, void *hip_stream) {
    dffw_set_last_op_kernels("");
    const int k = kernel_of(kernel, pad);
    if (!k) return DFFW_EINVAL;
    if (int rc = check_shape(precision, B, Cin, N, h, w)) return rc;
    if (!x || !grad_score || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(x, 16)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    if (!aligned(grad_score, 4) || !aligned(grad_w, 4) || !aligned(workspace, 8))
        return fail(DFFW_EINVAL, "grad_score and grad_w must be 4-byte aligned, the workspace 8-byte aligned");
    const Switches sw = Switches::read();
    ScoreArgs a = args_of(k, B, Cin, N, h, w);
    const int64_t need = workspace_bytes(k, a, sw);
    if (workspace_bytes_given < need)
        return fail(DFFW_ENOMEM, "score wgrad workspace too small (%lld < %lld bytes)", (long long)workspace_bytes_given, (long long)need);
    HIPCHK(hipSetDevice(device));
    a.x = (const uint16_t *)x;
    a.g = grad_score;
    a.partial = (double *)workspace;
    HIPCHK(launch_score_wgrad(precision, k, a, sw.score_wgs, grad_w, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels((std::string(score_wgrad_kernel_name(precision, k)) + ";dffw::score_wgrad_finish_kernel").c_str());
    return DFFW_OK;
}

}  // extern "C"
