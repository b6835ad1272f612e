// Backward of the convs without in-plane taps, 3x1x1 pad (1,0,0) and 1x1x1: the C ABI of the weight-gradient kernels of
// dffw_conv_pw_wgrad.hip.  As in §13 the data gradient is no kernel of its own: it is the adjoint conv through the forward's dispatch
// (dffw_op_conv_pw_backward, dffw_ops.cpp: dffw_op_conv3d -> pack_conv -> Run::conv).
#include "dffw_conv_pw_wgrad.h"
#include "dffw_run.h"

using namespace dffw;

namespace {

// 3 (k311), 1 (k111), or 0 with the error message set
int taps_of(const int kernel[3], const int pad[3]) {
    if (!kernel || !pad) {
        fail(DFFW_EINVAL, "null argument");
        return 0;
    }
    const bool flat = kernel[1] == 1 && kernel[2] == 1 && pad[1] == 0 && pad[2] == 0;
    if (flat && kernel[0] == 3 && pad[0] == 1) return 3;
    if (flat && kernel[0] == 1 && pad[0] == 0) return 1;
    fail(DFFW_EINVAL, "the pointwise conv backward serves 3x1x1 p(1,0,0) and 1x1x1 p0, stride 1; got k(%d,%d,%d) p(%d,%d,%d)", kernel[0], kernel[1], kernel[2],
         pad[0], pad[1], pad[2]);
    return 0;
}

int check_shape(int precision, int B, int Cin, int N, int H, int W, int Cout) {
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8 || Cin > 128 || Cout > 128)
        return fail(DFFW_EINVAL, "conv backward needs Cin and Cout multiples of 8 up to 128, got %d -> %d", Cin, Cout);
    const int64_t chunks = ((int64_t)H * W + pwgrad::P - 1) / pwgrad::P;
    if ((int64_t)H * W >= (1ll << 31) - pwgrad::P || B * chunks >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: the unit count does not fit 31 bits");
    return DFFW_OK;
}

struct PwgradPlan {
    PwgradArgs a;
    unsigned grid_x;
    int64_t bytes;
};

PwgradPlan plan_pwgrad(int kd, const void *x, int B, int Cin, int N, int H, int W, const void *gy, int Cout, const Switches &sw) {
    PwgradPlan p;
    memset(&p, 0, sizeof p);
    PwgradArgs &a = p.a;
    a.g = (const uint16_t *)gy;
    a.f = (const uint16_t *)x;
    a.B = B;
    a.N = N;
    a.HW = H * W;
    a.Cg = Cout;
    a.Cf = Cin;
    a.chunks = (a.HW + pwgrad::P - 1) / pwgrad::P;
    a.total_units = B * a.chunks;
    a.ncot = (a.Cg + pwgrad::CO_T - 1) / pwgrad::CO_T;
    a.ncig = (a.Cf + pwgrad::CI_G - 1) / pwgrad::CI_G;
    a.flush_steps = std::min(sw.pwgrad_flush_steps, pwgrad::FLUSH_STEPS);
    p.grid_x = conv_pw_wgrad_grid_x(a, sw.pwgrad_wgs);
    p.bytes = (int64_t)p.grid_x * a.ncot * a.ncig * 4 * pwgrad::block(kd) * (int64_t)sizeof(double);
    return p;
}

}  // namespace

int dffw::conv_pw_backward_check(int precision, int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int pad[3]) {
    return taps_of(kernel, pad) ? check_shape(precision, B, Cin, N, H, W, Cout) : DFFW_EINVAL;
}

extern "C" {

int64_t dffw_conv_pw_wgrad_workspace_bytes(int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int pad[3]) {
    const int kd = taps_of(kernel, pad);
    if (!kd || check_shape(0, B, Cin, N, H, W, Cout)) return 0;
    return plan_pwgrad(kd, nullptr, B, Cin, N, H, W, nullptr, Cout, Switches::read()).bytes;
}

int dffw_conv_pw_wgrad(int device, int precision, const void *x, int B, int Cin, int N, int H, int W, const void *grad_y, int Cout, const int kernel[3],
                       const int pad[3], float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    const int kd = taps_of(kernel, pad);
    if (!kd) return DFFW_EINVAL;
    if (int rc = check_shape(precision, B, Cin, N, H, W, Cout)) return rc;
    if (!x || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (((uintptr_t)x & 15) || ((uintptr_t)grad_y & 15) || ((uintptr_t)workspace & 7)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    const PwgradPlan p = plan_pwgrad(kd, x, B, Cin, N, H, W, grad_y, Cout, Switches::read());
    if (workspace_bytes < p.bytes) return fail(DFFW_ENOMEM, "wgrad workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)p.bytes);
    HIPCHK(hipSetDevice(device));
    PwgradArgs a = p.a;
    a.partial = (double *)workspace;
    HIPCHK(launch_conv_pw_wgrad(precision, kd, a, p.grid_x, grad_w, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels((std::string(conv_pw_wgrad_kernel_name(precision, kd)) + ";dffw::conv_pw_wgrad_finish_kernel").c_str());
    return DFFW_OK;
}

}  // extern "C"
