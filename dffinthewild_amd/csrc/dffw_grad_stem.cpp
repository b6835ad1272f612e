// Backward of the stem, Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2)) on the image stack: the C ABI of the
// weight-gradient kernels of dffw_stem_wgrad.hip.  The stem's input is the image, so there is no data gradient.
#include "dffw_run.h"
#include "dffw_stem_wgrad.h"

using namespace dffw;

namespace {

struct StemWgradPlan {
    StemWgradArgs a;
    unsigned grid_x;
    int64_t bytes;
};

StemWgradPlan plan_stem_wgrad(const float *x, const void *gy, int B, int N, int H, int W, const Switches &sw) {
    StemWgradPlan p;
    memset(&p, 0, sizeof p);
    StemWgradArgs &a = p.a;
    a.g = (const uint16_t *)gy;
    a.x = x;
    a.B = B;
    a.N = N;
    a.H = H;
    a.W = W;
    a.tiles_y = (H + stemw::TY - 1) / stemw::TY;
    a.tiles_x = (W + stemw::TX - 1) / stemw::TX;
    a.total_units = B * N * a.tiles_y * a.tiles_x;
    // DFFW_WGRAD_FLUSH_UNITS counts conv_wgrad's units of 64 pixels; a unit here is 512
    a.flush_units = std::max(1, std::min(sw.wgrad_flush_units * 64 / (stemw::TY * stemw::TX), stemw::FLUSH_UNITS));
    p.grid_x = stem_wgrad_grid_x(a, sw.wgrad_wgs);
    p.bytes = (int64_t)p.grid_x * stemw::BLOCK * (int64_t)sizeof(double);
    return p;
}

}  // namespace

int dffw::stem_backward_check(int precision, int B, int N, int H, int W) {
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if ((int64_t)B * N * H * W >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: the pixel count does not fit 31 bits");
    return DFFW_OK;
}

extern "C" {

int64_t dffw_stem_wgrad_workspace_bytes(int B, int N, int H, int W) {
    if (stem_backward_check(0, B, N, H, W)) return 0;
    return plan_stem_wgrad(nullptr, nullptr, B, N, H, W, Switches::read()).bytes;
}

int dffw_stem_wgrad(int device, int precision, const float *x, const void *grad_y, int B, int N, int H, int W, float *grad_w, void *workspace,
                    int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = stem_backward_check(precision, B, N, H, W)) return rc;
    if (!x || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (((uintptr_t)grad_y & 15) || ((uintptr_t)x & 3) || ((uintptr_t)workspace & 7)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    const StemWgradPlan p = plan_stem_wgrad(x, grad_y, B, N, H, W, Switches::read());
    if (workspace_bytes < p.bytes) return fail(DFFW_ENOMEM, "wgrad workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)p.bytes);
    HIPCHK(hipSetDevice(device));
    StemWgradArgs a = p.a;
    a.partial = (double *)workspace;
    HIPCHK(launch_stem_wgrad(precision, a, p.grid_x, grad_w, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels((std::string(stem_wgrad_kernel_name(precision)) + ";dffw::stem_wgrad_finish_kernel").c_str());
    return DFFW_OK;
}

}  // extern "C"
