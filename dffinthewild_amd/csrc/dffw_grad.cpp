// Backward of the aggregation network's plain convs: the C ABI of the weight-gradient kernels (dffw_conv_wgrad.hip).  The data
// gradient is no kernel of its own: it is the adjoint conv, packed by pack_conv under a layer definition of the adjoint geometry and run through the
// forward's own dispatch (dffw_op_conv3d_backward, dffw_ops.cpp: dffw_op_conv3d -> Run::conv).
#include "dffw_conv_wgrad.h"
#include "dffw_run.h"

using namespace dffw;

namespace {

enum Geometry { G_NONE, G_K333_S1, G_K133_S1, G_K333_S2, G_K333_T };

// one of the four geometries, or G_NONE with the error message set
Geometry geometry_of(const int kernel[3], const int stride[3], const int pad[3], int transposed) {
    if (!kernel || !stride || !pad) {
        fail(DFFW_EINVAL, "null argument");
        return G_NONE;
    }
    const bool k333 = kernel[0] == 3 && kernel[1] == 3 && kernel[2] == 3, k133 = kernel[0] == 1 && kernel[1] == 3 && kernel[2] == 3;
    const bool s1 = stride[0] == 1 && stride[1] == 1 && stride[2] == 1, s2 = stride[0] == 1 && stride[1] == 2 && stride[2] == 2;
    const bool p1 = pad[0] == 1 && pad[1] == 1 && pad[2] == 1, p0 = pad[0] == 0 && pad[1] == 1 && pad[2] == 1;
    Geometry g = G_NONE;
    if (transposed) g = k333 && s2 && p1 ? G_K333_T : G_NONE;
    else if (k333 && p1) g = s1 ? G_K333_S1 : s2 ? G_K333_S2 : G_NONE;
    else if (k133 && p0 && s1) g = G_K133_S1;
    if (g == G_NONE)
        fail(DFFW_EINVAL, "conv backward serves 3x3x3 p1 stride 1 or (1,2,2), 1x3x3 p(0,1,1) stride 1 and the transposed 3x3x3 s(1,2,2) p1 op(0,1,1); got k(%d,%d,%d) s(%d,%d,%d) p(%d,%d,%d)%s",
             kernel[0], kernel[1], kernel[2], stride[0], stride[1], stride[2], pad[0], pad[1], pad[2], transposed ? " transposed" : "");
    return g;
}

int check_shape(Geometry g, int precision, int B, int Cin, int N, int H, int W, int Cout) {
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8 || Cin > 128 || Cout > 128)
        return fail(DFFW_EINVAL, "conv backward needs Cin and Cout multiples of 8 up to 128, got %d -> %d", Cin, Cout);
    if (g == G_K333_S2 && (H % 2 || W % 2)) return fail(DFFW_EINVAL, "stride (1,2,2): H and W must be even, got %d x %d", H, W);
    return DFFW_OK;
}

struct WgradPlan {
    WgradArgs a;
    int stride;
    unsigned grid_x;
    int64_t bytes;
};

// x (B,N,H,W,Cin) and grad_y in the conv's own roles -> the kernel's grid-side / footprint-side tensors
WgradPlan plan_wgrad(Geometry g, const void *x, int B, int Cin, int N, int H, int W, const void *gy, int Cout, const Switches &sw) {
    WgradPlan p;
    memset(&p, 0, sizeof p);
    WgradArgs &a = p.a;
    a.B = B;
    a.N = N;
    a.kd = g == G_K133_S1 ? 1 : 3;
    a.pz = g == G_K133_S1 ? 0 : 1;
    p.stride = g == G_K333_S2 || g == G_K333_T ? 2 : 1;
    if (g == G_K333_T) {   // the stride-2 kernel with the roles swapped: x is on the grid, grad_y (B,N,2H,2W,Cout) holds the footprints
        a.g = (const uint16_t *)x; a.Cg = Cin; a.Hg = H; a.Wg = W;
        a.f = (const uint16_t *)gy; a.Cf = Cout;
    } else {
        a.g = (const uint16_t *)gy; a.Cg = Cout; a.Hg = H / p.stride; a.Wg = W / p.stride;
        a.f = (const uint16_t *)x; a.Cf = Cin;
    }
    a.tiles_y = (a.Hg + wgrad::TY - 1) / wgrad::TY;
    a.tiles_x = (a.Wg + wgrad::TX - 1) / wgrad::TX;
    a.total_tiles = B * N * a.tiles_y * a.tiles_x;
    a.ncot = (a.Cg + wgrad::CO_T - 1) / wgrad::CO_T;
    a.ncig = (a.Cf + wgrad::CI_G - 1) / wgrad::CI_G;
    a.flush_units = std::min(sw.wgrad_flush_units, wgrad::FLUSH_UNITS);
    p.grid_x = conv_wgrad_grid_x(a, sw.wgrad_wgs);
    p.bytes = (int64_t)p.grid_x * a.kd * a.ncot * a.ncig * wgrad::BLOCK * (int64_t)sizeof(double);
    return p;
}

}  // namespace

int dffw::conv_backward_check(int precision, int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int stride[3], const int pad[3],
                              int transposed) {
    const Geometry g = geometry_of(kernel, stride, pad, transposed);
    return g == G_NONE ? DFFW_EINVAL : check_shape(g, precision, B, Cin, N, H, W, Cout);
}

extern "C" {

int64_t dffw_conv_wgrad_workspace_bytes(int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int stride[3], const int pad[3],
                                        int transposed) {
    const Geometry g = geometry_of(kernel, stride, pad, transposed);
    if (g == G_NONE || check_shape(g, 0, B, Cin, N, H, W, Cout)) return 0;
    if ((int64_t)B * N * ((H + 3) / 4) * ((W + 15) / 16) >= (1ll << 31)) return 0;
    return plan_wgrad(g, nullptr, B, Cin, N, H, W, nullptr, Cout, Switches::read()).bytes;
}

int dffw_conv_wgrad(int device, int precision, const void *x, int B, int Cin, int N, int H, int W, const void *grad_y, int Cout, const int kernel[3],
                    const int stride[3], const int pad[3], int transposed, float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    const Geometry g = geometry_of(kernel, stride, pad, transposed);
    if (g == G_NONE) return DFFW_EINVAL;
    if (int rc = check_shape(g, precision, B, Cin, N, H, W, Cout)) return rc;
    if (!x || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if ((int64_t)B * N * ((H + 3) / 4) * ((W + 15) / 16) >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: the unit count does not fit 31 bits");
    const WgradPlan p = plan_wgrad(g, x, B, Cin, N, H, W, grad_y, Cout, Switches::read());
    if (workspace_bytes < p.bytes) return fail(DFFW_ENOMEM, "wgrad workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)p.bytes);
    HIPCHK(hipSetDevice(device));
    WgradArgs a = p.a;
    a.partial = (double *)workspace;
    HIPCHK(launch_conv_wgrad(precision, p.stride, a, p.grid_x, grad_w, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels((std::string(conv_wgrad_kernel_name(precision, p.stride)) + ";dffw::conv_wgrad_finish_kernel").c_str());
    return DFFW_OK;
}

}  // extern "C"
