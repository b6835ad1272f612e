// Backward of the convs: the C ABI of the four weight-gradient kernel families.
//   plain    3x3x3 / 1x3x3 stride 1, 3x3x3 stride (1,2,2), transposed 3x3x3   DESIGN.md §13   dffw_conv_wgrad.hip
//   cat      3x3x3 stride 1 over the concatenation of two sources             DESIGN.md §21   dffw_conv_wgrad.hip (the plain body, two-source fill)
//   pw       3x1x1 pad (1,0,0) and 1x1x1: no in-plane taps                    DESIGN.md §15   dffw_conv_pw_wgrad.hip
//   stem     Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2))             DESIGN.md §17   dffw_stem_wgrad.hip
//   score    Cin -> 1, 1x1x1 and 3x3x3 (and their data gradient)              DESIGN.md §19   dffw_score_grad.hip
//   att      the attention tail, both convs and both masks, data gradient too DESIGN.md §27   dffw_att_grad.hip
// A family owns its geometry recogniser and its plan_*(): geometry -> shape (check_volume) -> the kernel's arguments, the grid and the workspace
// size.  Its *_backward_check (for dffw_ops.cpp), its *_workspace_bytes and its record form all read that one Plan; a record form then checks its
// pointers and ends in launch_record().  Every refusal comes in the order geometry, shape, null, alignment, workspace.  The record forms enqueue
// on the caller's stream and allocate nothing.  The data gradient of the plain, pw and stem families is no kernel of its own: it is the adjoint
// conv through the forward's dispatch (dffw_ops.cpp), and the stem has none.
#include "dffw_att_grad.h"
#include "dffw_conv_pw_wgrad.h"
#include "dffw_conv_wgrad.h"
#include "dffw_run.h"
#include "dffw_score_grad.h"
#include "dffw_stem_wgrad.h"

using namespace dffw;

int dffw::check_volume(const char *family, int precision, int B, int N, int H, int W, std::initializer_list<int> channels, int div, int64_t units,
                       const char *unit) {
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    for (int c : channels)
        if (c < 8 || c % 8 || c > 128)
            return channels.size() == 2 ? fail(DFFW_EINVAL, "%s needs Cin and Cout multiples of 8 up to 128, got %d -> %d", family, channels.begin()[0], channels.begin()[1])
                                        : fail(DFFW_EINVAL, "%s needs a multiple of 8 channels up to 128, got %d", family, c);
    if (H % div || W % div) return fail(DFFW_EINVAL, "%s needs H and W divisible by %d, got %dx%d", family, div, H, W);
    if (units >= (1ll << 31)) return fail(DFFW_EINVAL, "volume too large: %lld %s do not fit 31 bits", (long long)units, unit);
    return DFFW_OK;
}

namespace {

// What a family makes of a call's geometry and shape.  With rc set (and the error message with it) nothing else is filled in
template <class Args>
struct Plan {
    int rc;
    int sub;          // the second index of the family's kernel table: in-plane stride (plain), slice taps (pw), kernel size (score)
    Args a;           // the kernel's arguments; `partial` is the record form's to set
    unsigned grid_x;
    int64_t bytes;    // the workspace of the launch
    int wgs;          // score: DFFW_SCORE_WGS as the plan read it (its launchers size the grid themselves); the switches are read once per call
};

// The end of every record form: the workspace's size, the device, kernel + finish kernel (`launch`), their names for dffw_last_op_kernels()
template <class Launch>
int launch_record(const char *what, int64_t need, int64_t given, int device, const char *kernel, const char *finish, Launch launch) {
    if (given < need) return fail(DFFW_ENOMEM, "%s workspace too small (%lld < %lld bytes)", what, (long long)given, (long long)need);
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch());
    dffw_set_last_op_kernels((std::string(kernel) + ";" + finish).c_str());
    return DFFW_OK;
}

// ---- plain ------------------------------------------------------------------------------------------------------------------------------------
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

// x (B,N,H,W,Cin) and grad_y in the conv's own roles -> the kernel's grid-side / footprint-side tensors
Plan<WgradArgs> plan_conv(int precision, const void *x, int B, int Cin, int N, int H, int W, const void *gy, int Cout, const int kernel[3],
                          const int stride[3], const int pad[3], int transposed) {
    Plan<WgradArgs> p{};
    const Geometry g = geometry_of(kernel, stride, pad, transposed);
    const bool s2 = g == G_K333_S2;
    // the limit counts the units of the input plane: no fewer than the grid-side plane has at any of the geometries
    const int64_t units = (int64_t)B * N * ((H + wgrad::TY - 1) / wgrad::TY) * ((W + wgrad::TX - 1) / wgrad::TX);
    p.rc = g == G_NONE ? DFFW_EINVAL
                       : check_volume(s2 ? "conv backward at stride (1,2,2)" : "conv backward", precision, B, N, H, W, {Cin, Cout}, s2 ? 2 : 1, units, "units");
    if (p.rc) return p;
    const Switches sw = Switches::read();
    WgradArgs &a = p.a;
    a.B = B;
    a.N = N;
    a.kd = g == G_K133_S1 ? 1 : 3;
    a.pz = g == G_K133_S1 ? 0 : 1;
    p.sub = s2 || g == G_K333_T ? 2 : 1;
    if (g == G_K333_T) {   // the stride-2 kernel with the roles swapped: x is on the grid, grad_y (B,N,2H,2W,Cout) holds the footprints
        a.g = (const uint16_t *)x; a.Cg = Cin; a.Hg = H; a.Wg = W;
        a.f = (const uint16_t *)gy; a.Cf = Cout;
    } else {
        a.g = (const uint16_t *)gy; a.Cg = Cout; a.Hg = H / p.sub; a.Wg = W / p.sub;
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

// ---- cat: the 3x3x3 stride-1 pad-1 conv whose input is the concatenation of xa (Ca channels) and xb (Cb channels) ---------------------------------
// The geometry is the entry point's name; the shape's refusals are check_volume's (Cout as a plain conv's) and then this family's own rule for
// the two sources, whose sum may pass 128: that is what the forward's two-source fill is known to serve
Plan<WgradCatArgs> plan_conv_cat(int precision, const void *xa, int Ca, const void *xb, int Cb, int B, int N, int H, int W, const void *gy, int Cout) {
    Plan<WgradCatArgs> p{};
    const int64_t units = (int64_t)B * N * ((H + wgrad::TY - 1) / wgrad::TY) * ((W + wgrad::TX - 1) / wgrad::TX);
    p.rc = check_volume("conv backward over a concatenation", precision, B, N, H, W, {Cout}, 1, units, "units");
    if (p.rc) return p;
    for (int c : {Ca, Cb})
        if (c < 8 || c % 8 || c > 128 || Ca + Cb > 192) {
            p.rc = fail(DFFW_EINVAL, "conv backward over a concatenation needs Ca and Cb multiples of 8 from 8 to 128 with Ca + Cb <= 192, got Ca=%d Cb=%d", Ca, Cb);
            return p;
        }
    const Switches sw = Switches::read();
    WgradCatArgs &a = p.a;
    a.g = (const uint16_t *)gy;
    a.f_a = (const uint16_t *)xa;
    a.f_b = (const uint16_t *)xb;
    a.B = B;
    a.N = N;
    a.Hg = H;
    a.Wg = W;
    a.Cg = Cout;
    a.Ca = Ca;
    a.Cb = Cb;
    a.tiles_y = (H + wgrad::TY - 1) / wgrad::TY;
    a.tiles_x = (W + wgrad::TX - 1) / wgrad::TX;
    a.total_tiles = B * N * a.tiles_y * a.tiles_x;
    a.ncot = (Cout + wgrad::CO_T - 1) / wgrad::CO_T;
    a.ncig = (Ca + Cb + wgrad::CI_G - 1) / wgrad::CI_G;
    a.flush_units = std::min(sw.wgrad_flush_units, wgrad::FLUSH_UNITS);
    p.grid_x = conv_wgrad_cat_grid_x(a, sw.wgrad_wgs);
    p.bytes = (int64_t)p.grid_x * 3 * a.ncot * a.ncig * wgrad::BLOCK * (int64_t)sizeof(double);
    return p;
}

// ---- pw ---------------------------------------------------------------------------------------------------------------------------------------
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

Plan<PwgradArgs> plan_pw(int precision, const void *x, int B, int Cin, int N, int H, int W, const void *gy, int Cout, const int kernel[3], const int pad[3]) {
    Plan<PwgradArgs> p{};
    p.sub = taps_of(kernel, pad);
    // two counts are ints in the kernel: the plane rounded up to whole chunks, and the units B * chunks
    const int64_t HW = (int64_t)H * W, chunks = (HW + pwgrad::P - 1) / pwgrad::P;
    p.rc = !p.sub ? DFFW_EINVAL : check_volume("conv backward", precision, B, N, H, W, {Cin, Cout}, 1, std::max(HW + pwgrad::P, B * chunks), "pixels of a plane or units");
    if (p.rc) return p;
    const Switches sw = Switches::read();
    PwgradArgs &a = p.a;
    a.g = (const uint16_t *)gy;
    a.f = (const uint16_t *)x;
    a.B = B;
    a.N = N;
    a.HW = H * W;
    a.Cg = Cout;
    a.Cf = Cin;
    a.chunks = (int)chunks;
    a.total_units = B * a.chunks;
    a.ncot = (a.Cg + pwgrad::CO_T - 1) / pwgrad::CO_T;
    a.ncig = (a.Cf + pwgrad::CI_G - 1) / pwgrad::CI_G;
    a.flush_steps = std::min(sw.pwgrad_flush_steps, pwgrad::FLUSH_STEPS);
    p.grid_x = conv_pw_wgrad_grid_x(a, sw.pwgrad_wgs);
    p.bytes = (int64_t)p.grid_x * a.ncot * a.ncig * 4 * pwgrad::block(p.sub) * (int64_t)sizeof(double);
    return p;
}

// ---- stem -------------------------------------------------------------------------------------------------------------------------------------
Plan<StemWgradArgs> plan_stem(int precision, const float *x, const void *gy, int B, int N, int H, int W) {
    Plan<StemWgradArgs> p{};
    p.rc = check_volume("the stem backward", precision, B, N, H, W, {}, 1, (int64_t)B * N * H * W, "pixels");   // (x is indexed by the pixel)
    if (p.rc) return p;
    const Switches sw = Switches::read();
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
    a.flush_units = std::max(1, std::min(sw.wgrad_flush_units * (wgrad::TY * wgrad::TX) / (stemw::TY * stemw::TX), stemw::FLUSH_UNITS));
    p.grid_x = stem_wgrad_grid_x(a, sw.wgrad_wgs);
    p.bytes = (int64_t)p.grid_x * stemw::BLOCK * (int64_t)sizeof(double);
    return p;
}

// ---- score ------------------------------------------------------------------------------------------------------------------------------------
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

// both gradients; `bytes` and `grid_x` are the weight gradient's
Plan<ScoreArgs> plan_score(int precision, int B, int Cin, int N, int H, int W, const int kernel[3], const int pad[3]) {
    Plan<ScoreArgs> p{};
    const int k = p.sub = kernel_of(kernel, pad);
    const int64_t M = (int64_t)B * N * H * W;
    static_assert(score::MAX_C == 128, "check_volume's channel limit");
    p.rc = !k ? DFFW_EINVAL : check_volume("the score conv backward", precision, B, N, H, W, {Cin}, 1, M, "pixels");
    if (p.rc) return p;
    ScoreArgs &a = p.a;
    a.C = Cin;
    a.M = (int)M;
    a.N = N;
    a.H = H;
    a.W = W;
    a.tiles_y = (H + score::TY - 1) / score::TY;
    a.tiles_x = (W + score::TX - 1) / score::TX;
    a.total_units = score_units(k, B, N, H, W);
    p.wgs = Switches::read().score_wgs;
    p.grid_x = score_grid(a.total_units, p.wgs);
    p.bytes = (int64_t)p.grid_x * a.C * (k * k * k) * (int64_t)sizeof(double);
    return p;
}

// ---- att --------------------------------------------------------------------------------------------------------------------------------------
Plan<AttGradArgs> plan_att(int precision, int B, int C, int N, int H, int W) {
    Plan<AttGradArgs> p{};
    if (C != 8 && C != 16 && C != 32) {
        p.rc = fail(DFFW_EINVAL, "the attention tails have 8, 16 or 32 channels, got %d", C);
        return p;
    }
    // two counts are ints in the kernel: the plane rounded up to whole chunks, and the units B * chunks
    const int64_t HW = (int64_t)H * W, chunks = (HW + attgrad::P - 1) / attgrad::P;
    p.rc = check_volume("the attention tail backward", precision, B, N, H, W, {C}, 1, std::max(HW + attgrad::P, B * chunks), "pixels of a plane or units");
    if (p.rc) return p;
    const Switches sw = Switches::read();
    AttGradArgs &a = p.a;
    a.B = B;
    a.N = N;
    a.HW = H * W;
    a.chunks = (int)chunks;
    a.total_units = B * a.chunks;
    a.flush_steps = std::min(sw.attgrad_flush_steps, attgrad::FLUSH_STEPS);
    p.sub = C;
    p.grid_x = att_tail_bwd_grid_x(a, sw.attgrad_wgs);
    p.bytes = (int64_t)p.grid_x * attgrad::block(C) * (int64_t)sizeof(double);
    return p;
}

}  // namespace

int dffw::att_tail_backward_check(int precision, int B, int C, int N, int H, int W) { return plan_att(precision, B, C, N, H, W).rc; }
int dffw::conv_backward_check(int precision, int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int stride[3], const int pad[3],
                              int transposed) {
    return plan_conv(precision, nullptr, B, Cin, N, H, W, nullptr, Cout, kernel, stride, pad, transposed).rc;
}
int dffw::conv_cat_backward_check(int precision, int B, int Ca, int Cb, int N, int H, int W, int Cout) {
    return plan_conv_cat(precision, nullptr, Ca, nullptr, Cb, B, N, H, W, nullptr, Cout).rc;
}
int dffw::conv_pw_backward_check(int precision, int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int pad[3]) {
    return plan_pw(precision, nullptr, B, Cin, N, H, W, nullptr, Cout, kernel, pad).rc;
}
int dffw::stem_backward_check(int precision, int B, int N, int H, int W) { return plan_stem(precision, nullptr, nullptr, B, N, H, W).rc; }
int dffw::score_conv_backward_check(int precision, int B, int Cin, int N, int H, int W, const int kernel[3], const int pad[3]) {
    return plan_score(precision, B, Cin, N, H, W, kernel, pad).rc;
}

extern "C" {

int64_t dffw_conv_wgrad_workspace_bytes(int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int stride[3], const int pad[3],
                                        int transposed) {
    return plan_conv(0, nullptr, B, Cin, N, H, W, nullptr, Cout, kernel, stride, pad, transposed).bytes;
}

int dffw_conv_wgrad(int device, int precision, const void *x, int B, int Cin, int N, int H, int W, const void *grad_y, int Cout, const int kernel[3],
                    const int stride[3], const int pad[3], int transposed, float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<WgradArgs> p = plan_conv(precision, x, B, Cin, N, H, W, grad_y, Cout, kernel, stride, pad, transposed);
    if (p.rc) return p.rc;
    if (!x || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(x, 16) || !aligned(grad_y, 16) || !aligned(workspace, 8)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    p.a.partial = (double *)workspace;
    return launch_record("wgrad", p.bytes, workspace_bytes, device, conv_wgrad_kernel_name(precision, p.sub), "dffw::conv_wgrad_finish_kernel",
                         [&] { return launch_conv_wgrad(precision, p.sub, p.a, p.grid_x, grad_w, (hipStream_t)hip_stream); });
}

int64_t dffw_conv_cat_wgrad_workspace_bytes(int B, int Ca, int Cb, int N, int H, int W, int Cout) {
    return plan_conv_cat(0, nullptr, Ca, nullptr, Cb, B, N, H, W, nullptr, Cout).bytes;
}

int dffw_conv_cat_wgrad(int device, int precision, const void *xa, int Ca, const void *xb, int Cb, int B, int N, int H, int W, const void *grad_y, int Cout,
                        float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<WgradCatArgs> p = plan_conv_cat(precision, xa, Ca, xb, Cb, B, N, H, W, grad_y, Cout);
    if (p.rc) return p.rc;
    if (!xa || !xb || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(xa, 16) || !aligned(xb, 16) || !aligned(grad_y, 16) || !aligned(workspace, 8)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    p.a.partial = (double *)workspace;
    return launch_record("wgrad", p.bytes, workspace_bytes, device, conv_wgrad_cat_kernel_name(precision), "dffw::conv_wgrad_finish_kernel",
                         [&] { return launch_conv_wgrad_cat(precision, p.a, p.grid_x, grad_w, (hipStream_t)hip_stream); });
}

int64_t dffw_conv_pw_wgrad_workspace_bytes(int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int pad[3]) {
    return plan_pw(0, nullptr, B, Cin, N, H, W, nullptr, Cout, kernel, pad).bytes;
}

int dffw_conv_pw_wgrad(int device, int precision, const void *x, int B, int Cin, int N, int H, int W, const void *grad_y, int Cout, const int kernel[3],
                       const int pad[3], float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<PwgradArgs> p = plan_pw(precision, x, B, Cin, N, H, W, grad_y, Cout, kernel, pad);
    if (p.rc) return p.rc;
    if (!x || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(x, 16) || !aligned(grad_y, 16) || !aligned(workspace, 8)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    p.a.partial = (double *)workspace;
    return launch_record("wgrad", p.bytes, workspace_bytes, device, conv_pw_wgrad_kernel_name(precision, p.sub), "dffw::conv_pw_wgrad_finish_kernel",
                         [&] { return launch_conv_pw_wgrad(precision, p.sub, p.a, p.grid_x, grad_w, (hipStream_t)hip_stream); });
}

int64_t dffw_att_tail_backward_workspace_bytes(int B, int C, int N, int H, int W) { return plan_att(0, B, C, N, H, W).bytes; }

int dffw_att_tail_backward(int device, int precision, const void *x, const void *a, const void *t, const void *grad_y, int B, int C, int N, int H, int W,
                           const float *w3, const float *w1, void *grad_x, float *grad_w3, float *grad_w1, void *workspace, int64_t workspace_bytes,
                           void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<AttGradArgs> p = plan_att(precision, B, C, N, H, W);
    if (p.rc) return p.rc;
    if ((grad_w3 != nullptr) != (grad_w1 != nullptr)) return fail(DFFW_EINVAL, "grad_w3 and grad_w1 go together");
    if (!grad_x && !grad_w3) return DFFW_OK;   // no output: nothing to launch
    if (!x || !a || !t || !grad_y || !w1 || (grad_x && !w3) || (grad_w3 && !workspace)) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(x, 16) || !aligned(a, 16) || !aligned(t, 16) || !aligned(grad_y, 16) || !aligned(grad_x, 16) || !aligned(workspace, 8))
        return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    if (!aligned(w3, 4) || !aligned(w1, 4) || !aligned(grad_w3, 4) || !aligned(grad_w1, 4)) return fail(DFFW_EINVAL, "the filters and their gradients must be 4-byte aligned");
    p.a.x = (const uint16_t *)x;
    p.a.a = (const uint16_t *)a;
    p.a.t = (const uint16_t *)t;
    p.a.gy = (const uint16_t *)grad_y;
    p.a.gx = (uint16_t *)grad_x;
    p.a.w3 = w3;
    p.a.w1 = w1;
    p.a.partial = grad_w3 ? (double *)workspace : nullptr;
    const char *kernel = att_tail_bwd_kernel_name(precision, C);
    if (!grad_w3) {
        HIPCHK(hipSetDevice(device));
        HIPCHK(launch_att_tail_bwd(precision, C, p.a, p.grid_x, nullptr, nullptr, (hipStream_t)hip_stream));
        dffw_set_last_op_kernels(kernel);
        return DFFW_OK;
    }
    return launch_record("attention tail backward", p.bytes, workspace_bytes, device, kernel, "dffw::att_tail_bwd_finish_kernel",
                         [&] { return launch_att_tail_bwd(precision, C, p.a, p.grid_x, grad_w3, grad_w1, (hipStream_t)hip_stream); });
}

int64_t dffw_stem_wgrad_workspace_bytes(int B, int N, int H, int W) { return plan_stem(0, nullptr, nullptr, B, N, H, W).bytes; }

int dffw_stem_wgrad(int device, int precision, const float *x, const void *grad_y, int B, int N, int H, int W, float *grad_w, void *workspace,
                    int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<StemWgradArgs> p = plan_stem(precision, x, grad_y, B, N, H, W);
    if (p.rc) return p.rc;
    if (!x || !grad_y || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(grad_y, 16) || !aligned(x, 4) || !aligned(workspace, 8))
        return fail(DFFW_EINVAL, "grad_y (records) must be 16-byte aligned, x (fp32) 4-byte aligned, the workspace 8-byte aligned");
    p.a.partial = (double *)workspace;
    return launch_record("wgrad", p.bytes, workspace_bytes, device, stem_wgrad_kernel_name(precision), "dffw::stem_wgrad_finish_kernel",
                         [&] { return launch_stem_wgrad(precision, p.a, p.grid_x, grad_w, (hipStream_t)hip_stream); });
}

int dffw_score_conv_dgrad(int device, int precision, const float *grad_score, int B, int Cin, int N, int h, int w, const float *weight, const int kernel[3],
                          const int pad[3], const void *b, void *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<ScoreArgs> p = plan_score(precision, B, Cin, N, h, w, kernel, pad);
    if (p.rc) return p.rc;
    if (!grad_score || !weight || !out) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(b, 16) || !aligned(out, 16)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    if (!aligned(grad_score, 4) || !aligned(weight, 4)) return fail(DFFW_EINVAL, "grad_score and weight must be 4-byte aligned");
    HIPCHK(hipSetDevice(device));
    p.a.g = grad_score;
    p.a.w = weight;
    p.a.b = (const uint16_t *)b;
    p.a.out = (uint16_t *)out;
    HIPCHK(launch_score_dgrad(precision, p.sub, p.a, p.wgs, (hipStream_t)hip_stream));
    dffw_set_last_op_kernels(score_dgrad_kernel_name(precision, p.sub, b != nullptr));
    return DFFW_OK;
}

int64_t dffw_score_conv_wgrad_workspace_bytes(int B, int Cin, int N, int h, int w, const int kernel[3], const int pad[3]) {
    return plan_score(0, B, Cin, N, h, w, kernel, pad).bytes;
}

int dffw_score_conv_wgrad(int device, int precision, const void *x, const float *grad_score, int B, int Cin, int N, int h, int w, const int kernel[3],
                          const int pad[3], float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    Plan<ScoreArgs> p = plan_score(precision, B, Cin, N, h, w, kernel, pad);
    if (p.rc) return p.rc;
    if (!x || !grad_score || !grad_w || !workspace) return fail(DFFW_EINVAL, "null argument");
    if (!aligned(x, 16)) return fail(DFFW_EINVAL, "records must be 16-byte aligned");
    if (!aligned(grad_score, 4) || !aligned(grad_w, 4) || !aligned(workspace, 8))
        return fail(DFFW_EINVAL, "grad_score and grad_w must be 4-byte aligned, the workspace 8-byte aligned");
    p.a.x = (const uint16_t *)x;
    p.a.g = grad_score;
    p.a.partial = (double *)workspace;
    return launch_record("score wgrad", p.bytes, workspace_bytes, device, score_wgrad_kernel_name(precision, p.sub), "dffw::score_wgrad_finish_kernel",
                         [&] { return launch_score_wgrad(precision, p.sub, p.a, p.wgs, grad_w, (hipStream_t)hip_stream); });
}

}  // extern "C"
