// The single-operator entry points of libdffw.so (dffw_op_*, include/dffw.h): one kernel family on fp32 NCDHW tensors, for the per-element
// bounds and the kernel-name assertions of the GPU tests.  Test-only: the forward never comes here.  Every op that moves tensors is a body
// on one shell (run_op): the body allocates from a Run's arena, stages its inputs into activation records, runs the graph's own code on
// them (Run::conv, srd(), efd(), of_block(), head_first_conv(), head_tail(), the record-form ABIs of dffw_grad.cpp / dffw_bn.cpp / dffw_pool_grad.cpp) and stages the outputs back.
#include <functional>
#include <string>
#include <vector>

#include "dffw_bn.h"
#include "dffw_att_grad.h"
#include "dffw_conv_pw_wgrad.h"
#include "dffw_conv_wgrad.h"
#include "dffw_pool_grad.h"
#include "dffw_run.h"
#include "dffw_score_grad.h"
#include "dffw_stem_wgrad.h"

using namespace dffw;

namespace {

// An op's private engine: the layers it packs, in the op's arithmetic.
struct OpEngine : dffw_engine {
    OpEngine(int device_, int prec_) { device = device_; prec = prec_; }
};

// The one device block of an op: synchronises the stream and frees on every way out of the scope, so no kernel outlives its workspace.
struct OpBlock {
    char *p = nullptr;
    hipStream_t s;
    explicit OpBlock(hipStream_t s_) : s(s_) {}
    OpBlock(const OpBlock &) = delete;
    OpBlock &operator=(const OpBlock &) = delete;
    hipError_t alloc(int64_t bytes) { return hipMalloc((void **)&p, bytes); }
    ~OpBlock() {
        if (!p) return;
        (void)hipStreamSynchronize(s);
        (void)hipFree(p);
    }
};

// Runs `body` twice on `eng`: a dry run sizes the arena (as dffw_workspace_bytes does), the real run gets ONE private block of that size
// filled with 0xFF -- NaN in fp32, bf16 and fp16, so an output element no kernel stores, or a workspace value read before it is written,
// shows as NaN instead of as whatever a recycled block held.  Returns the first error, after the stream has drained.
// record: every launch of the real run is profiled and the kernel names, in launch order, become dffw_last_op_kernels(); otherwise that
// list is left to the body (the record-form ABIs set it themselves; the staging kernels are never part of it).
int run_op(dffw_engine &eng, hipStream_t s, bool record, const std::function<void(Run &)> &body) {
    int64_t need;
    {
        Run d(&eng, s, true, nullptr, INT64_MAX / 2);
        body(d);
        if (!d.ok()) return d.err;
        need = d.arena.peak();
    }
    const int64_t bytes = need + 65536;   // (the slack a caching allocator's block would give the forward's workspace)
    OpBlock ws(s);
    HIPCHK(ws.alloc(bytes));
    HIPCHK(hipMemsetAsync(ws.p, 0xFF, bytes, s));
    eng.profiling = record;
    int rc;
    {
        Run r(&eng, s, false, ws.p, bytes);
        body(r);
        rc = r.err;
    }
    const hipError_t se = hipStreamSynchronize(s);
    if (rc == DFFW_OK && se != hipSuccess) rc = fail(DFFW_EHIP, "sync: %s", hipGetErrorString(se));
    if (record) {
        std::string names;
        for (const ProfRec &pr : eng.recs) names += (names.empty() ? "" : ";") + pr.kernel;
        dffw_set_last_op_kernels(names.c_str());
    }
    return rc;
}

// what a body does in the real run only
bool real(const Run &r) { return r.ok() && !r.dry; }

// an arena piece with the records of the fp32 NCDHW tensor x
Act stage_in(Run &r, const float *x, int B, int C, int N, int H, int W) {
    Act a = r.act(B, N, H, W, C);
    if (real(r)) r.check(launch_from_ncdhw(r.e->prec, x, a.p, B, C, N, H, W, r.s), "from_ncdhw");
    return a;
}
// ... and back: the records of `a` as the fp32 NCDHW tensor y
void stage_out(Run &r, const Act &a, float *y) {
    if (real(r)) r.check(launch_to_ncdhw(r.e->prec, a.p, y, a.B, a.C, a.N, a.H, a.W, r.s), "to_ncdhw");
}
// ... of an fp32 score volume of n values
void copy_out(Run &r, const float *score, float *y, int64_t n) {
    if (real(r)) r.check(hipMemcpyAsync(y, score, n * sizeof(float), hipMemcpyDeviceToDevice, r.s), "copy");
}

// the filter of the adjoint conv of a stride-1 conv (Cout, Cin, taps): every tap flipped, in and out channels swapped -> (Cin, Cout, taps)
std::vector<float> adjoint_filter(const float *weight, int Cout, int Cin, int64_t taps) {
    std::vector<float> wa((size_t)Cin * Cout * taps);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int64_t t = 0; t < taps; ++t) wa[((size_t)ci * Cout + co) * taps + (taps - 1 - t)] = weight[((size_t)co * Cin + ci) * taps + t];
    return wa;
}

// A weight-gradient op: x and grad_y staged into records (a null tensor is not staged: the record form reads the op's own fp32 one), `wsb` bytes of
// workspace, and in the real run `call(x's records, grad_y's records, workspace, stream)`, a record form of dffw_grad.cpp.  It sets
// dffw_last_op_kernels() itself
struct Staged {
    const float *t;
    int C, H, W;
};
int run_wgrad_op(int device, int precision, int B, int N, Staged x, Staged gy, int64_t wsb, hipStream_t s,
                 const std::function<int(const void *, const void *, void *, hipStream_t)> &call) {
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, s, false, [&](Run &r) {
        Act xa = x.t ? stage_in(r, x.t, B, x.C, N, x.H, x.W) : Act(), ya = gy.t ? stage_in(r, gy.t, B, gy.C, N, gy.H, gy.W) : Act();
        void *ws = r.raw(wsb);
        if (real(r)) r.err = call(xa.p, ya.p, ws, r.s);
    });
}
// ... of a conv with two sources: `call(xa's records, xb's records, grad_y's records, workspace, stream)`
int run_wgrad_op(int device, int precision, int B, int N, Staged xa, Staged xb, Staged gy, int64_t wsb, hipStream_t s,
                 const std::function<int(const void *, const void *, const void *, void *, hipStream_t)> &call) {
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, s, false, [&](Run &r) {
        Act aa = stage_in(r, xa.t, B, xa.C, N, xa.H, xa.W), ba = stage_in(r, xb.t, B, xb.C, N, xb.H, xb.W), ya = stage_in(r, gy.t, B, gy.C, N, gy.H, gy.W);
        void *ws = r.raw(wsb);
        if (real(r)) r.err = call(aa.p, ba.p, ya.p, ws, r.s);
    });
}

}  // namespace

extern "C" {

int dffw_op_conv3d(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *weight,
                   int Cout, const int kernel[3], const int stride[3], const int pad[3], const int dilation[3], int transposed,
                   const float *bn, const float *conv_bias, const float *residual, int relu, float *y, void *hip_stream) {
    return dffw_op_conv3d_ex(device, precision, x, B, Cin, N, H, W, weight, Cout, kernel, stride, pad, dilation, transposed, bn, conv_bias, residual, relu, y,
                             nullptr, nullptr, nullptr, hip_stream);
}

int dffw_op_conv3d_ex(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *weight,
                      int Cout, const int kernel[3], const int stride[3], const int pad[3], const int dilation[3], int transposed,
                      const float *bn, const float *conv_bias, const float *residual, int relu, float *y, float *y_pre, const float *cls_weight,
                      float *cls_score, void *hip_stream) {
    if (!x || !weight || !y || !kernel || !stride || !pad || !dilation) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (stride[0] != 1 || dilation[0] != 1) return fail(DFFW_EINVAL, "slice stride/dilation must be 1");
    if (stride[1] != stride[2] || dilation[1] != dilation[2]) return fail(DFFW_EINVAL, "row/col stride and dilation must match");
    if (Cout != 1 && Cout % 4) return fail(DFFW_EINVAL, "Cout must be 1 or a multiple of 4");
    if (Cout > 128) return fail(DFFW_EINVAL, "Cout > 128 unsupported");
    HIPCHK(hipSetDevice(device));
    LayerDef L{"op", "", Cin, Cout, kernel[0], kernel[1], kernel[2], stride[1], stride[2], pad[0], pad[1], pad[2],
               dilation[1], dilation[2], transposed != 0, true, false};
    if (transposed && !(kernel[0] == 3 && kernel[1] == 3 && kernel[2] == 3 && stride[1] == 2 && pad[0] == 1 && pad[1] == 1 && pad[2] == 1))
        return fail(DFFW_EINVAL, "transposed conv supports only k3 s(1,2,2) p1 op(0,1,1)");
    OpEngine eng(device, precision);
    int rc = pack_conv(L, precision, weight, bn, conv_bias, eng.convs["op"]);
    if (rc) return rc;
    if ((cls_weight != nullptr) != (cls_score != nullptr)) return fail(DFFW_EINVAL, "cls_weight and cls_score go together");
    if ((y_pre || cls_weight) && (Cout == 1 || Cout % 8)) return fail(DFFW_EINVAL, "second output / fused classifier need Cout %% 8 == 0");
    if (cls_weight) {   // the 1x1x1 Cout -> 1 classifier applied to the final value (DEN.py:51-55), bias-free, no BatchNorm
        LayerDef C{"cls", "", Cout, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, false, true, false};
        rc = pack_conv(C, precision, cls_weight, nullptr, nullptr, eng.convs["cls"]);
        if (rc) return rc;
    }
    const int cpad = (Cin + 7) / 8 * 8;
    const bool stem = (!transposed && kernel[0] == 1 && kernel[1] == 9 && kernel[2] == 9 && dilation[1] == 2 && pad[0] == 0 && pad[1] == 8 &&
                       stride[1] == 1 && Cin == 3);
    // through the same Run::conv path the graph uses; dffw_last_op_kernels() is not this op's to set
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        // the input records; zero-filled first (the arena is 0xFF) where the volume is wider than the tensor: the stem's paired-pixel volume of
        // width W + 2 and the volume whose channels are padded to a multiple of 8
        Act in = r.act(B, N, H, stem ? W + 2 : W, cpad);
        const int64_t plane = (int64_t)N * H * W;
        float *xp = !stem && cpad != Cin ? (float *)r.raw(B * cpad * plane * (int64_t)sizeof(float)) : nullptr;
        if (real(r)) {
            if (stem || xp) r.check(hipMemsetAsync(in.p, 0, (size_t)in.pixels() * prec_parts(precision) * cpad * 2, r.s), "input memset");
            if (stem) {
                r.check(launch_stack_in(precision, x, in.p, B, N, H, W, r.s), "stack_in");   // the stem's paired-pixel input format
            } else if (!xp) {
                r.check(launch_from_ncdhw(precision, x, in.p, B, Cin, N, H, W, r.s), "from_ncdhw");
            } else {   // the Cin real channels in the first channels of a zero-padded fp32 volume
                r.check(hipMemsetAsync(xp, 0, (size_t)B * cpad * plane * sizeof(float), r.s), "input memset");
                for (int b = 0; b < B && r.ok(); ++b)
                    r.check(hipMemcpyAsync(xp + (int64_t)b * cpad * plane, x + (int64_t)b * Cin * plane, (size_t)Cin * plane * sizeof(float),
                                           hipMemcpyDeviceToDevice, r.s), "copy");
                if (r.ok()) r.check(launch_from_ncdhw(precision, xp, in.p, B, cpad, N, H, W, r.s), "from_ncdhw");
            }
        }
        const int No = N + 2 * pad[0] - (kernel[0] - 1);
        const int Ho = transposed ? 2 * H : (H + 2 * pad[1] - dilation[1] * (kernel[1] - 1) - 1) / stride[1] + 1;
        const int Wo = transposed ? 2 * W : (W + 2 * pad[2] - dilation[2] * (kernel[2] - 1) - 1) / stride[2] + 1;
        const int64_t opix = (int64_t)B * No * Ho * Wo;
        ConvOpt o;
        o.relu = relu;
        Act res, pre;
        if (Cout == 1) {
            o.outf = (float *)r.raw(opix * sizeof(float));
        } else if (residual) {
            res = stage_in(r, residual, B, Cout, No, Ho, Wo);
            o.res0 = &res;
        }
        if (y_pre) o.out_pre = &pre;
        if (cls_weight) {
            o.cls = "cls";
            o.cls_out = (float *)r.raw(opix * sizeof(float));
        }
        Act out = r.conv("op", in, o);
        if (Cout == 1) copy_out(r, o.outf, y, opix);
        else stage_out(r, out, y);
        if (y_pre) stage_out(r, pre, y_pre);
        if (cls_weight) copy_out(r, o.cls_out, cls_score, opix);
    });
}

// The forward 3x3x3 stride-1 conv over the virtual concatenation [xa | xb] (ConvOpt::in1), as the hourglass conv0 layers and the pyramid's
// combine1 / combine2 run it: one layer of Ca + Cb input channels (pack_conv sees only the total), each tensor staged into records of its own,
// through the same Run::conv path the graph uses; dffw_last_op_kernels() is not this op's to set
int dffw_op_conv3d_cat(int device, int precision, const float *xa, int Ca, const float *xb, int Cb, int B, int N, int H, int W, const float *weight,
                       int Cout, const float *bn, const float *conv_bias, const float *residual, int relu, float *y, void *hip_stream) {
    if (!xa || !xb || !weight || !y) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (Ca < 8 || Cb < 8 || Ca % 8 || Cb % 8 || (int64_t)Ca + Cb > 192)
        return fail(DFFW_EINVAL, "Ca and Cb must be multiples of 8 from 8 on with Ca + Cb <= 192, got %d and %d", Ca, Cb);
    if (Cout < 8 || Cout % 8 || Cout > 128) return fail(DFFW_EINVAL, "Cout must be a multiple of 8 from 8 to 128, got %d", Cout);
    HIPCHK(hipSetDevice(device));
    LayerDef L{"op", "", Ca + Cb, Cout, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, false, true, false};
    OpEngine eng(device, precision);
    if (int rc = pack_conv(L, precision, weight, bn, conv_bias, eng.convs["op"])) return rc;
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act a = stage_in(r, xa, B, Ca, N, H, W), b = stage_in(r, xb, B, Cb, N, H, W), res;
        ConvOpt o;
        o.relu = relu;
        o.in1 = &b;
        if (residual) {
            res = stage_in(r, residual, B, Cout, N, H, W);
            o.res0 = &res;
        }
        stage_out(r, r.conv("op", a, o), y);
    });
}

int dffw_op_pool(int device, int precision, int mode, int k, const float *x, int B, int C, int N, int H, int W, float *y,
                 void *hip_stream) {
    if (!x || !y) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (C % 8 || k < 1 || H % k || W % k) return fail(DFFW_EINVAL, "pool needs C %% 8 == 0 and H,W divisible by k");
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act in = stage_in(r, x, B, C, N, H, W);
        stage_out(r, r.pool(in, mode, k), y);
    });
}

int dffw_op_pool3(int device, int precision, const float *x, int B, int C, int N, int H, int W, float *p2, float *p4, float *p8, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!x || !p2 || !p4 || !p8) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (B < 1 || C < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape");
    if (C % 8 || H % 8 || W % 8) return fail(DFFW_EINVAL, "the pyramid's pools need C, H and W multiples of 8, got C %d, %dx%d", C, H, W);
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, true, [&](Run &r) {
        Act in = stage_in(r, x, B, C, N, H, W), a2, a4, a8;
        r.pool3(in, a2, a4, a8);
        stage_out(r, a2, p2);
        stage_out(r, a4, p4);
        stage_out(r, a8, p8);
    });
}

// ---- block entry points: one SRD / EFD block of the front end, one feature block of the alignment network, through the graph's own
// srd() / efd() / of_block().  The block's convs are packed under the keys the graph looks up, so the dispatch is the forward's itself.
int dffw_op_srd(int device, int precision, const float *x, int B, int C, int N, int H, int W, const float *w0, const float *bn0,
                const float *w2, const float *bn2, const float *w3, const float *w1, float *y, float *pooled, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!x || !w0 || !bn0 || !w2 || !bn2 || !w3 || !w1 || !y) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (C != 8 && C != 16 && C != 32) return fail(DFFW_EINVAL, "the SRD blocks have 8, 16 or 32 channels, got %d", C);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape");
    if (pooled && (H % 2 || W % 2)) return fail(DFFW_EINVAL, "the pooled copy needs even H and W, got %dx%d", H, W);
    HIPCHK(hipSetDevice(device));
    const std::string p = C == 8 ? "DFF_net.FM_measure.Focus_extraction.2" : C == 16 ? "DFF_net.FM_conv1.1" : "DFF_net.FM_conv2.1";
    const std::vector<LayerDef> layers = srd_layers(p, C);
    const float *const wts[4] = {w0, w2, w3, w1}, *const bns[4] = {bn0, bn2, nullptr, nullptr};
    OpEngine eng(device, precision);
    for (int i = 0; i < 4; ++i) {
        const int rc = pack_conv(layers[i], precision, wts[i], bns[i], nullptr, eng.convs[layers[i].conv]);
        if (rc) return rc;
    }
    return run_op(eng, (hipStream_t)hip_stream, true, [&](Run &r) {
        Act in = stage_in(r, x, B, C, N, H, W);
        Act pl;
        Act out = srd(r, p, in, true, pooled ? &pl : nullptr);
        if (pooled && !pl.p) pl = r.pool(out, 0, 2);   // (this path writes no pooled copy: the engine's pool kernel, as efd() then runs it)
        stage_out(r, out, y);
        if (pooled) stage_out(r, pl, pooled);
    });
}

int dffw_op_efd(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *ws, const float *bns,
                const float *wp, const float *bnp, int pooled_at_hand, float *y, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!x || !ws || !bns || !wp || !bnp || !y) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (Cin != 8 && Cin != 16) return fail(DFFW_EINVAL, "the EFD blocks have 8 or 16 input channels, got %d", Cin);
    if (B < 1 || N < 1 || H < 2 || W < 2 || H % 2 || W % 2) return fail(DFFW_EINVAL, "bad shape (H and W must be even)");
    HIPCHK(hipSetDevice(device));
    const std::string p = Cin == 8 ? "DFF_net.FM_conv1.0" : "DFF_net.FM_conv2.0";
    const std::vector<LayerDef> layers = efd_layers(p, Cin, 2 * Cin);
    const float *const wts[2] = {ws, wp}, *const bnv[2] = {bns, bnp};
    OpEngine eng(device, precision);
    for (int i = 0; i < 2; ++i) {
        const int rc = pack_conv(layers[i], precision, wts[i], bnv[i], nullptr, eng.convs[layers[i].conv]);
        if (rc) return rc;
    }
    return run_op(eng, (hipStream_t)hip_stream, true, [&](Run &r) {
        Act in = stage_in(r, x, B, Cin, N, H, W);
        Act m;   // the pooled copy "at hand", as srd() leaves it for the forward's efd()
        if (pooled_at_hand) m = r.pool(in, 0, 2);
        stage_out(r, efd(r, p, in, &m), y);
    });
}

int dffw_op_of_block(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, int Cout, int stride,
                     const float *w0, const float *bn0, const float *w2, const float *bn2, const float *wf, float *y, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!x || !w0 || !bn0 || !w2 || !bn2 || !wf || !y) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    static const struct { int cin, cout, s; const char *name; } blocks[] = {
        {3, 8, 1, "OF_feature.0"}, {8, 8, 1, "OF_feature.1"}, {8, 16, 2, "OF_feature1.0"},
        {16, 16, 1, "OF_feature1.1"}, {16, 32, 2, "OF_feature2.0"}, {32, 32, 1, "OF_feature2.1"}};
    const char *name = nullptr;
    for (const auto &b : blocks)
        if (b.cin == Cin && b.cout == Cout && b.s == stride) name = b.name;
    if (!name) return fail(DFFW_EINVAL, "no alignment feature block has (Cin, Cout, stride) = (%d, %d, %d)", Cin, Cout, stride);
    if (B < 1 || N < 1 || H < 1 || W < 1 || H % stride || W % stride) return fail(DFFW_EINVAL, "bad shape (H and W must be multiples of the stride)");
    HIPCHK(hipSetDevice(device));
    const std::string p = std::string("optical_flow_aggregation.") + name;
    OpEngine eng(device, precision);
    for (const LayerDef &L : of_block_layers(p, Cin, Cout, stride)) {   // as dffw_engine_create packs them: a stride-1 block's shortcut folded into conv.2
        if (L.folded) continue;
        const bool sc = !L.shortcut.empty();
        const float *w = L.conv == p + ".conv.0.0" ? w0 : L.conv == p + ".conv.2.0" ? w2 : wf;
        const float *bn = L.conv == p + ".conv.0.0" ? bn0 : L.conv == p + ".conv.2.0" ? bn2 : nullptr;
        const int rc = pack_conv(L, precision, w, bn, nullptr, eng.convs[L.conv], sc ? wf : nullptr, sc ? Cin : 0);
        if (rc) return rc;
    }
    return run_op(eng, (hipStream_t)hip_stream, true, [&](Run &r) {
        Act out;
        if (Cin == 3) {
            out = of_first_block(r, p, x, B, N, H, W);
        } else {
            Act in = stage_in(r, x, B, Cin, N, H, W);
            out = of_block(r, p, in);
        }
        stage_out(r, out, y);
    });
}

// The back half of one alpha head through the graph's own head_tail() (start = 0: x is the first conv's output y0) or its end alone,
// head_tail_stored() (start = 2: x is y2), with convs .2.0, .4.0 and .6 packed under the names of the head C selects.
int dffw_op_head_tail(int device, int precision, const float *x, int B, int C, int N, int H, int W, const float *w2, const float *bn2,
                      const float *w4, const float *bn4, const float *w6, const float *bias6, int start, float *alpha, float *raw, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!x || !w2 || !bn2 || !w4 || !bn4 || !w6 || !bias6 || !alpha || !raw) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (C != 16 && C != 32 && C != 64) return fail(DFFW_EINVAL, "the alpha heads have 16, 32 or 64 channels, got %d", C);
    if (start != 0 && start != 2) return fail(DFFW_EINVAL, "start must be 0 (x is y0) or 2 (x is y2), got %d", start);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if ((int64_t)B * N * 3 > 65535) return fail(DFFW_EINVAL, "B * N * 3 = %lld planes do not fit one launch grid dimension (65535)", (long long)B * N * 3);
    HIPCHK(hipSetDevice(device));
    const char *head = C == 16 ? "conv3" : C == 32 ? "conv2" : "conv1";
    const std::string hp = std::string("optical_flow_aggregation.") + head, label = std::string("flow.") + head;
    OpEngine eng(device, precision);
    for (const LayerDef &L : alpha_head_layers(hp, C + 2, C)) {   // as dffw_engine_create packs them; the first conv is not this op's
        const bool l2 = L.conv == hp + ".2.0", l4 = L.conv == hp + ".4.0", l6 = L.conv == hp + ".6";
        if (!l2 && !l4 && !l6) continue;
        const int rc = pack_conv(L, precision, l2 ? w2 : l4 ? w4 : w6, l2 ? bn2 : l4 ? bn4 : nullptr, l6 ? bias6 : nullptr, eng.convs[L.conv]);
        if (rc) return rc;
    }
    return run_op(eng, (hipStream_t)hip_stream, true, [&](Run &r) {
        Act in = stage_in(r, x, B, C, N, H, W);
        if (start == 0) head_tail(r, hp, label, in, alpha, raw);
        else head_tail_stored(r, hp, label, in, alpha, raw);
    });
}

// The front half of one alpha head through the graph's own head_first_conv(): fe warped by (alpha, fov), [ref | cur | flow] through conv .0.0,
// packed (whole and as its #ref / #cur halves) under the names of the head C selects.
int dffw_op_head_front(int device, int precision, const float *fe, int B, int C, int N, int H, int W, const float *w0, const float *bn0,
                       const float *alpha, const float *fov, float *y0, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!fe || !w0 || !bn0 || !alpha || !fov || !y0) return fail(DFFW_EINVAL, "null argument");
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (C != 8 && C != 16 && C != 32) return fail(DFFW_EINVAL, "the alpha heads take level features of 8, 16 or 32 channels, got %d", C);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    HIPCHK(hipSetDevice(device));
    const char *head = C == 8 ? "conv3" : C == 16 ? "conv2" : "conv1";
    const std::string hp = std::string("optical_flow_aggregation.") + head, label = std::string("flow.") + head;
    OpEngine eng(device, precision);
    for (const LayerDef &L : alpha_head_layers(hp, 2 * C + 2, 2 * C)) {   // as dffw_engine_create packs them; the other convs are not this op's
        if (L.conv != hp + ".0.0") continue;
        int rc = pack_conv(L, precision, w0, bn0, nullptr, eng.convs[L.conv]);
        if (!rc && L.head_split > 0) rc = pack_head_split(L, precision, w0, bn0, eng.convs[L.conv + "#ref"], eng.convs[L.conv + "#cur"]);
        if (rc) return rc;
    }
    return run_op(eng, (hipStream_t)hip_stream, true, [&](Run &r) {
        Act in = stage_in(r, fe, B, C, N, H, W);
        stage_out(r, head_first_conv(r, hp, label, in, alpha, fov), y0);
    });
}

// The refusals of the two regression-head entry points, before any GPU call: with N < 1 the kernels' slice clamp (N - 1) reads in front of the
// score volume, and a size below 1 makes the tap clamp (h - 1, w - 1) negative.
static int regress_check(int n_heads, const float *const *score, const int *h, const int *w, float *const *depth, int B, int N, int H, int W,
                         const float *focus_dists, const int64_t *fd_strides) {
    if (!score || !h || !w || !depth || !focus_dists || !fd_strides) return fail(DFFW_EINVAL, "null argument");
    if (n_heads < 1 || n_heads > 4) return fail(DFFW_EINVAL, "n_heads must be 1..4, got %d", n_heads);
    if (B < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    for (int k = 0; k < n_heads; ++k) {
        if (!score[k] || !depth[k]) return fail(DFFW_EINVAL, "null argument (head %d)", k);
        if (h[k] < 1 || w[k] < 1) return fail(DFFW_EINVAL, "bad shape: head %d is %dx%d", k, h[k], w[k]);
    }
    return DFFW_OK;
}

int dffw_op_regress(int device, const float *score, int B, int N, int h, int w, int H, int W, const float *focus_dists,
                    const int64_t fd_strides[4], float *depth, void *hip_stream) {
    if (int rc = regress_check(1, &score, &h, &w, &depth, B, N, H, W, focus_dists, fd_strides)) return rc;
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(launch_regress(score, B, N, h, w, H, W, focus_dists, fd_strides[0], fd_strides[1], fd_strides[2], fd_strides[3], depth, s));
    HIPCHK(hipStreamSynchronize(s));
    return DFFW_OK;
}

int dffw_op_regress_heads(int device, int n_heads, const float *const score[4], const int h[4], const int w[4], float *const depth[4], int B, int N,
                          int H, int W, const float *focus_dists, const int64_t fd_strides[4], int fused, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = regress_check(n_heads, score, h, w, depth, B, N, H, W, focus_dists, fd_strides)) return rc;
    HIPCHK(hipSetDevice(device));
    RegressHeads hd{};   // as regress() / flush_regress queue the forward's heads
    hd.n = n_heads;
    hd.nofuse = fused ? 0 : 1;
    for (int k = 0; k < n_heads; ++k) {
        hd.score[k] = score[k];
        hd.depth[k] = depth[k];
        hd.h[k] = h[k];
        hd.w[k] = w[k];
    }
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(launch_regress_heads(hd, B, N, H, W, focus_dists, fd_strides[0], fd_strides[1], fd_strides[2], fd_strides[3], s));
    dffw_set_last_op_kernels(regress_kernel_name(hd, B, N, H, W));
    HIPCHK(hipStreamSynchronize(s));
    return DFFW_OK;
}

int dffw_op_fov_warp(int device, const float *x, int B, int C, int N, int H, int W, const float *alpha, const float *fovs,
                     int alpha_from_sample0, float *out, float *flow, void *hip_stream) {
    if (!x || !alpha || !fovs || !out) return fail(DFFW_EINVAL, "null argument");
    if (B < 1 || C < 1 || N < 1 || H < 1 || W < 1) return fail(DFFW_EINVAL, "bad shape");
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(launch_fov_warp(x, alpha, fovs, out, flow, B, C, N, H, W, alpha_from_sample0, s));
    HIPCHK(hipStreamSynchronize(s));
    return DFFW_OK;
}

// ---- training ops: the record-form ABIs (dffw_conv_wgrad, dffw_bn_train_*) between a stage-in and a stage-out.  Those calls set
// dffw_last_op_kernels() themselves; their bodies need an engine only for its precision.
int dffw_op_conv3d_backward(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *weight, int Cout,
                            const int kernel[3], const int stride[3], const int pad[3], int transposed, const float *grad_y, float *grad_x,
                            float *grad_w, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = conv_backward_check(precision, B, Cin, N, H, W, Cout, kernel, stride, pad, transposed)) return rc;
    if (!x || !grad_y || (grad_x && !weight)) return fail(DFFW_EINVAL, "null argument");
    // grad_y's shape follows from the geometry: the output volume of the forward
    const bool s2 = stride[1] == 2 && !transposed;
    const int Ho = transposed ? 2 * H : s2 ? H / 2 : H, Wo = transposed ? 2 * W : s2 ? W / 2 : W;
    const int one[3] = {1, 1, 1};
    if (grad_x) {   // the adjoint conv over grad_y (Cout -> Cin channels), through dffw_op_conv3d: pack_conv + Run::conv, the forward's kernel choice
        const int64_t taps = (int64_t)kernel[0] * 9;
        int rc;
        if (!transposed && !s2) {   // stride-1 conv of grad_y: filter flipped, in/out channels swapped, padding k - 1 - p (the same)
            rc = dffw_op_conv3d(device, precision, grad_y, B, Cout, N, Ho, Wo, adjoint_filter(weight, Cout, Cin, taps).data(), Cin, kernel, stride, pad, one, 0,
                                nullptr, nullptr, nullptr, 0, grad_x, hip_stream);
        } else {   // the stride-2 conv and the transposed conv are each other's adjoint, on the same filter
            rc = dffw_op_conv3d(device, precision, grad_y, B, Cout, N, Ho, Wo, weight, Cin, kernel, stride, pad, one, s2, nullptr, nullptr, nullptr, 0,
                                grad_x, hip_stream);
        }
        if (rc) return rc;
    }
    if (!grad_w) return DFFW_OK;
    const int64_t wsb = dffw_conv_wgrad_workspace_bytes(B, Cin, N, H, W, Cout, kernel, stride, pad, transposed);
    return run_wgrad_op(device, precision, B, N, {x, Cin, H, W}, {grad_y, Cout, Ho, Wo}, wsb, (hipStream_t)hip_stream,
                        [&](const void *xr, const void *yr, void *ws, hipStream_t s) {
                            return dffw_conv_wgrad(device, precision, xr, B, Cin, N, H, W, yr, Cout, kernel, stride, pad, transposed, grad_w, ws, wsb, s);
                        });
}

// ---- the 3x3x3 stride-1 conv over the concatenation of xa and xb: weight (Cout, Ca + Cb, 3,3,3) host fp32
int dffw_op_conv_cat_backward(int device, int precision, const float *xa, int Ca, const float *xb, int Cb, int B, int N, int H, int W, const float *weight,
                              int Cout, const float *grad_y, float *grad_xa, float *grad_xb, float *grad_w, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = conv_cat_backward_check(precision, B, Ca, Cb, N, H, W, Cout)) return rc;
    if (!xa || !xb || !grad_y || ((grad_xa || grad_xb) && !weight)) return fail(DFFW_EINVAL, "null argument");
    const int k3[3] = {3, 3, 3}, one[3] = {1, 1, 1};
    const int64_t taps = 27, plane = (int64_t)N * H * W;
    hipStream_t s = (hipStream_t)hip_stream;
    // grad_xa, grad_xb: the adjoint conv over grad_y (filter flipped, in / out channels swapped), through dffw_op_conv3d like every plain conv's.
    // The forward's dispatch picks its kernel, and with it the order of the fp32 sums, by the number of output channels too, so two convs of Ca
    // and Cb output channels need not give the bits of one of Ca + Cb.  Where that one exists (Ca + Cb <= 128) it is run, once, and its output
    // split: the halves of dffw_op_conv3d_backward's grad_x, bit for bit.  Beyond 128 channels no single conv is served: one per source, on the
    // weight's channels [0, Ca) and [Ca, Ca + Cb), each of at most 128 output channels
    const struct { float *out; int c0, C; } halves[2] = {{grad_xa, 0, Ca}, {grad_xb, Ca, Cb}};
    if ((grad_xa || grad_xb) && Ca + Cb <= 128) {
        HIPCHK(hipSetDevice(device));
        OpBlock gx(s);
        HIPCHK(gx.alloc(B * (Ca + Cb) * plane * (int64_t)sizeof(float)));
        if (int rc = dffw_op_conv3d(device, precision, grad_y, B, Cout, N, H, W, adjoint_filter(weight, Cout, Ca + Cb, taps).data(), Ca + Cb, k3, one, one, one, 0,
                                    nullptr, nullptr, nullptr, 0, (float *)gx.p, hip_stream))
            return rc;
        for (const auto &h : halves)   // (B, Ca + Cb, N, H, W) -> (B, C, N, H, W): one row of C * plane floats per sample
            if (h.out)
                HIPCHK(hipMemcpy2DAsync(h.out, h.C * plane * sizeof(float), (const float *)gx.p + h.c0 * plane, (Ca + Cb) * plane * sizeof(float),
                                        h.C * plane * sizeof(float), B, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    } else {
        for (const auto &h : halves) {
            if (!h.out) continue;
            std::vector<float> ws((size_t)Cout * h.C * taps);   // weight[:, c0 : c0 + C]
            for (int co = 0; co < Cout; ++co)
                std::copy(weight + ((size_t)co * (Ca + Cb) + h.c0) * taps, weight + ((size_t)co * (Ca + Cb) + h.c0 + h.C) * taps, ws.begin() + (size_t)co * h.C * taps);
            if (int rc = dffw_op_conv3d(device, precision, grad_y, B, Cout, N, H, W, adjoint_filter(ws.data(), Cout, h.C, taps).data(), h.C, k3, one, one, one, 0,
                                        nullptr, nullptr, nullptr, 0, h.out, hip_stream))
                return rc;
        }
    }
    if (!grad_w) return DFFW_OK;
    const int64_t wsb = dffw_conv_cat_wgrad_workspace_bytes(B, Ca, Cb, N, H, W, Cout);
    return run_wgrad_op(device, precision, B, N, {xa, Ca, H, W}, {xb, Cb, H, W}, {grad_y, Cout, H, W}, wsb, s,
                        [&](const void *ar, const void *br, const void *yr, void *ws, hipStream_t s) {
                            return dffw_conv_cat_wgrad(device, precision, ar, Ca, br, Cb, B, N, H, W, yr, Cout, grad_w, ws, wsb, s);
                        });
}

int dffw_op_bn_train(int device, int precision, const float *x, int B, int C, int N, int H, int W, const float *gamma, const float *beta, double eps,
                     double momentum, float *running_mean, float *running_var, const float *res, int relu, float *y, float *save_mean,
                     float *save_invstd, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = bn_train_check(precision, B, C, N, H, W)) return rc;
    if (!(eps > 0.0)) return fail(DFFW_EINVAL, "eps must be positive, got %g", eps);
    if (!x || !gamma || !beta || !y || !save_mean || !save_invstd) return fail(DFFW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(device));
    const int64_t wsb = dffw_bn_train_workspace_bytes(B, C, N, H, W);
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act xa = stage_in(r, x, B, C, N, H, W), ra = res ? stage_in(r, res, B, C, N, H, W) : Act();
        Act ya = r.act(B, N, H, W, C);
        void *ws = r.raw(wsb);
        if (real(r))
            r.err = dffw_bn_train_forward(device, precision, xa.p, B, C, N, H, W, gamma, beta, eps, momentum, running_mean, running_var, ra.p, relu, ya.p,
                                          save_mean, save_invstd, ws, wsb, r.s);
        stage_out(r, ya, y);
    });
}

int dffw_op_bn_train_backward(int device, int precision, const float *x, const float *y, const float *grad_y, int B, int C, int N, int H, int W,
                              const float *gamma, const float *save_mean, const float *save_invstd, int relu, float *grad_x, float *grad_res,
                              float *grad_gamma, float *grad_beta, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = bn_train_check(precision, B, C, N, H, W)) return rc;
    if (!x || !grad_y || !gamma || !save_mean || !save_invstd || !grad_gamma || !grad_beta) return fail(DFFW_EINVAL, "null argument");
    if (relu && !y) return fail(DFFW_EINVAL, "the ReLU mask is read from y: y may be NULL only without ReLU");
    if (grad_res && !grad_x) return fail(DFFW_EINVAL, "grad_res is written with grad_x");
    HIPCHK(hipSetDevice(device));
    const int64_t wsb = dffw_bn_train_workspace_bytes(B, C, N, H, W);
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act xa = stage_in(r, x, B, C, N, H, W), ya = relu ? stage_in(r, y, B, C, N, H, W) : Act(), ga = stage_in(r, grad_y, B, C, N, H, W);
        Act gx = grad_x ? r.act(B, N, H, W, C) : Act(), gr = grad_res ? r.act(B, N, H, W, C) : Act();
        void *ws = r.raw(wsb);
        if (real(r))
            r.err = dffw_bn_train_backward(device, precision, xa.p, ya.p, ga.p, B, C, N, H, W, gamma, save_mean, save_invstd, relu, gx.p, gr.p, grad_gamma,
                                           grad_beta, ws, wsb, r.s);
        if (grad_x) stage_out(r, gx, grad_x);
        if (grad_res) stage_out(r, gr, grad_res);
    });
}

// ---- the convs without in-plane taps: 3x1x1 p(1,0,0) and 1x1x1, stride 1
int dffw_op_conv_pw_backward(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *weight, int Cout,
                             const int kernel[3], const int pad[3], const float *grad_y, float *grad_x, float *grad_w, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = conv_pw_backward_check(precision, B, Cin, N, H, W, Cout, kernel, pad)) return rc;
    if (!x || !grad_y || (grad_x && !weight)) return fail(DFFW_EINVAL, "null argument");
    const int one[3] = {1, 1, 1};
    if (grad_x) {   // the adjoint conv over grad_y (Cout -> Cin channels): filter flipped along the slice axis, in/out channels swapped, the same padding
        const int rc = dffw_op_conv3d(device, precision, grad_y, B, Cout, N, H, W, adjoint_filter(weight, Cout, Cin, kernel[0]).data(), Cin, kernel, one, pad, one, 0,
                                      nullptr, nullptr, nullptr, 0, grad_x, hip_stream);
        if (rc) return rc;
    }
    if (!grad_w) return DFFW_OK;
    const int64_t wsb = dffw_conv_pw_wgrad_workspace_bytes(B, Cin, N, H, W, Cout, kernel, pad);
    return run_wgrad_op(device, precision, B, N, {x, Cin, H, W}, {grad_y, Cout, H, W}, wsb, (hipStream_t)hip_stream,
                        [&](const void *xr, const void *yr, void *ws, hipStream_t s) {
                            return dffw_conv_pw_wgrad(device, precision, xr, B, Cin, N, H, W, yr, Cout, kernel, pad, grad_w, ws, wsb, s);
                        });
}

int dffw_op_grad_combine(int device, int precision, const float *a, const float *y, const float *b, int B, int C, int N, int H, int W, float *out,
                         void *hip_stream) {
    dffw_set_last_op_kernels("");
    // the record form's refusals first: nothing is staged for a call it will not take (the pointers only say which operands there are)
    if (int rc = check_volume("grad_combine", precision, B, N, H, W, {C}, 1, (int64_t)B * N * H * W, "pixels")) return rc;
    if (!a || !out) return fail(DFFW_EINVAL, "null argument");
    if (!y && !b) return fail(DFFW_EINVAL, "grad_combine without a mask (y) and without a second gradient (b) is a copy: not an operation");
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act aa = stage_in(r, a, B, C, N, H, W), ya = y ? stage_in(r, y, B, C, N, H, W) : Act(), ba = b ? stage_in(r, b, B, C, N, H, W) : Act();
        Act oa = r.act(B, N, H, W, C);
        if (real(r)) r.err = dffw_grad_combine(device, precision, aa.p, ya.p, ba.p, B, C, N, H, W, oa.p, r.s);
        stage_out(r, oa, out);
    });
}

// ---- backward of the attention tail as one node: w3 and w1 are host fp32 and go to the device as they are
int dffw_op_att_tail_backward(int device, int precision, const float *x, const float *a, const float *t, const float *grad_y, int B, int C, int N, int H,
                              int W, const float *w3, const float *w1, float *grad_x, float *grad_w3, float *grad_w1, void *hip_stream) {
    dffw_set_last_op_kernels("");
    // the record form's refusals first: nothing is staged for a call it will not take
    if (int rc = att_tail_backward_check(precision, B, C, N, H, W)) return rc;
    if ((grad_w3 != nullptr) != (grad_w1 != nullptr)) return fail(DFFW_EINVAL, "grad_w3 and grad_w1 go together");
    if (!grad_x && !grad_w3) return DFFW_OK;
    if (!x || !a || !t || !grad_y || !w1 || (grad_x && !w3)) return fail(DFFW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(device));
    const int64_t wsb = grad_w3 ? dffw_att_tail_backward_workspace_bytes(B, C, N, H, W) : 0;
    const int64_t n1 = (int64_t)C * C, n3 = 3 * n1;
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act xa = stage_in(r, x, B, C, N, H, W), aa = stage_in(r, a, B, C, N, H, W), ta = stage_in(r, t, B, C, N, H, W), ga = stage_in(r, grad_y, B, C, N, H, W);
        Act gx = grad_x ? r.act(B, N, H, W, C) : Act();
        float *w1d = (float *)r.raw(n1 * sizeof(float)), *w3d = w3 ? (float *)r.raw(n3 * sizeof(float)) : nullptr;
        void *ws = wsb ? r.raw(wsb) : nullptr;
        if (real(r)) {
            r.check(hipMemcpyAsync(w1d, w1, n1 * sizeof(float), hipMemcpyHostToDevice, r.s), "copy");
            if (w3d && r.ok()) r.check(hipMemcpyAsync(w3d, w3, n3 * sizeof(float), hipMemcpyHostToDevice, r.s), "copy");
            if (r.ok())
                r.err = dffw_att_tail_backward(device, precision, xa.p, aa.p, ta.p, ga.p, B, C, N, H, W, w3d, w1d, gx.p, grad_w3, grad_w1, ws, wsb, r.s);
        }
        if (grad_x) stage_out(r, gx, grad_x);
    });
}

// ---- backward of the pools: H and W are the pools' input resolution, g / g2 / g4 / g8 have the pooled shapes
int dffw_op_pool_backward(int device, int precision, int mode, int k, const float *g, const float *x, const float *b, int B, int C, int N, int H, int W,
                          float *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    // the record form's refusals first: nothing is staged for a call it will not take
    if (int rc = pool_backward_check(precision, mode, k, x != nullptr, B, C, N, H, W)) return rc;
    if (!g || !out) return fail(DFFW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act ga = stage_in(r, g, B, C, N, H / k, W / k), xa = x && mode == POOL_MAX ? stage_in(r, x, B, C, N, H, W) : Act();
        Act ba = b ? stage_in(r, b, B, C, N, H, W) : Act(), oa = r.act(B, N, H, W, C);
        if (real(r)) r.err = dffw_pool_backward(device, precision, mode, k, ga.p, xa.p, ba.p, B, C, N, H, W, oa.p, r.s);
        stage_out(r, oa, out);
    });
}

int dffw_op_pool3_backward(int device, int precision, const float *g2, const float *g4, const float *g8, const float *b, int B, int C, int N, int H, int W,
                           float *out, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = pool3_backward_check(precision, B, C, N, H, W)) return rc;
    if (!g2 || !g4 || !g8) return fail(DFFW_EINVAL, "the pyramid backward needs all of g2, g4 and g8");
    if (!out) return fail(DFFW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(device));
    OpEngine eng(device, precision);
    return run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
        Act a2 = stage_in(r, g2, B, C, N, H / 2, W / 2), a4 = stage_in(r, g4, B, C, N, H / 4, W / 4), a8 = stage_in(r, g8, B, C, N, H / 8, W / 8);
        Act ba = b ? stage_in(r, b, B, C, N, H, W) : Act(), oa = r.act(B, N, H, W, C);
        if (real(r)) r.err = dffw_pool3_backward(device, precision, a2.p, a4.p, a8.p, ba.p, B, C, N, H, W, oa.p, r.s);
        stage_out(r, oa, out);
    });
}

// ---- backward of the stem: the weight gradient only, x is the image stack and stays fp32
int dffw_op_stem_backward(int device, int precision, const float *x, const float *grad_y, int B, int N, int H, int W, float *grad_w, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (int rc = stem_backward_check(precision, B, N, H, W)) return rc;
    if (!x || !grad_y || !grad_w) return fail(DFFW_EINVAL, "null argument");
    const int64_t wsb = dffw_stem_wgrad_workspace_bytes(B, N, H, W);
    return run_wgrad_op(device, precision, B, N, {}, {grad_y, stemw::CO, H, W}, wsb, (hipStream_t)hip_stream,
                        [&](const void *, const void *yr, void *ws, hipStream_t s) { return dffw_stem_wgrad(device, precision, x, yr, B, N, H, W, grad_w, ws, wsb, s); });
}

// ---- backward of the score convs, Cin -> 1: grad_score stays fp32 planar, weight is device fp32; x and b become records
int dffw_op_score_conv_backward(int device, int precision, const float *x, int B, int Cin, int N, int h, int w, const float *weight, const int kernel[3],
                                const int pad[3], const float *grad_score, const float *b, float *grad_x, float *grad_w, void *hip_stream) {
    dffw_set_last_op_kernels("");
    // the record forms' refusals first: nothing is staged for a call they will not take
    if (int rc = score_conv_backward_check(precision, B, Cin, N, h, w, kernel, pad)) return rc;
    if (!grad_score || (grad_x && !weight) || (grad_w && !x)) return fail(DFFW_EINVAL, "null argument");
    if (b && !grad_x) return fail(DFFW_EINVAL, "b is added to grad_x: it needs grad_x");
    if (!grad_x && !grad_w) return DFFW_OK;
    HIPCHK(hipSetDevice(device));
    std::string names;   // of both halves, data gradient first
    int rc = DFFW_OK;
    if (grad_x) {
        OpEngine eng(device, precision);
        rc = run_op(eng, (hipStream_t)hip_stream, false, [&](Run &r) {
            Act ba = b ? stage_in(r, b, B, Cin, N, h, w) : Act(), oa = r.act(B, N, h, w, Cin);
            if (real(r)) r.err = dffw_score_conv_dgrad(device, precision, grad_score, B, Cin, N, h, w, weight, kernel, pad, ba.p, oa.p, r.s);
            stage_out(r, oa, grad_x);
        });
        names = dffw_last_op_kernels();
    }
    if (grad_w && rc == DFFW_OK) {
        const int64_t wsb = dffw_score_conv_wgrad_workspace_bytes(B, Cin, N, h, w, kernel, pad);
        rc = run_wgrad_op(device, precision, B, N, {x, Cin, h, w}, {}, wsb, (hipStream_t)hip_stream, [&](const void *xr, const void *, void *ws, hipStream_t s) {
            return dffw_score_conv_wgrad(device, precision, xr, grad_score, B, Cin, N, h, w, kernel, pad, grad_w, ws, wsb, s);
        });
        names += (names.empty() ? "" : ";") + std::string(dffw_last_op_kernels());
    }
    dffw_set_last_op_kernels(rc == DFFW_OK ? names.c_str() : "");
    return rc;
}

}  // extern "C"
