// Host side of libdffw.so: the layer table (weight contract), BatchNorm folding + MFMA-fragment
// weight packing, the static workspace arena and the whole-graph executor of DFF_net.forward
// (reference Depth_Estimation_Test/Depth_Estimation_Network.py:74-127), behind the C ABI of include/dffw.h.
// The End_to_End variant (End_to_End/End_to_End.py: alignment network + FOV warp in front of the same DFF_net)
// is dffw_align.cpp.  All arithmetic of the forward runs in the gfx950 kernels; nothing here touches activation values.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "dffw_repack.h"
#include "dffw_run.h"
#include "dffw_srd_roll.h"
#include "dffw_stem.h"

namespace dffw {

// ---- errors ------------------------------------------------------------------------------------
static thread_local std::string g_err;
static thread_local std::string g_last_kernel;   // dffw_last_conv_kernel()
static thread_local std::string g_last_op_kernels;   // dffw_last_op_kernels()
}  // namespace dffw
int dffw_fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    dffw::g_err = buf;
    return code;
}
void dffw_set_last_op_kernels(const char *names) { dffw::g_last_op_kernels = names ? names : ""; }
void dffw_set_last_conv_kernel(const char *name) { dffw::g_last_kernel = name; }
namespace dffw {

// ---- layer table -------------------------------------------------------------------------------
struct ParamInfo {
    std::string name;
    int64_t shape[5];
    int ndim;
    int flags;  // bit0 buffer, bit1 int64 counter, bit2 dead
};

class Table {
  public:
    std::vector<LayerDef> layers;
    std::vector<ParamInfo> params;
    std::map<std::string, int> by_name;

    void conv(const std::string &key, int cin, int cout, int kd, int kh, int kw, int s, int pd, int ph, int pw, int dil,
              bool bn, bool live = true) {
        // `key` is the prefix of a reference convbn_3d pair when bn (conv = key.0, BatchNorm = key.1,
        // DEN.py:286-289), else the conv's own prefix
        LayerDef L{bn ? key + ".0" : key, bn ? key + ".1" : "", cin, cout, kd, kh, kw, s, s, pd, ph, pw, dil, dil, false, live, false};
        add(L);
    }
    void deconv(const std::string &key, int cin, int cout) {
        LayerDef L{key + ".0", key + ".1", cin, cout, 3, 3, 3, 2, 2, 1, 1, 1, 1, 1, true, true, false};
        add(L);
    }
    void c3(const std::string &key, int cin, int cout, int s = 1, bool bn = true) { conv(key, cin, cout, 3, 3, 3, s, 1, 1, 1, 1, bn); }

    void srd(const std::string &p, int c) {  // DEN.py:295-330
        conv(p + ".Focus_Measure.conv.0", c, c, 1, 3, 3, 1, 0, 1, 1, 1, true);
        conv(p + ".Focus_Measure.conv.2", c, c, 1, 3, 3, 1, 0, 1, 1, 1, true);
        conv(p + ".N_ch_attention.0", c, c, 3, 1, 1, 1, 1, 0, 0, 1, false);
        conv(p + ".N_ch_attention.2", c, c, 1, 1, 1, 1, 0, 0, 0, 1, false);
    }
    void efd(const std::string &p, int cin, int cout) {  // DEN.py:306-315
        c3(p + ".stride_conv", cin, cout, 2);
        c3(p + ".max_pooling.1", cin, cout, 1);
    }
    void hourglass(const std::string &p, int c) {  // DEN.py:240-264
        c3(p + ".conv0.0", 2 * c, c);
        c3(p + ".conv1.0", c, 2 * c, 2);
        conv(p + ".pre_conv.0", 2 * c, 2 * c, 1, 1, 1, 1, 0, 0, 0, 1, true, /*live=*/false);
        c3(p + ".conv2", 2 * c, 2 * c);
        c3(p + ".conv3.0", 2 * c, 2 * c, 2);
        c3(p + ".conv4.0", 2 * c, 2 * c);
        deconv(p + ".conv5", 2 * c, 2 * c);
        deconv(p + ".conv6", 2 * c, c);
    }

    void biased(const std::string &key, int cin, int cout, int kd, int kh, int kw, int pd, int ph, int pw) {
        LayerDef L{key, "", cin, cout, kd, kh, kw, 1, 1, pd, ph, pw, 1, 1, false, true, true};
        add(L);
    }
    void of_block(const std::string &p, int cin, int cout, int s) {  // resnet_block_2d_OF, End_to_End.py:135-145
        conv(p + ".conv.0", cin, cout, 1, 3, 3, s, 0, 1, 1, 1, true);
        conv(p + ".conv.2", cout, cout, 1, 3, 3, 1, 0, 1, 1, 1, true);
        conv(p + ".feature", cin, cout, 1, 1, 1, s, 0, 0, 0, 1, false);
        if (s == 1) {   // same resolution on both branches: the shortcut rides in conv.2's contraction
            layers[by_name[p + ".conv.2.0"]].shortcut = p + ".feature";
            layers[by_name[p + ".feature"]].folded = true;
        }
    }
    void alpha_head(const std::string &p, int cin, int c) {  // conv1/conv2/conv3 of FlowNetwork, End_to_End.py:37-69
        conv(p + ".0", cin, c, 1, 3, 3, 1, 0, 1, 1, 1, true);
        layers[by_name[p + ".0.0"]].head_split = (cin - 2) / 2;
        conv(p + ".2", c, c, 1, 3, 3, 1, 0, 1, 1, 1, true);
        conv(p + ".4", c, c, 1, 3, 3, 1, 0, 1, 1, 1, true);
        biased(p + ".6", c, 3, 1, 3, 3, 0, 1, 1);
    }

    // End_to_End.Network (End_to_End.py:9-12): DFF_net registered first, then optical_flow_aggregation = FlowNetwork(8)
    static Table e2e_net() {
        Table t = depth_net();
        const std::string P = "optical_flow_aggregation";
        const int C = 8;
        t.of_block(P + ".OF_feature.0", 3, C, 1);
        t.of_block(P + ".OF_feature.1", C, C, 1);
        t.of_block(P + ".OF_feature1.0", C, 2 * C, 2);
        t.of_block(P + ".OF_feature1.1", 2 * C, 2 * C, 1);
        t.of_block(P + ".OF_feature2.0", 2 * C, 4 * C, 2);
        t.of_block(P + ".OF_feature2.1", 4 * C, 4 * C, 1);
        t.alpha_head(P + ".conv1", 8 * C + 2, 8 * C);
        t.alpha_head(P + ".conv2", 4 * C + 2, 4 * C);
        t.alpha_head(P + ".conv3", 2 * C + 2, 2 * C);
        return t;
    }

    static Table depth_net() {
        Table t;
        const std::string P = "DFF_net";
        t.conv(P + ".FM_measure.Focus_extraction.0", 3, 8, 1, 9, 9, 1, 0, 8, 8, 2, true);  // DEN.py:135
        t.srd(P + ".FM_measure.Focus_extraction.2", 8);
        t.efd(P + ".FM_conv1.0", 8, 16);
        t.srd(P + ".FM_conv1.1", 16);
        t.efd(P + ".FM_conv2.0", 16, 32);
        t.srd(P + ".FM_conv2.1", 32);
        const std::string S = P + ".SPP_module";  // DEN.py:145-210
        const char *scales[3] = {"8", "16", "32"};
        const int widths[3] = {32, 64, 64};
        for (int i = 0; i < 3; ++i) {
            const std::string d = S + ".dres" + scales[i];
            t.c3(d + "_0.0", 32, widths[i]);
            t.c3(d + "_0.2", widths[i], widths[i]);
            t.c3(d + "_1.0", widths[i], widths[i]);
            t.c3(d + "_1.2", widths[i], widths[i]);
        }
        t.c3(S + ".conv1", 32, 64, 2, false);
        t.c3(S + ".conv2.0", 64, 64);
        t.c3(S + ".conv3", 64, 128, 2, false);
        t.c3(S + ".conv4.0", 128, 128);
        t.deconv(S + ".conv8", 128, 64);
        t.deconv(S + ".conv9", 64, 32);
        t.c3(S + ".combine1.0", 128, 64);
        t.c3(S + ".combine2.0", 192, 128);
        t.conv(S + ".redir1", 32, 32, 1, 1, 1, 1, 0, 0, 0, 1, true);
        t.conv(S + ".redir2", 64, 64, 1, 1, 1, 1, 0, 0, 0, 1, true);
        t.conv(S + ".redir3", 128, 128, 1, 1, 1, 1, 0, 0, 0, 1, true, /*live=*/false);
        t.c3(P + ".confidence.0", 32, 32);
        t.c3(P + ".confidence.2", 32, 1, 1, false);
        t.c3(P + ".dres0.0", 32, 64);
        t.c3(P + ".dres0.2", 64, 64);
        t.deconv(P + ".deconv_1", 64, 32);
        t.hourglass(P + ".dres2", 32);
        t.deconv(P + ".deconv_2", 32, 16);
        t.hourglass(P + ".dres3", 16);
        t.deconv(P + ".deconv_3", 16, 8);
        t.hourglass(P + ".dres4", 8);
        t.conv(P + ".classif1.0", 32, 1, 1, 1, 1, 1, 0, 0, 0, 1, false);
        t.conv(P + ".classif2.0", 16, 1, 1, 1, 1, 1, 0, 0, 0, 1, false);
        t.conv(P + ".classif3.0", 8, 1, 1, 1, 1, 1, 0, 0, 0, 1, false);
        return t;
    }

  private:
    void add(const LayerDef &L) {
        by_name[L.conv] = (int)layers.size();
        layers.push_back(L);
        const int dead = L.live ? 0 : 4;
        ParamInfo w{L.conv + ".weight", {0, 0, 0, 0, 0}, 5, dead};
        w.shape[0] = L.transposed ? L.cin : L.cout;
        w.shape[1] = L.transposed ? L.cout : L.cin;
        w.shape[2] = L.kd;
        w.shape[3] = L.kh;
        w.shape[4] = L.kw;
        params.push_back(w);
        if (L.bias) params.push_back(ParamInfo{L.conv + ".bias", {L.cout, 0, 0, 0, 0}, 1, dead});
        if (!L.bn.empty()) {
            params.push_back(ParamInfo{L.bn + ".weight", {L.cout, 0, 0, 0, 0}, 1, dead});
            params.push_back(ParamInfo{L.bn + ".bias", {L.cout, 0, 0, 0, 0}, 1, dead});
            params.push_back(ParamInfo{L.bn + ".running_mean", {L.cout, 0, 0, 0, 0}, 1, dead | 1});
            params.push_back(ParamInfo{L.bn + ".running_var", {L.cout, 0, 0, 0, 0}, 1, dead | 1});
            params.push_back(ParamInfo{L.bn + ".num_batches_tracked", {0, 0, 0, 0, 0}, 0, dead | 3});
        }
    }
};

static bool known_net(int net) { return net == DFFW_NET_DEPTH || net == DFFW_NET_E2E; }
static const Table &table_for(int net) {
    static const Table depth = Table::depth_net();
    static const Table e2e = Table::e2e_net();
    return net == DFFW_NET_E2E ? e2e : depth;
}

const std::vector<LayerDef> &net_layers(int net) { return table_for(net).layers; }   // (dffw_repack.cpp)

// the layers of one block as the table defines them (the single-operator entry points of dffw_ops.cpp pack them under the forward's names)
std::vector<LayerDef> srd_layers(const std::string &p, int c) { Table t; t.srd(p, c); return t.layers; }
std::vector<LayerDef> efd_layers(const std::string &p, int cin, int cout) { Table t; t.efd(p, cin, cout); return t.layers; }
std::vector<LayerDef> of_block_layers(const std::string &p, int cin, int cout, int s) { Table t; t.of_block(p, cin, cout, s); return t.layers; }
std::vector<LayerDef> alpha_head_layers(const std::string &p, int cin, int c) { Table t; t.alpha_head(p, cin, c); return t.layers; }

}  // namespace dffw

using namespace dffw;

namespace dffw {

#ifdef DFFW_TRACE_BUILD
constexpr size_t SRD_TRACE_WORDS = Run::STEP_TRACE_WORDS;
#else
constexpr size_t SRD_TRACE_WORDS = 0;   // (the production srd kernels write no step timeline)
#endif

// SRD block (DEN.py:317-330): x -> feat = relu(x + BN(conv(relu(BN(conv x))))) ; feat + relu(conv1(relu(conv3x1x1 feat)))
// pooled (optional): receives max_pool(1,2,2) of the block's output when the fused attention kernel can produce it
// on the way (else it is left empty and the caller pools separately).
Act srd(Run &r, const std::string &p, Act &x, bool drop_x, Act *pooled) {
    // the 8- / 16-channel block on whole 8 x 16 / 4 x 16 columns: one fused persistent kernel (dffw_srd_roll.hip)
    {
        auto c0 = r.e->convs.find(p + ".Focus_Measure.conv.0.0"), c2 = r.e->convs.find(p + ".Focus_Measure.conv.2.0");
        auto a3 = r.e->convs.find(p + ".N_ch_attention.0"), a1 = r.e->convs.find(p + ".N_ch_attention.2");
        int sty, stx;
        if (x.C == 16) srd_roll16_tile(&sty, &stx);
        else srd_roll_tile(&sty, &stx);
        const auto end = r.e->convs.end();
        if ((x.C == 8 || x.C == 16) && c0 != end && c2 != end && a3 != end && a1 != end &&
            c0->second.wsrd && c2->second.wsrd && a3->second.w32 &&
            a1->second.w32 && a3->second.watt && a1->second.watt && a3->second.def.kd == 3 && a1->second.def.kd == 1 &&
            x.H % sty == 0 && x.W % stx == 0 && x.H % 2 == 0 && (int64_t)x.B * (x.H / sty) * (x.W / stx) >= r.sw.roll_min_units &&
            !r.sw.on(SW_NO_FUSED_SRD) && !r.sw.on(SW_NO_FUSED_ATTENTION) && !r.sw.on(SW_NO_TILE)) {
            Act out = r.act(x.B, x.N, x.H, x.W, x.C);
            const bool with_pool = pooled && !r.sw.on(SW_NO_FUSED_POOL);
            if (with_pool) *pooled = r.act(x.B, x.N, x.H / 2, x.W / 2, x.C);
            if (r.ok() && !r.dry) {
                SrdArgs a = srd_args(x.p, out.p, c0->second, c2->second, x.B, x.N, x.H, x.W, sty, stx, r.sw.srd_wgs);
                if (!(a.zero = r.zero_page())) return out;
                a.pooled = with_pool ? pooled->p : nullptr;
                a.w3 = a3->second.w32; a.w1 = a1->second.w32;
                a.w3f = a3->second.watt; a.w1f = a1->second.watt;
                char kn[64];
                const bool pipe16 = x.C == 16 && r.sw.srd_pipe;   // (opt-in: measured 6 % slower than srd_roll16, profiles/r06_srd_two_slice.txt)
                if (pipe16) srd_pipe16_kernel_name(r.e->prec, with_pool, kn, sizeof kn);
                else if (x.C == 16) srd_roll16_kernel_name(r.e->prec, with_pool, kn, sizeof kn);
                else srd_roll_kernel_name(r.e->prec, with_pool, kn, sizeof kn);
                const double px = (double)x.pixels();
                // algorithmic: two 1x3x3 C -> C convs + the 3x1x1 and 1x1x1 attention convs; x read once, out (+ pooled) written once
                r.launch(kn, p, "", 2.0 * px * (2 * 9 + 4) * x.C * x.C, (with_pool ? 2.25 : 2.0) * px * x.C * r.elem_bytes(), "srd_roll", SRD_TRACE_WORDS, [&](unsigned long long *trace) {
#ifdef DFFW_TRACE_BUILD
                    a.trace = trace;
#endif
                    return pipe16 ? launch_srd_pipe16(r.e->prec, a, r.s) : x.C == 16 ? launch_srd_roll16(r.e->prec, a, r.s) : launch_srd_roll(r.e->prec, a, r.s);
                });
                r.trace_end();
            }
            if (drop_x) r.drop(x);
            return out;
        }
    }
    ConvOpt o1; o1.relu = 1;
    Act t = r.conv(p + ".Focus_Measure.conv.0.0", x, o1);
    ConvOpt o2; o2.relu = 1; o2.res0 = &x;
    Act feat = r.conv(p + ".Focus_Measure.conv.2.0", t, o2);
    r.drop(t);
    if (drop_x) r.drop(x);
    Act out;
    auto i3 = r.e->convs.find(p + ".N_ch_attention.0");
    auto i1 = r.e->convs.find(p + ".N_ch_attention.2");
    if (srd_attention_supported(feat.C) && i3 != r.e->convs.end() && i1 != r.e->convs.end() && i3->second.w32 && i1->second.w32 &&
        !r.sw.on(SW_NO_FUSED_ATTENTION)) {
        out = r.act(feat.B, feat.N, feat.H, feat.W, feat.C);
        const bool with_pool = pooled && !r.sw.on(SW_NO_FUSED_POOL);
        if (with_pool) *pooled = r.act(feat.B, feat.N, feat.H / 2, feat.W / 2, feat.C);
        if (r.ok() && !r.dry) {
            char kn[64];
            snprintf(kn, sizeof kn, "dffw::srd_attention_kernel<%d, %d>", r.e->prec, feat.C);
            const double px = (double)feat.pixels();
            r.launch_unnamed(kn, p, ".N_ch_attention", 2.0 * px * 4 * feat.C * feat.C, (with_pool ? 2.25 : 2.0) * px * feat.C * r.elem_bytes(), "srd_attention", 0, [&](unsigned long long *) {
                return launch_srd_attention(r.e->prec, feat.p, out.p, i3->second.w32, i1->second.w32, feat.B, feat.N, feat.H, feat.W, feat.C, with_pool ? pooled->p : nullptr, r.s);
            });
        }
    } else if (feat.C == 32 && i3 != r.e->convs.end() && i1 != r.e->convs.end() && i3->second.watt && i1->second.watt && feat.W % 16 == 0 &&
               !r.sw.on(SW_NO_FUSED_ATTENTION)) {
        out = r.act(feat.B, feat.N, feat.H, feat.W, feat.C);
        if (r.ok() && !r.dry) {
            char kn[64];
            snprintf(kn, sizeof kn, "dffw::srd_attention_mfma<%d>", r.e->prec);
            const double px = (double)feat.pixels();
            r.launch_unnamed(kn, p, ".N_ch_attention", 2.0 * px * 4 * feat.C * feat.C, 2.0 * px * feat.C * r.elem_bytes(), "srd_attention_mfma", 0, [&](unsigned long long *) {
                return launch_srd_attention_mfma(r.e->prec, feat.p, out.p, i3->second.watt, i1->second.watt, feat.B, feat.N, feat.H, feat.W, r.s);
            });
        }
    } else {
        ConvOpt o3; o3.relu = 1;
        Act a = r.conv(p + ".N_ch_attention.0", feat, o3);
        ConvOpt o4; o4.relu = 2; o4.res0 = &feat;
        out = r.conv(p + ".N_ch_attention.2", a, o4);
        r.drop(a);
    }
    r.drop(feat);
    return out;
}

// EFD block (DEN.py:306-315)
Act efd(Run &r, const std::string &p, const Act &x, Act *pooled) {
    auto ca = r.e->convs.find(p + ".stride_conv.0"), cb = r.e->convs.find(p + ".max_pooling.1.0");
    const int Ho = x.H / 2, Wo = x.W / 2;
    const double opx = (double)x.B * x.N * Ho * Wo;
    // a fused block serves the shape: its pooled input is at hand, both layers are packed, whole ty x tx columns of the output grid that fill the chip
    auto fused = [&](int C, int ty, int tx) {
        return x.C == C && pooled && pooled->p && ca != r.e->convs.end() && cb != r.e->convs.end() && x.H % 2 == 0 && x.W % 2 == 0 && Ho % ty == 0 && Wo % tx == 0 &&
               (int64_t)x.B * (Ho / ty) * (Wo / tx) >= r.sw.roll_min_units && !r.sw.on(SW_NO_ROLL) && !r.sw.on(SW_NO_FUSED_EFD) && !r.sw.on(SW_NO_TILE);
    };
    auto args = [&](int cout, uint16_t *out) {   // a.in0 = x, a.in1 = its (1,2,2) max-pool
        ConvArgs a;
        memset(&a, 0, sizeof a);
        a.in0 = x.p; a.C0 = x.C;
        a.in1 = pooled->p; a.C1 = x.C;
        a.B = x.B; a.Ni = x.N; a.Hi = x.H; a.Wi = x.W;
        a.Ng = x.N; a.Hg = Ho; a.Wg = Wo;
        a.No = x.N; a.Ho = Ho; a.Wo = Wo;
        a.Cout = cout;
        a.bias = ca->second.bias;
        a.out = out;
        a.relu = 1;
        a.M = (int64_t)x.B * x.N * Ho * Wo;
        return a;
    };
    int ty, tx;
    // the 8 -> 16 channel block with its pooled input at hand: both branches in one rolling kernel (conv_roll_efd)
    efd_roll_tile(&ty, &tx);
    if (fused(8, ty, tx) && ca->second.wroll8 && cb->second.wroll8) {
        Act out = r.act(x.B, x.N, Ho, Wo, 16);
        if (r.ok() && !r.dry) {
            ConvArgs a = args(16, out.p);
            if (!(a.zero = r.zero_page())) return out;
            a.dbg = (r.sw.debug_flags & 6) | r.sw.path_bits();
            RollArgs t = roll_args(ca->second.wroll8, x.B, Ho / ty, Wo / tx, 1, r.sw.roll_wgs);
            t.wroll2 = cb->second.wroll8;
            t.bias2 = cb->second.bias;
            char kn[64];
            conv_roll_efd_kernel_name(r.e->prec, a, true, kn, sizeof kn);
            r.launch(kn, p, "", 2.0 * opx * 27.0 * 8 * 16 * 2, ((double)x.pixels() * 8 + opx * 8 + opx * 16) * r.elem_bytes(), "conv_roll_efd", 0,
                     [&](unsigned long long *) { return launch_conv_roll_efd(r.e->prec, a, t, r.s); });
        }
        r.drop(*pooled);
        return out;
    }
    // the 16 -> 32 channel block (`FM_conv2.0`): both branches in one streaming kernel, the waves split by branch / output tile / pixel half (conv_efd16)
    efd16_tile(&ty, &tx);
    if (fused(16, ty, tx) && ca->second.wroll_s2 && cb->second.wroll15 && ca->second.def.cout == 32) {
        ConvArgs a = args(32, (uint16_t *)16);   // (a placeholder output for the check below: the output is allocated once the kernel is known to serve the shape)
        RollArgs t = roll_args(ca->second.wroll_s2, x.B, Ho / ty, Wo / tx, 1, r.sw.roll_wgs);
        t.wroll2 = cb->second.wroll15;
        t.bias2 = cb->second.bias;
        if (efd16_ok(r.e->prec, a, t)) {
            Act out = r.act(x.B, x.N, Ho, Wo, 32);
            if (r.ok() && !r.dry) {
                a.out = out.p;
                char kn[64];
                conv_efd16_kernel_name(kn, sizeof kn);
                r.launch(kn, p, "", 2.0 * opx * 27.0 * 16 * 32 * 2, ((double)x.pixels() * 16 + opx * 16 + opx * 32) * r.elem_bytes(), "conv_efd16", 0,
                         [&](unsigned long long *) { return launch_conv_efd16(a, t, r.s); });
            }
            r.drop(*pooled);
            return out;
        }
    }
    Act a = r.conv(p + ".stride_conv.0", x);
    Act m = (pooled && pooled->p) ? *pooled : r.pool(x, 0, 2);
    ConvOpt o; o.relu = 1; o.res0 = &a;
    Act out = r.conv(p + ".max_pooling.1.0", m, o);
    r.drop(m);
    r.drop(a);
    return out;
}

// one scale of the pyramid: r0 = dresX_0(t) ; dresX_1(r0) + r0   (DEN.py:216-223)
static Act pyramid_scale(Run &r, const std::string &S, const char *tag, Act &t) {
    const std::string d = S + ".dres" + tag;
    ConvOpt rl; rl.relu = 1;
    Act a = r.conv(d + "_0.0.0", t, rl);
    Act r0 = r.conv(d + "_0.2.0", a, rl);
    r.drop(a);
    Act b = r.conv(d + "_1.0.0", r0, rl);
    ConvOpt o; o.res0 = &r0;
    Act out = r.conv(d + "_1.2.0", b, o);
    r.drop(b);
    r.drop(r0);
    return out;
}

// hourglassup.forward (DEN.py:212-238)
static Act pyramid(Run &r, const std::string &S, const Act &v3) {
    ConvOpt rl; rl.relu = 1;
    Act p8, p16, p32;
    if (v3.H % 8 == 0 && v3.W % 8 == 0 && !r.sw.on(SW_NO_POOL3)) {   // one pass over v3 for the three pyramid scales (pool3_kernel)
        r.pool3(v3, p8, p16, p32);
    } else {
        p8 = r.pool(v3, 1, 2);
        p16 = r.pool(v3, 1, 4);
        p32 = r.pool(v3, 1, 8);
    }
    // the three scales are independent chains of 4 convs (DEN.py:216-223): side by side when concurrency is on
    r.forked = r.concurrent;
    // (one hipEventRecord per side stream: with ONE event that both side streams wait for the batch-1 forward is 80 us SLOWER, 0.877 -> 0.958 ms; and
    // chaining the joins -- side 1 waits for side 0, the main stream for side 1 -- costs as much: profiles/r06_batch1_teams.txt)
    r.fork(0);
    r.fork(1);
    Act s8 = pyramid_scale(r, S, "8", p8);
    r.drop(p8);
    r.on(0);
    Act s16 = pyramid_scale(r, S, "16", p16);
    r.drop(p16);
    r.on(1);
    Act s32 = pyramid_scale(r, S, "32", p32);
    r.drop(p32);
    r.on(-1);
    r.join(0);
    r.join(1);
    r.forked = false;
    r.release_deferred();
    // redir1 / redir2 (1x1x1 conv + BN of x_8 / of conv2's output, DEN.py:209-210,234-237) only feed the residual inputs of conv9 / conv8: they run on the
    // side streams next to the chain conv1 ... conv4 instead of between its launches (two small gather-GEMM launches off the critical path)
    // (below 2M stack pixels -- batch 1 and 2 of 10x256x256 -- in line: a fork and a join hold the main queue for ~6 us each, the launch itself is 7-9 us:
    // 0.877 -> 0.870 ms at batch 1, 1.122 -> 1.118 at batch 2; from batch 4 up the side streams win by 0.3-0.7 %)
    const bool redir_side = r.concurrent && (r.sw.redir_side == 1 || (r.sw.redir_side < 0 && (int64_t)v3.B * v3.N * v3.H * v3.W * 16 >= (2 << 20)));
    r.forked = redir_side;
    if (redir_side) {
        r.fork(0);
        r.on(0);
    }
    Act rd1 = r.conv(S + ".redir1.0", s8);
    r.on(-1);
    Act d1 = r.conv(S + ".conv1", s8);
    r.drop(s8);
    ConvOpt c1 = rl; c1.in1 = &s16;
    Act m1 = r.conv(S + ".combine1.0.0", d1, c1);
    r.drop(d1); r.drop(s16);
    Act c2 = r.conv(S + ".conv2.0.0", m1, rl);
    r.drop(m1);
    if (redir_side) {
        r.fork(1);
        r.on(1);
    }
    Act rd2 = r.conv(S + ".redir2.0", c2);
    r.on(-1);
    Act d2 = r.conv(S + ".conv3", c2);
    r.drop(c2);
    ConvOpt cc2 = rl; cc2.in1 = &s32;
    Act m2 = r.conv(S + ".combine2.0.0", d2, cc2);
    r.drop(d2); r.drop(s32);
    Act c4 = r.conv(S + ".conv4.0.0", m2, rl);
    r.drop(m2);
    if (redir_side) r.join(1);
    ConvOpt u8o = rl; u8o.res0 = &rd2;
    Act u8 = r.conv(S + ".conv8.0", c4, u8o);
    r.drop(c4); r.drop(rd2);
    if (redir_side) r.join(0);
    ConvOpt u9o = rl; u9o.res0 = &rd1;
    Act u9 = r.conv(S + ".conv9.0", u8, u9o);
    r.drop(u8); r.drop(rd1);
    r.forked = false;
    r.release_deferred();
    return u9;
}

// hourglass.forward (DEN.py:265-284).  x = cat[xa, xb] on channels.  Returns conv6's output `out`
// in *out_raw (if wanted) and out + skip in the return value; pre1 = conv0's output.
static Act hourglass(Run &r, const std::string &p, const Act &xa, const Act &xb, const Act *presqu, const Act *postsqu,
                     const Act &skip, Act *pre1_out, Act *out_raw, const std::string &cls, float *cls_out, bool discard_sum) {
    ConvOpt rl; rl.relu = 1;
    ConvOpt c0 = rl; c0.in1 = &xb;
    Act pre1 = r.conv(p + ".conv0.0.0", xa, c0);
    Act o1 = r.conv(p + ".conv1.0.0", pre1, rl);
    ConvOpt c2 = rl; c2.res0 = postsqu;
    Act pre = r.conv(p + ".conv2.0", o1, c2);
    r.drop(o1);
    Act o3 = r.conv(p + ".conv3.0.0", pre, rl);
    Act o4 = r.conv(p + ".conv4.0.0", o3, rl);
    r.drop(o3);
    ConvOpt c5 = rl; c5.res0 = presqu ? presqu : &pre;
    Act o5 = r.conv(p + ".conv5.0", o4, c5);
    r.drop(o4); r.drop(pre);
    // conv6 + skip (DEN.py:96,102,107) with the 1x1x1 classifier (DEN.py:97,103,108) folded into the epilogue
    ConvOpt c6; c6.res0 = &skip; c6.out_pre = out_raw; c6.cls = cls.c_str(); c6.cls_out = cls_out; c6.discard = discard_sum;
    Act sum = r.conv(p + ".conv6.0", o5, c6);
    r.drop(o5);
    if (pre1_out) *pre1_out = pre1; else r.drop(pre1);
    return sum;
}

// The four regression heads (mid_out, pred1..3) run as ONE launch at the end of the forward (DFFW_NO_REGRESS_MERGE: one launch each,
// where the score volume is ready): a head is queued here, its score volume stays allocated until flush_regress.
struct RegressQueue {
    RegressHeads hd{};
    void *keep[4] = {nullptr, nullptr, nullptr, nullptr};
    int nkeep = 0;
    double bytes = 0.0;
};
static void regress(Run &r, RegressQueue &q, const char *tag, float *score, int B, int N, int h, int w, int H, int W, const float *fd,
                    const int64_t fst[4], float *out, bool merge) {
    if (!merge) {
        if (r.ok() && !r.dry && out)
            r.launch_unnamed("dffw::regress_kernel", tag, "", 0.0, (double)B * N * h * w * 4.0 + (double)B * H * W * 4.0, tag, 0,
                             [&](unsigned long long *) { return launch_regress(score, B, N, h, w, H, W, fd, fst[0], fst[1], fst[2], fst[3], out, r.s); });
        r.drop_raw(score);
        return;
    }
    // (the score volume is kept in the dry run that sizes the workspace exactly as in the real one)
    q.keep[q.nkeep++] = score;
    if (!out || r.dry) return;
    const int k = q.hd.n++;
    q.hd.score[k] = score;
    q.hd.depth[k] = out;
    q.hd.h[k] = h;
    q.hd.w[k] = w;
    q.bytes += (double)B * N * h * w * 4.0 + (double)B * H * W * 4.0;
}
static void flush_regress(Run &r, RegressQueue &q, int B, int N, int H, int W, const float *fd, const int64_t fst[4]) {
    if (q.hd.n && r.ok() && !r.dry) {
        q.hd.nofuse = r.sw.on(SW_NO_REGRESS_FUSED) ? 1 : 0;
        const bool fused = regress_form(q.hd, B, N, H, W) != 0;   // launch_regress_heads' own test
        // algorithmic bytes: the score volumes and depth maps + a dense focus-distance map once (the fused kernel does read it once; per-head launches re-read it)
        const double bytes = q.bytes + ((fst[2] || fst[3]) ? (double)B * N * H * W * 4.0 : 0.0);
        r.launch_unnamed(fused ? "dffw::regress_fused_kernel" : "dffw::regress_kernel", "regress.mid_out+pred1+pred2+pred3", "", 0.0, bytes, "regress", 0,
                         [&](unsigned long long *) { return launch_regress_heads(q.hd, B, N, H, W, fd, fst[0], fst[1], fst[2], fst[3], r.s); });
    }
    for (int k = 0; k < q.nkeep; ++k) r.drop_raw(q.keep[k]);
    q.hd.n = 0;
    q.nkeep = 0;
}

// raw != null: FS is not given; the stem reads the raw stack (or, when the tiled stem kernel does not serve this
// shape, the stack is first expanded into a temporary fp32 volume from the workspace)
int run_depth(Run &r, const float *FS, const float *fd, const int64_t fst[4], int B, int N, int H, int W, float *const out[4], const RawStack *raw) {
    const std::string P = "DFF_net";
    const int prec = r.e->prec;
    ConvOpt rl; rl.relu = 1;
    // the low-resolution layers of the pyramid cannot fill 256 CUs on their own (at batch 32 its 1/32-resolution scale is
    // 128 tiles per launch): the three pyramid scales run side by side on the main + two side streams (measured +7 % at
    // batch 1, +5 % at batch 4, +4 % at batch 8, +1..2.5 % at batch 32; the regression heads on a side stream gained
    // nothing).  DFFW_CONCURRENT_MAX_PIXELS restricts it to stacks below that many pixels.
    {
        const int64_t z = r.sw.concurrent_max_pixels;
        // (not in profiling mode: the per-launch event durations are meant to be each kernel's own)
        const int64_t px = (int64_t)B * N * H * W;
        if ((z < 0 || px < z) && px >= r.sw.concurrent_min_pixels && !r.sw.on(SW_NO_CONCURRENT) && !r.e->profiling) r.enable_concurrency();
    }

    // feature extraction: V1 (8ch, full), V2 (16ch, 1/2), V3 (32ch, 1/4)            DEN.py:77-80
    const std::string stem_name = P + ".FM_measure.Focus_extraction.0.0";
    Act stem;
    if (r.tiled(stem_name, H, W) && !r.sw.on(SW_NO_FUSED_STEM)) {
        // the tiled stem kernel builds its paired-pixel records from the fp32 stack on the fly: no record volume
        Act geom;
        geom.B = B; geom.N = N; geom.H = H; geom.W = W + 2; geom.C = 8;
        ConvOpt so = rl;
        so.fs32 = FS;
        RawStack *rdev = nullptr;
        if (raw) {
            rdev = (RawStack *)r.raw(256);
            if (r.ok() && !r.dry) r.check(launch_set_raw(*raw, rdev, r.s), "set_raw");
            so.fs32 = (const float *)rdev;
            so.raw = true;
        }
        stem = r.conv(stem_name, geom, so);
        r.drop_raw(rdev);
    } else {
        float *tmp = nullptr;
        if (raw) {
            tmp = (float *)r.raw((int64_t)B * 3 * N * H * W * (int64_t)sizeof(float));
            if (r.ok() && !r.dry) {
                const int64_t st[5] = {raw->sb, raw->sn, raw->sy, raw->sx, raw->sc};
                if (dffw_pack_stack(r.e->device, raw->p, raw->dtype, st, B, N, raw->h, raw->w, H, W, tmp, r.s) != DFFW_OK) r.err = DFFW_EHIP;
            }
            FS = tmp;
        }
        Act in = r.act(B, N, H, W + 2, 8);   // paired-pixel records, see stack_in_kernel
        if (r.ok() && !r.dry) {
            char kn[48];
            snprintf(kn, sizeof kn, "dffw::stack_in_kernel<%d>", prec);
            r.launch_unnamed(kn, "stack_in", "", 0.0, (double)B * N * H * W * 3 * 4.0 + (double)B * N * H * (W + 2) * 8 * r.elem_bytes(), "stack_in", 0,
                             [&](unsigned long long *) { return launch_stack_in(prec, FS, in.p, B, N, H, W, r.s); });
        }
        stem = r.conv(stem_name, in, rl);
        r.drop(in);
        r.drop_raw(tmp);
    }
    r.tap("stem", stem);
    Act v1p, v2p;   // max-pooled copies written by the attention kernels on the way (EFD's second branch)
    Act v1 = srd(r, P + ".FM_measure.Focus_extraction.2", stem, true, &v1p);
    r.tap("V1", v1);
    Act e1 = efd(r, P + ".FM_conv1.0", v1, &v1p);
    r.tap("E1", e1);
    Act v2 = srd(r, P + ".FM_conv1.1", e1, true, &v2p);
    r.tap("V2", v2);
    Act e2 = efd(r, P + ".FM_conv2.0", v2, &v2p);
    r.tap("E2", e2);
    Act v3 = srd(r, P + ".FM_conv2.1", e2, true);
    r.tap("V3", v3);

    // multi-scale aggregation (1st hourglass)                                      DEN.py:82
    Act vol = pyramid(r, P + ".SPP_module", v3);
    r.tap("FS_volume", vol);

    // confidence head -> mid_out                                                   DEN.py:83-90
    // (on side stream 0 next to dres0 / deconv_1 below 16M stack pixels: two 1/8-resolution convs and a regression head that
    // nothing else waits for -- measured +2.7 % at batch 1, +2.3 % at batch 8, -0.3 % at batch 32 where dres0 fills the chip)
    RegressQueue rq;
    const bool merge_heads = true;   // (DFFW_NO_REGRESS_MERGE retired in round 5: one launch per head lost the A/B of rounds 3 and 4)
    const int h8 = H / 8, w8 = W / 8;
    float *conf = (float *)r.raw((int64_t)B * N * h8 * w8 * sizeof(float));
    const bool conf_side = r.concurrent && (int64_t)B * N * H * W < (16 << 20) && !r.sw.on(SW_NO_CONF_FORK);
    r.forked = conf_side;
    if (conf_side) {
        r.fork(0);
        r.on(0);
    }
    {
        Act c = r.conv(P + ".confidence.0.0", vol, rl);
        ConvOpt of; of.outf = conf;
        r.conv(P + ".confidence.2", c, of);
        r.drop(c);
        r.tap_f32("conf", conf, (int64_t)B * N * h8 * w8);
        regress(r, rq, "regress.mid_out", conf, B, N, h8, w8, H, W, fd, fst, out[0], merge_heads);
    }
    r.on(-1);

    // refinement                                                                   DEN.py:92-108
    Act d0 = r.conv(P + ".dres0.0.0", vol, rl);
    r.drop(vol);
    Act d1 = r.conv(P + ".dres0.2.0", d0, rl);
    r.drop(d0);
    Act x1 = r.conv(P + ".deconv_1.0", d1);
    r.drop(d1);
    if (conf_side) r.join(0);
    r.forked = false;
    r.release_deferred();

    Act pre_a, out_a;
    const int h4 = H / 4, w4 = W / 4;
    float *cost1 = (float *)r.raw((int64_t)B * N * h4 * w4 * sizeof(float));
    Act s1 = hourglass(r, P + ".dres2", x1, v3, nullptr, nullptr, x1, &pre_a, &out_a, P + ".classif1.0", cost1, false);
    r.drop(x1); r.drop(v3);
    r.tap_f32("cost1", cost1, (int64_t)B * N * h4 * w4);
    regress(r, rq, "regress.pred1", cost1, B, N, h4, w4, H, W, fd, fst, out[1], merge_heads);

    Act x2 = r.conv(P + ".deconv_2.0", s1);
    r.drop(s1);
    Act pre_b, out_b;
    const int h2 = H / 2, w2 = W / 2;
    float *cost2 = (float *)r.raw((int64_t)B * N * h2 * w2 * sizeof(float));
    Act s2 = hourglass(r, P + ".dres3", x2, v2, &pre_a, &out_a, x2, &pre_b, &out_b, P + ".classif2.0", cost2, false);
    r.drop(x2); r.drop(v2); r.drop(pre_a); r.drop(out_a);
    r.tap_f32("cost2", cost2, (int64_t)B * N * h2 * w2);
    regress(r, rq, "regress.pred2", cost2, B, N, h2, w2, H, W, fd, fst, out[2], merge_heads);

    Act x3 = r.conv(P + ".deconv_3.0", s2);
    r.drop(s2);
    float *cost3 = (float *)r.raw((int64_t)B * N * H * W * sizeof(float));
    Act s3 = hourglass(r, P + ".dres4", x3, v1, &pre_b, &out_b, x3, nullptr, nullptr, P + ".classif3.0", cost3, true);  // only its score is used
    r.drop(x3); r.drop(v1); r.drop(pre_b); r.drop(out_b);
    r.drop(s3);
    r.tap_f32("cost3", cost3, (int64_t)B * N * H * W);
    regress(r, rq, "regress.pred3", cost3, B, N, H, W, H, W, fd, fst, out[3], merge_heads);
    flush_regress(r, rq, B, N, H, W, fd, fst);
    return r.err;
}

static int check_dims(int B, int N, int H, int W) {
    if (B < 1 || N < 1) return fail(DFFW_EINVAL, "B and N must be >= 1 (got B=%d N=%d)", B, N);
    if (H < 32 || W < 32 || H % 32 || W % 32)
        return fail(DFFW_EINVAL, "H and W must be positive multiples of 32 (got %dx%d); pad with -1 as the reference loaders do", H, W);
    return DFFW_OK;
}

}  // namespace dffw

// ---- C ABI -------------------------------------------------------------------------------------
extern "C" {

const char *dffw_version(void) { return "dffw 0.1 (gfx950)"; }
const char *dffw_last_error(void) { return g_err.c_str(); }
const char *dffw_last_conv_kernel(void) { return g_last_kernel.c_str(); }

int dffw_param_count(int net) {
    if (!known_net(net)) return fail(DFFW_EINVAL, "unknown net %d", net);
    return (int)table_for(net).params.size();
}

int dffw_param_info(int net, int index, const char **name, int64_t shape[5], int *ndim, int *flags) {
    if (!known_net(net)) return fail(DFFW_EINVAL, "unknown net %d", net);
    const Table &t = table_for(net);
    if (index < 0 || index >= (int)t.params.size()) return fail(DFFW_EINVAL, "param index %d out of range", index);
    const ParamInfo &p = t.params[index];
    if (name) *name = p.name.c_str();
    if (shape) memcpy(shape, p.shape, sizeof p.shape);
    if (ndim) *ndim = p.ndim;
    if (flags) *flags = p.flags;
    return DFFW_OK;
}

int dffw_engine_create(int device, int net, const dffw_tensor *tensors, int n_tensors, int precision, dffw_engine **out) {
    if (!out) return fail(DFFW_EINVAL, "out is null");
    *out = nullptr;
    if (!known_net(net)) return fail(DFFW_EINVAL, "unknown net %d", net);
    if (precision < 0 || precision > 2) return fail(DFFW_EINVAL, "unknown precision %d", precision);
    if (!tensors || n_tensors <= 0) return fail(DFFW_EINVAL, "no tensors given");
    HIPCHK(hipSetDevice(device));
    std::map<std::string, const dffw_tensor *> by;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name) return fail(DFFW_EINVAL, "tensor %d has no name", i);
        std::string nm = tensors[i].name;
        if (nm.rfind("module.", 0) == 0) nm = nm.substr(7);
        by[nm] = &tensors[i];
    }
    auto need = [&](const std::string &nm, int64_t numel, const float **p) -> int {
        auto it = by.find(nm);
        if (it == by.end()) return fail(DFFW_EMISSING, "state dict has no entry '%s'", nm.c_str());
        if (it->second->numel != numel)
            return fail(DFFW_EINVAL, "'%s' has %lld elements, expected %lld", nm.c_str(), (long long)it->second->numel, (long long)numel);
        if (!it->second->data) return fail(DFFW_EINVAL, "'%s' has null data", nm.c_str());
        *p = it->second->data;
        return DFFW_OK;
    };
    std::unique_ptr<dffw_engine> e(new dffw_engine);
    e->device = device;
    e->net = net;
    e->prec = precision;
    const Table &t = table_for(net);
    for (const LayerDef &L : t.layers) {
        if (!L.live) continue;
        const float *w = nullptr, *cb = nullptr, *sw = nullptr;
        int scin = 0;
        if (!L.shortcut.empty()) {
            const LayerDef &S = t.layers[t.by_name.at(L.shortcut)];
            scin = S.cin;
            int rc2 = need(S.conv + ".weight", (int64_t)S.cin * S.cout, &sw);
            if (rc2) return rc2;
        }
        if (L.folded) continue;
        int rc = need(L.conv + ".weight", (int64_t)L.cin * L.cout * L.kd * L.kh * L.kw, &w);
        if (rc) return rc;
        if (L.bias && (rc = need(L.conv + ".bias", L.cout, &cb))) return rc;
        std::vector<float> bn;
        if (!L.bn.empty()) {
            const char *sfx[4] = {".weight", ".bias", ".running_mean", ".running_var"};
            bn.resize(4 * (size_t)L.cout);
            for (int k = 0; k < 4; ++k) {
                const float *p = nullptr;
                if ((rc = need(L.bn + sfx[k], L.cout, &p))) return rc;
                memcpy(bn.data() + (size_t)k * L.cout, p, L.cout * sizeof(float));
            }
        }
        PackedConv &pc = e->convs[L.conv];
        rc = pack_conv(L, precision, w, bn.empty() ? nullptr : bn.data(), cb, pc, sw, scin);
        if (rc) return rc;
        if (L.head_split > 0 && !bn.empty() && (rc = pack_head_split(L, precision, w, bn.data(), e->convs[L.conv + "#ref"], e->convs[L.conv + "#cur"]))) return rc;
    }
    *out = e.release();
    return DFFW_OK;
}

void dffw_engine_destroy(dffw_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    delete e;
}

int dffw_engine_precision(const dffw_engine *e) { return e ? e->prec : fail(DFFW_EINVAL, "null engine"); }

int64_t dffw_workspace_bytes(const dffw_engine *e, int B, int N, int H, int W) {
    if (!e) return fail(DFFW_EINVAL, "null engine");
    int rc = check_dims(B, N, H, W);
    if (rc) return rc;
    if (e->net == DFFW_NET_E2E && N != DFFW_E2E_SLICES)
        return fail(DFFW_EINVAL, "the alignment network is built for %d focal slices (End_to_End.py:46), got %d", DFFW_E2E_SLICES, N);
    Run r(const_cast<dffw_engine *>(e), nullptr, true, nullptr, INT64_MAX / 2);
    const int64_t st[4] = {0, 0, 0, 0};
    float *outs[4] = {nullptr, nullptr, nullptr, nullptr};
    rc = e->net == DFFW_NET_E2E ? run_e2e(r, nullptr, nullptr, st, nullptr, B, N, H, W, outs, nullptr)
                                : run_depth(r, nullptr, nullptr, st, B, N, H, W, outs);
    if (rc) return rc;
    return r.arena.peak();
}

int dffw_forward_e2e(dffw_engine *e, const float *FS, const float *focus_dists, const int64_t fd_strides[4], const float *fovs,
                     int B, int N, int H, int W, float *const out[4], float *aligned, void *workspace, int64_t workspace_bytes,
                     void *hip_stream, const dffw_tap *taps, int n_taps) {
    if (!e || !FS || !focus_dists || !fd_strides || !fovs || !out || !aligned) return fail(DFFW_EINVAL, "null argument");
    if (e->net != DFFW_NET_E2E) return fail(DFFW_EINVAL, "engine was not created with DFFW_NET_E2E");
    int rc = check_dims(B, N, H, W);
    if (rc) return rc;
    if (N != DFFW_E2E_SLICES)
        return fail(DFFW_EINVAL, "the alignment network is built for %d focal slices (End_to_End.py:46), got %d", DFFW_E2E_SLICES, N);
    if (!workspace) return fail(DFFW_ENOMEM, "workspace is null");
    HIPCHK(hipSetDevice(e->device));
    if (e->profiling) e->clear_recs();
    Run r(e, (hipStream_t)hip_stream, false, (char *)workspace, workspace_bytes);
    r.taps = taps;
    r.n_taps = taps ? n_taps : 0;
    return run_e2e(r, FS, focus_dists, fd_strides, fovs, B, N, H, W, out, aligned);
}

int dffw_forward_taps(dffw_engine *e, const float *FS, const float *focus_dists, const int64_t fd_strides[4], int B, int N,
                      int H, int W, float *const out[4], void *workspace, int64_t workspace_bytes, void *hip_stream,
                      const dffw_tap *taps, int n_taps) {
    if (!e || !FS || !focus_dists || !fd_strides || !out) return fail(DFFW_EINVAL, "null argument");
    int rc = check_dims(B, N, H, W);
    if (rc) return rc;
    if (!workspace) return fail(DFFW_ENOMEM, "workspace is null");
    HIPCHK(hipSetDevice(e->device));
    if (e->profiling) e->clear_recs();
    Run r(e, (hipStream_t)hip_stream, false, (char *)workspace, workspace_bytes);
    r.taps = taps;
    r.n_taps = taps ? n_taps : 0;
    return run_depth(r, FS, focus_dists, fd_strides, B, N, H, W, out);
}

int dffw_forward_raw(dffw_engine *e, const void *raw, int dtype, const int64_t raw_strides[5], int h, int w, const float *focus_dists,
                     const int64_t fd_strides[4], int B, int N, int H, int W, float *const out[4], void *workspace,
                     int64_t workspace_bytes, void *hip_stream) {
    if (!e || !raw || !raw_strides || !focus_dists || !fd_strides || !out) return fail(DFFW_EINVAL, "null argument");
    if (e->net != DFFW_NET_DEPTH) return fail(DFFW_EINVAL, "dffw_forward_raw serves DFFW_NET_DEPTH engines");
    if ((dtype & ~DFFW_RAW_NORM_F64) != DFFW_RAW_U8 && (dtype & ~DFFW_RAW_NORM_F64) != DFFW_RAW_F32) return fail(DFFW_EINVAL, "unknown raw dtype %d", dtype);
    static_assert(DFFW_RAW_NORM_F64 == DFFW_RAW_NORM_F64_BIT, "dffw.h and dffw_internal.h disagree");
    int rc = check_dims(B, N, H, W);
    if (rc) return rc;
    if (h < 1 || w < 1 || h > H || w > W) return fail(DFFW_EINVAL, "source %dx%d does not fit the padded stack %dx%d", h, w, H, W);
    if (!workspace) return fail(DFFW_ENOMEM, "workspace is null");
    HIPCHK(hipSetDevice(e->device));
    if (e->profiling) e->clear_recs();
    Run r(e, (hipStream_t)hip_stream, false, (char *)workspace, workspace_bytes);
    RawStack rs{raw, dtype, raw_strides[0], raw_strides[1], raw_strides[2], raw_strides[3], raw_strides[4], h, w};
    return run_depth(r, nullptr, focus_dists, fd_strides, B, N, H, W, out, &rs);
}

int dffw_forward(dffw_engine *e, const float *FS, const float *focus_dists, const int64_t fd_strides[4], int B, int N, int H,
                 int W, float *const out[4], void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return dffw_forward_taps(e, FS, focus_dists, fd_strides, B, N, H, W, out, workspace, workspace_bytes, hip_stream, nullptr, 0);
}

int dffw_profile_enable(dffw_engine *e, int on) {
    if (!e) return fail(DFFW_EINVAL, "null engine");
    e->profiling = on != 0;
    if (!on) e->clear_recs();
    return DFFW_OK;
}

int dffw_profile_collect(dffw_engine *e, dffw_prof_entry *out, int capacity) {
    if (!e) return fail(DFFW_EINVAL, "null engine");
    const int n = (int)e->recs.size();
    if (!out) return n;
    for (int i = 0; i < n && i < capacity; ++i) {
        ProfRec &r = e->recs[i];
        float ms = 0.f;
        if (r.e0 && r.e1) {
            HIPCHK(hipEventSynchronize(r.e1));
            HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
        }
        out[i].kernel = r.kernel.c_str();
        out[i].layer = r.layer.c_str();
        out[i].flops = r.flops;
        out[i].bytes = r.bytes;
        out[i].ms = ms;
    }
    return n;
}

const char *dffw_last_op_kernels(void) { return g_last_op_kernels.c_str(); }

}  // extern "C"
