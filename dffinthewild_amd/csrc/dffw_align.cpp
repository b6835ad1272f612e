// The alignment network of End_to_End (FlowNetwork, End_to_End.py:37-105) in front of the depth network: the feature blocks (of_block,
// of_first_block), one level of the alpha heads (align_level) and the graph that strings them together (run_e2e).  Every form a block or a
// level can take has its applicability test written once, as a named predicate beside it; the streaming kernels are dffw_align.hip, the rest
// goes through Run::conv (dffw_dispatch.cpp).  Nothing here touches activation values.
#include "dffw_run.h"

namespace dffw {

// a (B,N,H,W) grid is whole ty x tx columns, enough of them for a persistent streaming kernel, and the streaming kernels are not switched off
static bool columns_ok(const Run &r, int B, int H, int W, int ty, int tx) {
    return H % ty == 0 && W % tx == 0 && (int64_t)B * (H / ty) * (W / tx) >= r.sw.roll_min_units && !r.sw.on(SW_NO_TILE);
}
// both 1x3x3 convs of a block are packed for the streaming block kernels
static bool block_packed(const PackedConv *c0, const PackedConv *c2) { return c0 && c2 && c0->wsrd && c2->wsrd; }

// of_roll8 / of_roll: a stride-1 block (its shortcut folded into conv.2) with 8 -> 8 or 8 / 16 -> 16 channels on whole 8 x 16 columns
static bool of_roll_ok(const Run &r, const PackedConv *c0, const PackedConv *c2, const PackedConv *cf, const Act &x) {
    const int co = c0 ? c0->def.cout : 0;
    return !cf && block_packed(c0, c2) && (x.C == 8 || x.C == 16) && (co == 16 || (co == 8 && x.C == 8)) && c2->def.cout == co && c2->cin_all == co + x.C &&
           columns_ok(r, x.B, x.H, x.W, 8, 16) && !r.sw.on(SW_NO_FUSED_OF);
}
// of_s2: the 8 -> 16 down-sampling block on whole 8 x 16 output columns
static bool of_s2_ok(const Run &r, const PackedConv *c0, const PackedConv *c2, const PackedConv *cf, const Act &x) {
    return block_packed(c0, c2) && cf && cf->wsrd && x.C == 8 && c0->def.sh == 2 && c0->def.cout == 16 && c2->def.cout == 16 && c2->cin_all == 16 && cf->def.sh == 2 &&
           cf->def.cout == 16 && columns_ok(r, x.B, x.H, x.W, 16, 32) && !r.sw.on(SW_NO_FUSED_OF);
}
// of_first: the 3 -> 8 block straight from the fp32 stack, where of_roll8 would serve its record volume
static bool of_first_ok(const Run &r, const PackedConv *c0, const PackedConv *c2, const PackedConv *cf, int B, int H, int W) {
    return !cf && block_packed(c0, c2) && c0->def.cin == 3 && c0->def.cout == 8 && c2->def.cout == 8 && c2->cin_all == 16 && columns_ok(r, B, H, W, 8, 16) &&
           !r.sw.on(SW_NO_FUSED_OF) && !r.sw.on(SW_NO_OF_FIRST);
}

// resnet_block_2d_OF (End_to_End.py:135-145): relu(feature(x) + BN(conv(relu(BN(conv_s(x))))))
Act of_block(Run &r, const std::string &p, const Act &x) {
    const PackedConv *c0 = r.layer(p + ".conv.0.0"), *c2 = r.layer(p + ".conv.2.0"), *cf = r.layer(p + ".feature");
    const int prec = r.e->prec;
    char kn[64];
    if (of_roll_ok(r, c0, c2, cf, x)) {   // conv.0, conv.2 and the shortcut in one streaming kernel
        const int co = c0->def.cout;
        Act out = r.act(x.B, x.N, x.H, x.W, co);
        if (r.ok() && !r.dry) {
            SrdArgs a = srd_args(x.p, out.p, *c0, *c2, x.B, x.N, x.H, x.W, 8, 16, r.sw.srd_wgs);
            if (!(a.zero = r.zero_page())) return out;
            if (co == 8) of_roll8_kernel_name(prec, kn, sizeof kn);
            else of_roll_kernel_name(prec, x.C == 8, kn, sizeof kn);
            const double px = (double)x.pixels(), cin = c0->def.cin;
            r.launch(kn, p, "", 2.0 * px * (9.0 * cin * co + 9.0 * co * co + cin * co), px * (x.C + co) * r.elem_bytes(), "of_roll", 0,
                     [&](unsigned long long *) { return co == 8 ? launch_of_roll8(prec, a, r.s) : launch_of_roll(prec, x.C == 8, a, r.s); });
        }
        return out;
    }
    if (of_s2_ok(r, c0, c2, cf, x)) {   // the same for the strided block (a.H, a.W = the OUTPUT grid)
        Act out = r.act(x.B, x.N, x.H / 2, x.W / 2, 16);
        if (r.ok() && !r.dry) {
            SrdArgs a = srd_args(x.p, out.p, *c0, *c2, x.B, x.N, out.H, out.W, 8, 16, r.sw.srd_wgs);
            a.w3f = cf->wsrd;
            of_s2_kernel_name(prec, kn, sizeof kn);
            const double px = (double)out.pixels();
            r.launch(kn, p, "", 2.0 * px * (9.0 * 8 * 16 + 9.0 * 16 * 16 + 8.0 * 16), (4.0 * px * 8 + px * 16) * r.elem_bytes(), "of_s2", 0,
                     [&](unsigned long long *) { return launch_of_s2(prec, a, r.s); });
        }
        return out;
    }
    ConvOpt o; o.relu = 1;
    Act t = r.conv(p + ".conv.0.0", x, o);
    Act f;
    if (!cf) o.in1 = &x;   // stride-1 block: shortcut folded into conv.2 over [t | x]
    else {
        f = r.conv(p + ".feature", x);
        o.res0 = &f;
    }
    Act out = r.conv(p + ".conv.2.0", t, o);
    r.drop(t);
    r.drop(f);
    return out;
}

// The first feature block (OF_feature.0, End_to_End.py:72) from the fp32 stack FS (B,3,N,H,W): of_first_kernel reads the stack itself
// when its streaming form applies (of_roll8 with the record conversion inside its fill: the 8-channel record volume of the stack is
// neither written nor read), else the stack is converted to an 8-channel record volume and of_block() takes it.
Act of_first_block(Run &r, const std::string &p0, const float *FS, int B, int N, int H, int W) {
    const PackedConv *c0 = r.layer(p0 + ".conv.0.0"), *c2 = r.layer(p0 + ".conv.2.0");
    const int prec = r.e->prec;
    const double px = (double)B * N * H * W;
    char kn[64];
    if (of_first_ok(r, c0, c2, r.layer(p0 + ".feature"), B, H, W)) {
        Act a0 = r.act(B, N, H, W, 8);
        if (r.ok() && !r.dry) {
            SrdArgs a = srd_args(nullptr, a0.p, *c0, *c2, B, N, H, W, 8, 16, r.sw.srd_wgs);
            a.w3 = FS;   // (the one field of its type: of_first has no attention weights)
            of_first_kernel_name(prec, kn, sizeof kn);
            r.launch(kn, p0, "", 2.0 * px * (9.0 * 3 * 8 + 9.0 * 8 * 8 + 3.0 * 8), px * (3 * 4.0 + 8 * r.elem_bytes()), "of_first", 0,
                     [&](unsigned long long *) { return launch_of_first(prec, a, r.s); });
        }
        return a0;
    }
    Act in = r.act(B, N, H, W, 8);
    if (r.ok() && !r.dry) {
        snprintf(kn, sizeof kn, "dffw::from_ncdhw_pad_kernel<%d>", prec);
        r.launch_unnamed(kn, "flow.stack_in", "", 0.0, px * (3 * 4.0 + 8 * r.elem_bytes()), "from_ncdhw_pad", 0,
                         [&](unsigned long long *) { return launch_from_ncdhw_pad(prec, FS, in.p, B, 3, 8, N, H, W, r.s); });
    }
    Act a0 = of_block(r, p0, in);
    r.drop(in);
    return a0;
}

// ---- one level of the alpha heads (End_to_End.py:77-103) ----------------------------------------------------------------------------------
// The head's first conv is linear in its input channels: the part over the warped reference slice is the same for all N slices of a
// sample, so it runs once per sample (1/N of the work, no ref channels in the volume) and enters the per-slice conv over [cur | flow]
// as a slice-broadcast residual in front of the ReLU.
static bool head_split_ok(const Run &r, const std::string &hp) { return r.e->convs.count(hp + ".0.0#ref") && !r.sw.on(SW_NO_HEAD_SPLIT); }
// ... and [cur | flow] is not materialised when head_warp_kernel serves the level (8- and 16-channel levels, whole 8 x 16 columns): it
// samples the warped features while staging its tiles.  (The same inside conv_tile's fill was measured slower than flow_volume + LDS-DMA
// fill -- 1.64 vs 0.85 + 0.93 ms at level 1: a tile's gathers are one dependent latency chain per workgroup there -- and removed again.)
static bool head_warp_ok(const Run &r, const PackedConv *cur, const Act &fe) {
    return (fe.C == 8 || fe.C == 16) && cur && cur->wsrd && cur->def.cin == fe.C + 2 && cur->def.cout == 2 * fe.C && columns_ok(r, fe.B, fe.H, fe.W, 8, 16) &&
           (int64_t)fe.B * fe.N <= head_warp_max_planes() && !r.sw.on(SW_NO_HEAD_WARP);
}

// the head's first conv over [warped ref | warped cur | flow] of the level features (consumed): head_warp on the split filter, the split
// filter over a [cur | flow] volume, or the whole filter over the whole volume.  `label` names the level in the profile ("flow.conv1")
Act head_first_conv(Run &r,const std::string &hp, const std::string &label, Act &fe, const float *alpha, const float *fov) {
    const int prec = r.e->prec, B = fe.B, N = fe.N;
    ConvOpt rl; rl.relu = 1;
    char kn[64];
    snprintf(kn, sizeof kn, "dffw::flow_volume_kernel<%d>", prec);
    // mode 0: [ref | cur | flow | pad], 1: [cur | flow | pad], 2: the warped reference slice alone
    auto volume = [&](uint16_t *dst, int mode) { return launch_flow_volume(prec, fe.p, dst, alpha, fov, B, N, fe.H, fe.W, fe.C, mode, r.s); };
    if (!head_split_ok(r, hp)) {
        const int Cv = 2 * fe.C + 8;                      // 2C+2 channels of End_to_End.py:81-84, padded to a multiple of 8
        Act vol = r.act(B, N, fe.H, fe.W, Cv);
        if (r.ok() && !r.dry)
            r.launch_unnamed(kn, label, ".volume", 0.0, (double)fe.pixels() * (2.0 * fe.C + Cv) * r.elem_bytes(), "flow_volume", 0, [&](unsigned long long *) { return volume(vol.p, 0); });
        r.drop(fe);
        Act y0 = r.conv(hp + ".0.0", vol, rl);
        r.drop(vol);
        return y0;
    }
    const PackedConv *cur = r.layer(hp + ".0.0#cur");
    const bool warp = head_warp_ok(r, cur, fe);
    Act refw = r.act(B, 1, fe.H, fe.W, fe.C), vol, y0;
    if (!warp) vol = r.act(B, N, fe.H, fe.W, fe.C + 8);
    if (r.ok() && !r.dry)   // (one record for the two launches)
        r.launch_unnamed(kn, label, ".volume", 0.0, ((double)(warp ? 0 : fe.pixels()) * (2.0 * fe.C + 8) + (double)refw.pixels() * 2.0 * fe.C) * r.elem_bytes(), "flow_volume cur", 0,
                         [&](unsigned long long *) {
                             r.check(volume(refw.p, 2), "flow_volume ref");
                             return warp ? hipSuccess : volume(vol.p, 1);
                         });
    if (!warp) r.drop(fe);
    // per-slice conv: the B reference slices are presented as the B slices of ONE sample so that the 5-slice tiles are filled (same memory either way)
    Act refw1 = refw;
    refw1.B = 1; refw1.N = B;
    Act refpart = r.conv(hp + ".0.0#ref", refw1);
    refpart.B = B; refpart.N = 1;
    r.drop(refw);
    if (warp) {
        y0 = r.act(B, N, fe.H, fe.W, 2 * fe.C);
        if (r.ok() && !r.dry) {
            const HeadWarpArgs ha = head_warp_args(fe, refpart.p, y0.p, *cur, alpha, fov, r.sw.srd_wgs);
            head_warp_kernel_name(prec, fe.C, kn, sizeof kn);
            const double px = (double)fe.pixels();
            r.launch(kn, hp, ".0.0#cur", 2.0 * px * 9.0 * (fe.C + 2) * 2 * fe.C, (px * 3 + (double)refpart.pixels() * 2) * fe.C * r.elem_bytes(), "head_warp", 0,
                     [&](unsigned long long *) { return launch_head_warp(prec, fe.C, ha, r.s); });
        }
        r.drop(fe);
    } else {
        ConvOpt oc = rl;
        oc.res0 = &refpart;
        oc.res_bcast = true;
        y0 = r.conv(hp + ".0.0#cur", vol, oc);
        r.drop(vol);
    }
    r.drop(refpart);
    return y0;
}

// the head's tail (conv .6 + plane mean) as plane sums: conv .6 is packed for them
static bool tail_sums_ok(const Run &r, const PackedConv *c6) { return c6 && c6->whead && !r.sw.on(SW_NO_HEAD_SUMS); }
// two 16 -> 16 per-slice convs in a row (level-1 head at full resolution): one streaming kernel (of_roll), the intermediate in LDS
static bool head_pair_ok(const Run &r, const PackedConv *c2, const PackedConv *c4, const Act &y0) {
    return y0.C == 16 && block_packed(c2, c4) && c2->def.cout == 16 && c4->def.cout == 16 && c2->cin_all == 16 && c4->cin_all == 16 && columns_ok(r, y0.B, y0.H, y0.W, 8, 16) &&
           !r.sw.on(SW_NO_FUSED_OF);
}
// ... whose output is not stored either when the tail runs as plane sums: the kernel leaves nine 16-channel vectors per (slice, column)
// and head_tail_finish_tiles does the rest
static bool head_pair_sums_ok(const Run &r, const PackedConv *c6) { return tail_sums_ok(r, c6) && c6->def.cin == 16 && !r.sw.on(SW_NO_HEAD_SUMS_FUSED); }
// the third conv (.4) of a head without the pair kernel on conv_tile's row-sums variant: its output y1 -> y2 is not stored either
static bool head_rows_ok(const Run &r, const std::string &hp, const PackedConv *c4, const PackedConv *c6, const Act &y1) {
    return tail_sums_ok(r, c6) && c6->def.cin == y1.C && c4 && c4->def.cout == y1.C && !r.sw.on(SW_NO_HEAD_SUMS_FUSED) && r.sums_conv_ok(hp + ".4.0", y1.B, y1.N, y1.H, y1.W);
}

// the end of a head on a stored y2 (consumed): conv .6 and the plane mean, as plane sums of y2 or as the conv into three fp32 planes and
// alpha_mean; alpha += damped head output, rawh = the undamped one
void head_tail_stored(Run &r, const std::string &hp, const std::string &label, Act &y2, float *alpha, float *rawh) {
    const PackedConv *c6 = r.layer(hp + ".6");
    const int prec = r.e->prec, B = y2.B, N = y2.N;
    const int64_t na = (int64_t)B * 3 * N, hw = (int64_t)y2.H * y2.W;
    char kn[64];
    if (tail_sums_ok(r, c6) && c6->def.cin == y2.C) {
        // last conv + plane mean collapsed into plane sums of y2 (dffw_kernels.hip, "alpha head tail"): y2 is read once, the 3-plane fp32 head output is never formed
        double *partial = (double *)r.raw((int64_t)B * N * (head_tail_chunks(B, N, hw) + 4) * y2.C * sizeof(double));
        if (r.ok() && !r.dry) {
            snprintf(kn, sizeof kn, "dffw::plane_sums_kernel<%d>", prec);
            r.launch_unnamed(kn, hp, ".6+mean", 2.0 * (double)y2.pixels() * 9.0 * y2.C * 3, (double)y2.pixels() * y2.C * r.elem_bytes(), "head_tail", 0,
                             [&](unsigned long long *) { return launch_head_tail(prec, y2.p, partial, c6->whead, alpha, rawh, B, N, y2.H, y2.W, y2.C, r.s); });
        }
        r.drop_raw(partial);
        r.drop(y2);
        return;
    }
    float *hf = (float *)r.raw(na * hw * sizeof(float));
    ConvOpt of; of.outf = hf; of.outf_ch = 3;
    r.conv(hp + ".6", y2, of);
    r.drop(y2);
    if (r.ok() && !r.dry)
        r.launch_unnamed("dffw::alpha_mean_kernel", label, ".mean", 0.0, (double)na * hw * 4.0, "alpha_mean", 0, [&](unsigned long long *) { return launch_alpha_mean(hf, alpha, rawh, B, N, hw, r.s); });
    r.drop_raw(hf);
}

// from the first conv's output y0 (consumed) through convs .2, .4, .6 and the plane mean to alpha += damped head output, rawh = the undamped one
void head_tail(Run &r, const std::string &hp, const std::string &label, Act &y0, float *alpha, float *rawh) {
    const PackedConv *c2 = r.layer(hp + ".2.0"), *c4 = r.layer(hp + ".4.0"), *c6 = r.layer(hp + ".6");
    const int prec = r.e->prec, B = y0.B, N = y0.N;
    ConvOpt rl; rl.relu = 1;
    char kn[64];
    Act y2;
    if (head_pair_ok(r, c2, c4, y0)) {
        const bool sums = head_pair_sums_ok(r, c6);
        const int tiles_y = y0.H / 8, tiles_x = y0.W / 16;
        const int64_t tsum_bytes = (int64_t)B * N * tiles_y * tiles_x * 18 * 16 * sizeof(float);
        float *tsum = nullptr;
        double *seg = nullptr;
        if (sums) {
            tsum = (float *)r.raw(tsum_bytes);
            seg = (double *)r.raw(head_tail_tiles_scratch_bytes(B, N, 16));
        } else y2 = r.act(B, N, y0.H, y0.W, 16);
        if (r.ok() && !r.dry) {
            SrdArgs a = srd_args(y0.p, sums ? (uint16_t *)tsum : y2.p, *c2, *c4, B, N, y0.H, y0.W, 8, 16, r.sw.srd_wgs);
            if (!(a.zero = r.zero_page())) return;
            of_roll_kernel_name(prec, false, kn, sizeof kn, sums);
            const double px = (double)y0.pixels();
            r.launch(kn, hp, sums ? ".2.0+.4.0+.6+mean" : ".2.0+.4.0", 2.0 * px * (2 * 9.0 * 16 * 16 + (sums ? 9.0 * 16 * 3 : 0.0)), px * (sums ? 16 : 32) * r.elem_bytes(), "of_roll (head)", 0,
                     [&](unsigned long long *) { return launch_of_roll(prec, false, a, r.s, sums); });
            if (sums)
                r.launch_unnamed("dffw::head_tail_tiles_reduce_kernel", hp, ".6+mean (finish)", 0.0, (double)tsum_bytes, "head_tail_tiles", 0, [&](unsigned long long *) {
                    return launch_head_tail_tiles(tsum, seg, tiles_y, tiles_x, c6->whead, alpha, rawh, B, N, y0.H, y0.W, 16, r.s);
                });
        }
        r.drop(y0);
        r.drop_raw(seg);
        r.drop_raw(tsum);
        if (sums) return;
    } else {
        Act y1 = r.conv(hp + ".2.0", y0, rl);
        r.drop(y0);
        if (head_rows_ok(r, hp, c4, c6, y1)) {
            const int tiles_x = y1.W / c4->tile.cfg->tx;
            const int64_t rows_bytes = (int64_t)B * N * y1.H * tiles_x * 3 * y1.C * sizeof(float);
            float *rows = (float *)r.raw(rows_bytes);
            double *seg = (double *)r.raw(head_tail_tiles_scratch_bytes(B, N, y1.C));
            ConvOpt os = rl;
            os.sums = rows;
            r.conv(hp + ".4.0", y1, os);
            if (r.ok() && !r.dry)
                r.launch_unnamed("dffw::head_tail_rows_reduce_kernel", hp, ".6+mean (finish)", 0.0, (double)rows_bytes, "head_tail_rows", 0, [&](unsigned long long *) {
                    return launch_head_tail_rows(rows, seg, tiles_x, c6->whead, alpha, rawh, B, N, y1.H, y1.W, y1.C, r.s);
                });
            r.drop_raw(seg);
            r.drop_raw(rows);
            r.drop(y1);
            return;
        }
        y2 = r.conv(hp + ".4.0", y1, rl);
        r.drop(y1);
    }
    head_tail_stored(r, hp, label, y2, alpha, rawh);
}

// One level of End_to_End.py:77-103 with the head `hp`: warps the level features `fe` (consumed) by the alpha accumulated so far, runs the
// head on [ref | cur | flow], adds its damped plane means to `alpha` (B,3,N) and leaves the undamped ones in `rawh`.  No taps.
static void align_level(Run &r, const std::string &hp, const std::string &label, Act &fe, float *alpha, float *rawh, const float *fov) {
    Act y0 = head_first_conv(r, hp, label, fe, alpha, fov);
    head_tail(r, hp, label, y0, alpha, rawh);
}

// End_to_End.Network.forward (End_to_End.py:13-16): FlowNetwork.forward (End_to_End.py:71-105) aligns the stack,
// DFF_net runs on the aligned stack.  `aligned` receives the warped focal stack (the 5th return value).
int run_e2e(Run &r, const float *FS, const float *fd, const int64_t fst[4], const float *fov, int B, int N, int H, int W, float *const out[4], float *aligned) {
    const std::string P = "optical_flow_aggregation";
    // three feature levels: full, 1/2, 1/4 resolution                               End_to_End.py:72-74
    Act a0 = of_first_block(r, P + ".OF_feature.0", FS, B, N, H, W);
    Act fe1 = of_block(r, P + ".OF_feature.1", a0);
    r.drop(a0);
    r.tap("fe1", fe1);
    Act a1 = of_block(r, P + ".OF_feature1.0", fe1);
    Act fe2 = of_block(r, P + ".OF_feature1.1", a1);
    r.drop(a1);
    r.tap("fe2", fe2);
    Act a2 = of_block(r, P + ".OF_feature2.0", fe2);
    Act fe3 = of_block(r, P + ".OF_feature2.1", a2);
    r.drop(a2);
    r.tap("fe3", fe3);

    const int64_t na = (int64_t)B * 3 * N;
    float *alpha = (float *)r.raw(na * sizeof(float));   // accumulated (scale offset, x shift, y shift) per (b, slice)
    float *rawh = (float *)r.raw(na * sizeof(float));    // last head output before damping (debug tap)
    if (r.ok() && !r.dry) r.check(hipMemsetAsync(alpha, 0, na * sizeof(float), r.s), "alpha memset");

    struct Level { Act *fe; const char *head; const char *tap; const char *atap; };
    Level levels[3] = {{&fe3, ".conv1", "head3", "alpha3"}, {&fe2, ".conv2", "head2", "alpha2"}, {&fe1, ".conv3", "head1", nullptr}};
    for (const Level &lv : levels) {                      // coarse to fine
        align_level(r, P + lv.head, std::string("flow") + lv.head, *lv.fe, alpha, rawh, fov);
        r.tap_f32(lv.tap, rawh, na);
        if (lv.atap) r.tap_f32(lv.atap, alpha, na);   // (after level 1 it is the final "alpha" below)
    }
    r.tap_f32("alpha", alpha, na);
    if (r.ok() && !r.dry)                                 // End_to_End.py:104
        r.launch_unnamed("dffw::fov_warp_kernel", "flow.warp_stack", "", 0.0, (double)B * N * H * W * 3 * 8.0, "fov_warp", 0,
                         [&](unsigned long long *) { return launch_fov_warp(FS, alpha, fov, aligned, nullptr, B, 3, N, H, W, 0, r.s); });
    r.drop_raw(rawh);
    r.drop_raw(alpha);
    if (!r.ok()) return r.err;
    return run_depth(r, aligned, fd, fst, B, N, H, W, out);
}

}  // namespace dffw
