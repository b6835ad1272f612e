// Conv dispatch of libdffw.so: which kernel family serves one convolution of the graph, and its launches.
//
// plan_conv() DECIDES: from the packed layer, the input / output geometry, the ConvOpt, the switch snapshot and the precision it
// returns a ConvPlan -- the family, its one to four launches (kernel name, profile label, kernel arguments, flops and bytes), the
// split-K scratch size and whether the classifier's score volume is cleared first.  It makes no HIP call, touches no arena and sets
// no global.  Run::conv() LAUNCHES: it allocates the outputs, asks for the plan, accounts for the scratch block, and -- unless this
// is the dry run that sizes the workspace -- walks the plan's launches through Run::launch().  Dry and real run call the same
// plan_conv(), so they cannot take different allocation paths.
//
// The ten streaming (persistent rolling-window) families are the rows of kStream[], in order of precedence.  A row is one small
// function that states the family's facts (filter, conditions, column tile, units and threshold, zsplit rule, launches, flops and
// bytes) + two adapters to its name function and launcher; Planner::columns / on_grid / zsplit / add are the shell they share.  A new
// streaming family is one more row, one more such function and its two adapters (DESIGN.md 5.2 has the table in words).
#include "dffw_run.h"
#include "dffw_stem.h"

namespace dffw {
namespace {

struct ConvLaunch {
    char kernel[96];
    const char *suffix;   // profile label = layer name + suffix
    ConvArgs a;
    RollArgs r;           // (streaming families)
    int v0, v1;           // what the family's launcher takes beside the arguments: row phase | output tiles, input halves | pair form
    double flops, bytes;
};

enum { F_TILE = 100, F_GATHER = 101 };   // ConvPlan::family: an index into kStream[], or one of these

struct ConvPlan {
    int family = -1;
    int n = 0;
    ConvLaunch l[4];
    bool clear_scores = false;   // conv_rollt ADDS the fused classifier's two partial dots per pixel to the score volume
    // conv_tile (one launch, l[0]; + the split-K finish)
    const TileCfg *cfg = nullptr;
    TileArgs t;
    bool stem_pipe = false;      // ... on the persistent pipelined stem kernel (dffw_stem.hip) instead
    int64_t partial_bytes = 0;   // split-K scratch block (fp32 partial sums), 0: none
    int64_t M_out = 0;
    double finish_bytes = 0;
    int err = DFFW_OK;
    char msg[192];
};

struct Cols {
    int tiles_y, tiles_x;
    int64_t n;
    bool whole;   // the grid is whole columns (else the bottom / right ones are partial)
};

struct Planner;
struct StreamFamily {
    bool (Planner::*plan)(ConvPlan &p) const;   // false: the family does not serve this call
    void (*name)(int prec, const ConvLaunch &l, char *buf, int n);
    hipError_t (*go)(int prec, const ConvLaunch &l, hipStream_t s);
    bool step_trace;   // the kernel writes a step timeline (make TRACE=1) through ConvArgs::trace
};
extern const StreamFamily kStream[];
// the stem_pair bias swap of plan_conv() happens after the first five families and before the rest
constexpr int kStreamBeforeStemPair = 5, kStreamCount = 10;

struct Planner {
    const std::string &name;
    const PackedConv &pc;
    const LayerDef &L;
    const Act &in0;
    const ConvOpt &o;
    const Switches &sw;
    const int prec;
    const Act &out;
    ConvArgs a;   // everything but the grid: volumes, epilogue, switch bits
    const int No, Ho, Wo, cin_pad;
    const double eb, opx, in_b;   // bytes per element; output pixels; bytes of the input volume
    int fam = 0;                  // the row of kStream[] being tried

    // terms of the byte counts (all integer valued, so sums and quotients of them are exact in any order)
    double out_b(int k) const { return opx * L.cout * eb * k; }
    double w_b(double taps) const { return taps * L.cin * L.cout * eb; }
    double cls_b() const { return o.cls ? opx * 4.0 : 0.0; }
    double sums_b() const { return opx / 16.0 * 3.0 * L.cout * 4.0; }
    double mac(double points, double taps) const { return 2.0 * points * taps * L.cin * L.cout; }
    int res(const Act *r) const { return r ? 1 : 0; }

    // columns of ty x tx on the input grid (transposed forms) or the output grid
    Cols columns(bool in_grid, int ty, int tx) const {
        const int H = in_grid ? in0.H : Ho, W = in_grid ? in0.W : Wo;
        Cols g;
        g.tiles_y = (H + ty - 1) / ty;
        g.tiles_x = (W + tx - 1) / tx;
        g.n = (int64_t)g.tiles_y * g.tiles_x;
        g.whole = H % ty == 0 && W % tx == 0;
        return g;
    }
    // the arguments with the GEMM columns counted on that grid
    ConvArgs on_grid(bool in_grid) const {
        ConvArgs g = a;
        g.Ng = in_grid ? in0.N : No;
        g.Hg = in_grid ? in0.H : Ho;
        g.Wg = in_grid ? in0.W : Wo;
        g.M = (int64_t)g.B * g.Ng * g.Hg * g.Wg;
        return g;
    }
    // (the ablation bits these kernels know + the launchers' path switches)
    static ConvArgs masked(ConvArgs g) {
        g.dbg &= (6 | DFFW_ARGS_NO_LEAN_TILE | DFFW_ARGS_NO_LEAN_ROLL | DFFW_ARGS_NO_ROLLX | DFFW_ARGS_NO_ROLLK | DFFW_ARGS_NO_SLICE32);
        return g;
    }
    // a sample's slices as two ranges where whole columns leave the chip short of workgroups; DFFW_ROLL_ZSPLIT overrides
    int zsplit(int64_t units, int64_t below) const {
        int z = (units < below && No >= 8) ? 2 : 1;
        if (sw.roll_zsplit >= 1 && sw.roll_zsplit <= No) z = sw.roll_zsplit;
        return z;
    }
    // one launch of family `fam`
    void add(ConvPlan &p, const ConvArgs &g, const uint16_t *filter, const Cols &c, int zs, int pair, double flops, double bytes,
             const char *suffix = "", int v0 = 0, int v1 = 0) const {
        p.family = fam;
        ConvLaunch &l = p.l[p.n++];
        l.a = g;
        l.r = roll_args(filter, in0.B, c.tiles_y, c.tiles_x, zs, sw.roll_wgs, pair);
        l.suffix = suffix;
        l.v0 = v0;
        l.v1 = v1;
        l.flops = flops;
        l.bytes = bytes;
        kStream[fam].name(prec, l, l.kernel, sizeof l.kernel);
    }

    // transposed 32 / 64 -> 32 / 64 (deconv_1, dres2.conv5 / conv6, dres3.conv5, SPP conv9) on 8 x 8 columns of the input grid: the streaming kernel with the
    // filter split over the waves by output phase; a unit = (column, 32-channel output half)
    bool rollt(ConvPlan &p) const {
        if (!(pc.wrollt && !o.in1 && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_ROLLT))) return false;
        int ty, tx;
        rollt_tile(L.cout, &ty, &tx);
        const Cols c = columns(true, ty, tx);   // (partial columns are predicated in the kernel)
        const ConvArgs g = on_grid(true);
        // (column, output half) units from which the kernel beats conv_tile / conv_roll_t32, measured at batch 8 / 16 / 32 (profiles/r06_rollt_thresholds.txt): 128 for the
        // 8-wave forms -- half the CUs busy, and still 0.046 vs 0.058 ms on deconv_1 at batch 8, 0.052 vs 0.072 on SPP conv9 at batch 32; 64 units lose --, 192 for the 4-wave form
        const int64_t units = (int64_t)in0.B * c.n * std::max(1, L.cout / 32);
        const bool four = cin_pad == 32 && L.cout != 16;
        if (!(units >= (int64_t)sw.rollt_min_units * (four ? 3 : 2) / 2 && rollt_ok(prec, g))) return false;
        p.clear_scores = g.cls_w != nullptr;
        add(p, g, pc.wrollt, c, 1, 0, mac((double)g.M, 27.0),
            in_b + out_b((o.discard ? 0 : 1) + (o.out_pre ? 1 : 0) + res(o.res0)) + cls_b() + w_b(27.0));
        return true;
    }
    // transposed 32 -> 16 (deconv_2, dres3.conv6): two sweeps of conv_roll_t32, one per output row phase
    bool roll_t32(ConvPlan &p) const {
        if (!(pc.wroll_t32 && (in0.C == 32 || in0.C == 16) && !o.in1 && !o.res_bcast && !o.res1 && !o.outf && in0.H % 8 == 0 && in0.W % 16 == 0 &&
              (int64_t)in0.B * (in0.H / 8) * (in0.W / 16) >= sw.roll_min_units && !sw.on(SW_NO_ROLL)))
            return false;
        const ConvArgs g = masked(on_grid(true));
        for (int py = 0; py < 2; ++py) {
            int ty, tx;
            roll_t32_tile(py, &ty, &tx);
            const Cols c = columns(true, ty, tx);   // (8 x 16 or 4 x 16: whole columns, by the test above)
            // (0.5: this sweep's output pixels)
            add(p, g, pc.wroll_t32 + (size_t)(py ? ROLL_CHUNKS_T32_0 : 0) * prec_parts(prec) * 512, c, 1, 0, mac((double)g.M, py ? 18.0 : 9.0),
                in_b + 0.5 * out_b((o.discard ? 0 : 1) + (o.out_pre ? 1 : 0) + res(o.res0)) + 0.5 * cls_b(), py ? " (odd rows)" : " (even rows)", py);
        }
        return true;
    }
    // strided 3x3x3 over 16 / 32 channels (FM_conv2.0.stride_conv, dres3.conv1, dres4.conv3; dres3.conv3, dres2.conv1, SPP conv1):
    // rolling window with whole pixel records
    bool roll_s2(ConvPlan &p) const {
        if (!(pc.wroll_s2 && !L.transposed && L.sh == 2 && (in0.C == 16 || in0.C == 32) && !o.in1 && !o.res1 && !o.res_bcast && !o.outf && !o.out_pre &&
              !o.cls && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_ROLL_S2) &&
              (L.cout <= 32 || !sw.on(SW_NO_ROLL_S2_WIDE))))   // 32 -> 64 as two launches: level with conv_tile in r02, 4-7 % faster since the r04 row-pitch fix of conv_roll_s2
            return false;
        const int khn = in0.C / 16;
        const int ntk = (khn == 2 || L.cout >= 32) ? 2 : 1;     // output tiles per launch
        const int nlaunch = (L.cout / 16 + ntk - 1) / ntk;
        int ty, tx;
        s2_roll_tile(ntk, &ty, &tx);
        const Cols c = columns(false, ty, tx);
        if (!((L.cout / 16) % ntk == 0 && c.whole && in0.H == 2 * Ho && in0.W == 2 * Wo && (int64_t)in0.B * c.n >= sw.roll_min_units)) return false;
        const ConvArgs g = masked(on_grid(false));
        for (int li = 0; li < nlaunch; ++li)   // pair: first 16-channel output tile of this launch
            add(p, g, pc.wroll_s2, c, 1, li * ntk, mac(opx, 27.0) / nlaunch, in_b + out_b(1 + res(o.res0)) / nlaunch + w_b(27.0) / nlaunch,
                nlaunch > 1 ? (li ? " (upper output channels)" : " (lower output channels)") : "", ntk, khn);
        return true;
    }
    // strided 3x3x3 8 -> 16 (dres4.conv1): the single-branch form of conv_roll_efd
    bool roll_efd(ConvPlan &p) const {
        int ty, tx;
        efd_roll_tile(&ty, &tx);
        const Cols c = columns(false, ty, tx);
        if (!(pc.wroll8 && !L.transposed && L.sh == 2 && in0.C == 8 && !o.in1 && !o.res0 && !o.res1 && !o.res_bcast && !o.outf && !o.out_pre &&
              !o.cls && c.whole && (int64_t)in0.B * c.n >= sw.roll_min_units && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_ROLL_S2)))
            return false;
        add(p, masked(on_grid(false)), pc.wroll8, c, 1, 0, mac(opx, 27.0), in_b + out_b(1) + w_b(27.0));
        return true;
    }
    // ... and its transposed sibling (16 -> 8 channels), tiled over the input grid
    bool roll_t(ConvPlan &p) const {
        int ty, tx;
        roll_tile(&ty, &tx);
        const Cols c = columns(true, ty, tx);
        if (!(pc.wroll_t && c.whole && in0.C == 16 && !o.in1 && !o.res_bcast && !o.res1 && !o.outf &&
              (int64_t)in0.B * c.n >= sw.roll_min_units && !sw.on(SW_NO_ROLL)))
            return false;
        const ConvArgs g = on_grid(true);
        add(p, g, pc.wroll_t, c, zsplit((int64_t)in0.B * c.n, 1024), 1, mac((double)g.M, 27.0),
            in_b + out_b((o.discard ? 0 : 1) + (o.out_pre ? 1 : 0)) + out_b(res(o.res0)) + cls_b() + w_b(27.0));
        return true;
    }
    // 32 -> 16 channels on whole 8 x 16 columns: the pipelined rolling window with the contraction split over the two input halves
    bool rollx_k2(ConvPlan &p) const {
        const Cols c = columns(false, 8, 16);
        const bool halves = o.in1 ? (in0.C == 16 && o.in1->C == 16) : in0.C == 32;
        if (!(pc.wroll_k2 && halves && c.whole && (int64_t)in0.B * c.n >= sw.roll_min_units && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_ROLLX))) return false;
        const ConvArgs g = on_grid(false);
        if (!rollx_k2_ok(prec, g)) return false;
        add(p, g, pc.wroll_k2, c, zsplit((int64_t)in0.B * c.n, 512), 0, mac(opx, 27.0), in_b + out_b(1) + w_b(27.0));
        return true;
    }
    // per-slice 1x3x3, 32 -> 32 channels on whole 8 x 16 columns: the streaming kernel with the filter resident in every wave
    bool slice32(ConvPlan &p) const {
        if (!(pc.wslice32 && !o.in1 && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_SLICE32))) return false;
        int ty, tx;
        slice32_tile(&ty, &tx);
        const Cols c = columns(false, ty, tx);
        const ConvArgs g = on_grid(false);
        if (!(c.whole && (int64_t)in0.B * c.n >= sw.roll_min_units && slice32_ok(prec, g))) return false;
        add(p, g, pc.wslice32, c, 1, 0, mac(opx, 9.0), in_b + (o.sums ? sums_b() : out_b(1 + res(o.res0))) + w_b(9.0));
        return true;
    }
    // per-slice 1x3x3, 64 -> 64 channels on whole 8 x 16 columns: the streaming kernel with one output tile's filter resident per wave
    bool slice64(ConvPlan &p) const {
        if (!(pc.wslice64 && (pc.slice_cat ? (o.in1 && o.in1->C == 32) : !o.in1) && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_SLICE32))) return false;
        int ty, tx;
        slice32_tile(&ty, &tx);
        const Cols c = columns(false, ty, tx);
        const ConvArgs g = on_grid(false);
        if (!(c.whole && (int64_t)in0.B * c.n >= sw.roll_min_units && slice64_ok(prec, g))) return false;
        add(p, g, pc.wslice64, c, 1, 0, mac(opx, 9.0), in_b + (o.sums ? sums_b() : out_b(1)) + w_b(9.0));
        return true;
    }
    // 32 / 64 -> 32 / 64 channels on 8 x 8 columns: the K-split rolling window (one launch per 32 output channels)
    bool rollk(ConvPlan &p) const {
        if (!(pc.wrollk && !sw.on(SW_NO_ROLL) && !sw.on(SW_NO_ROLLK))) return false;
        int ty, tx;
        rollk_tile(&ty, &tx);
        const Cols c = columns(false, ty, tx);   // (partial columns at the bottom / right edge are predicated in the kernel)
        const ConvArgs g = on_grid(false);
        // 64 output channels = two 32-channel halves as grid.y of ONE launch (round 6: the 16 x 16-grid layers `dres16_*`, `conv2`, `dres2.conv4` at batch 32
        // are 128 columns x 2 halves = one unit per CU and now take this kernel; DFFW_ROLLK_MERGE_BELOW=1: two launches)
        const int npair = L.cout / 32;
        const bool merged = npair == 2 && (int64_t)in0.B * c.n < sw.rollk_merge_below;
        const int64_t units = (int64_t)in0.B * c.n * (merged ? npair : 1);
        if (!(units >= sw.roll_min_units && rollk_waves(prec, g) == cin_pad / 8)) return false;
        const int nlaunch = merged ? 1 : npair;
        // zsplit: 16 waves per CU: 256 8-wave / 512 4-wave units;  pair: first 16-channel output tile of this launch (-1: every half, as grid.y)
        for (int op = 0; op < nlaunch; ++op)
            add(p, g, pc.wrollk + (size_t)op * (cin_pad / 8) * ROLLK_CHUNKS * 2 * prec_parts(prec) * 512, c, zsplit(units, cin_pad == 64 && merged ? 256 : 512),
                merged ? -1 : op * 2, mac(opx, 27.0) / nlaunch, in_b + out_b(1 + res(o.res0)) / nlaunch + w_b(27.0) / nlaunch,
                nlaunch > 1 ? (op ? " (upper output channels)" : " (lower output channels)") : "");
        return true;
    }
    // rolling-window kernel: 16-channel 3x3x3 stride-1 layers whose grid is whole columns and fills the chip
    bool roll(ConvPlan &p) const {
        int ty, tx;
        roll_tile(&ty, &tx);
        const Cols c = columns(false, ty, tx);
        if (!(pc.wroll && c.whole && in0.C % 8 == 0 && (!o.in1 || o.in1->C == in0.C) && !o.res_bcast && !o.res1 &&
              (int64_t)in0.B * c.n >= sw.roll_min_units && !sw.on(SW_NO_ROLL)))
            return false;
        add(p, on_grid(false), pc.wroll, c, zsplit((int64_t)in0.B * c.n, 1024), pc.roll_pair ? 1 : 0, mac(opx, 27.0),
            in_b + (o.outf ? opx * L.cout * 4.0 : out_b(o.out_pre ? 2 : 1)) + out_b(res(o.res0) + res(o.res1)) + w_b(27.0), "", pc.roll_pair);
        return true;
    }

    void tile(ConvPlan &p, const TilePack &tp, bool stem_pair, int gH, int gW);
    void gather(ConvPlan &p);
};

const StreamFamily kStream[kStreamCount] = {
    {&Planner::rollt, [](int, const ConvLaunch &l, char *b, int n) { conv_rollt_kernel_name(l.a, b, n); },
     [](int, const ConvLaunch &l, hipStream_t s) { return launch_conv_rollt(l.a, l.r, s); }, false},
    {&Planner::roll_t32, [](int prec, const ConvLaunch &l, char *b, int n) { conv_roll_t32_kernel_name(prec, l.v0, l.a, b, n); },
     [](int prec, const ConvLaunch &l, hipStream_t s) { return launch_conv_roll_t32(prec, l.v0, l.a, l.r, s); }, false},
    {&Planner::roll_s2, [](int prec, const ConvLaunch &l, char *b, int n) { conv_roll_s2_kernel_name(prec, l.v0, l.v1, l.a, b, n); },
     [](int prec, const ConvLaunch &l, hipStream_t s) { return launch_conv_roll_s2(prec, l.v0, l.v1, l.a, l.r, s); }, false},
    {&Planner::roll_efd, [](int prec, const ConvLaunch &l, char *b, int n) { conv_roll_efd_kernel_name(prec, l.a, false, b, n); },
     [](int prec, const ConvLaunch &l, hipStream_t s) { return launch_conv_roll_efd(prec, l.a, l.r, s); }, false},
    {&Planner::roll_t, [](int prec, const ConvLaunch &l, char *b, int n) { conv_roll_t_kernel_name(prec, l.a, b, n); },
     [](int prec, const ConvLaunch &l, hipStream_t s) { return launch_conv_roll_t(prec, l.a, l.r, s); }, false},
    {&Planner::rollx_k2, [](int, const ConvLaunch &l, char *b, int n) { conv_rollx_k2_kernel_name(l.a, b, n); },
     [](int, const ConvLaunch &l, hipStream_t s) { return launch_conv_rollx_k2(l.a, l.r, s); }, false},
    {&Planner::slice32, [](int, const ConvLaunch &l, char *b, int n) { conv_slice32_kernel_name(l.a, b, n); },
     [](int, const ConvLaunch &l, hipStream_t s) { return launch_conv_slice32(l.a, l.r, s); }, false},
    {&Planner::slice64, [](int, const ConvLaunch &l, char *b, int n) { conv_slice64_kernel_name(l.a, b, n); },
     [](int, const ConvLaunch &l, hipStream_t s) { return launch_conv_slice64(l.a, l.r, s); }, false},
    {&Planner::rollk, [](int, const ConvLaunch &l, char *b, int n) { conv_rollk_kernel_name(l.a, b, n); },
     [](int, const ConvLaunch &l, hipStream_t s) { return launch_conv_rollk(l.a, l.r, s); }, false},
    {&Planner::roll, [](int prec, const ConvLaunch &l, char *b, int n) { conv_roll_kernel_name(prec, l.a, l.v0 != 0, b, n); },
     [](int prec, const ConvLaunch &l, hipStream_t s) { return launch_conv_roll(prec, l.a, l.r, s); }, true},
};

// conv_tile: the LDS-tiled kernel with its channel split / pass split / team / split-K planning
void Planner::tile(ConvPlan &p, const TilePack &tp, bool stem_pair, int gH, int gW) {
    const TileCfg *cfg = tp.cfg;   // may be replaced by a narrower instantiation of the same tile (channel split)
    a.Ng = L.transposed ? in0.N : No;
    a.Hg = gH;
    a.Wg = gW;
    a.sy = a.sx = L.transposed ? 1 : L.sh;
    a.osy = a.osx = L.transposed ? 2 : 1;
    a.M = (int64_t)a.B * a.Ng * a.Hg * a.Wg;
    TileArgs &t = p.t;
    memset(&t, 0, sizeof t);
    t.npass = tp.npass;
    t.nstage = tp.nstage;
    double flops = 0;
    for (int ps = 0; ps < tp.npass; ++ps) {
        t.KC[ps] = tp.KC[ps];
        t.tab[ps] = tp.tab[ps];
        t.wpk[ps] = tp.wpk[ps];
        t.ooy[ps] = tp.ooy[ps];
        t.oox[ps] = tp.oox[ps];
        flops += 2.0 * (double)a.M * (L.transposed ? tp.ntaps[ps] : L.kd * L.kh * L.kw) * L.cin * L.cout;
    }
    t.nt_total = pc.nt;
    t.nsplit = pc.nt / cfg->nt;   // (1, except the narrow packs of layers with more than 4 output tiles)
    // the tiles of configuration `c` on this grid, one per workgroup with the launch a multiple of the 8 XCDs, and whether the t.nsplit workgroups of each are
    // few enough to warm their weights (so: called again when t.nsplit has changed)
    auto set_tiles = [&](const TileCfg *c) {
        t.tiles_z = (a.Ng + c->tz - 1) / c->tz;
        t.tiles_y = (a.Hg + c->ty - 1) / c->ty;
        t.tiles_x = (a.Wg + c->tx - 1) / c->tx;
        t.total_tiles = a.B * t.tiles_z * t.tiles_y * t.tiles_x;
        t.grid = 8 * ((t.total_tiles + 7) / 8);
        t.warm = (t.total_tiles * t.nsplit <= sw.warm_max_wgs) ? 1 : 0;
    };
    // workgroups of a launch on the team configuration `c` with `nsplit` output-channel workgroups per tile and `npass` passes over grid.z
    auto team_wgs = [&](const TileCfg *c, int nsplit, int npass) {
        return (int64_t)a.B * ((a.Ng + c->tz - 1) / c->tz) * ((a.Hg + c->ty - 1) / c->ty) * ((a.Wg + c->tx - 1) / c->tx) * nsplit * npass;
    };
    set_tiles(cfg);
    // few-tile layers (the 1/16..1/32-resolution pyramid, or batch 1): split the output channels over
    // grid.y so that at least ~one workgroup per CU exists
    // (3x3x3 stride-1 and transposed layers also at exactly one tile per CU -- the 16x16-grid layers at batch 32: two 32-channel
    // workgroups per tile keep three workgroups resident instead of two, -10 % on those layers; the stride-2 layers lose 40 % with it)
    // (transposed layers with 64 outputs: the 4-output-tile block runs at 127 TFLOP/s where two launches' worth of 2-tile workgroups run at 212 -- measured on End_to_End's
    // `dres2.conv5`, 384 tiles at batch 8 --, so they split up to 1024 tiles)
    const int split_below = (cfg->geo == G3T && pc.nt >= 4) ? sw.split_t64 : (cfg->geo == G3S1 && pc.nt == 4) || (cfg->geo == G3S2 && pc.nt >= 8) ? sw.split_s64 : ((cfg->geo == G3S1 || cfg->geo == G3T) ? 257 : 256);
    if (t.total_tiles < split_below && pc.nt > 1 && !o.cls && !sw.on(SW_NO_SPLIT)) {
        const int want = (256 + t.total_tiles - 1) / t.total_tiles;   // split factor that would fill the chip (narrow blocks: 512 measured level)
        for (int nts = pc.nt / 2; nts >= 1; nts /= 2) {               // coarsest split first
            const TileCfg *c2 = pc.nt % nts == 0 ? tile_cfg_find_like(tp.cfg, nts) : nullptr;   // (whole splits only)
            if (!c2) continue;
            cfg = c2;
            t.nsplit = pc.nt / nts;
            if (t.nsplit >= want) break;
        }
        set_tiles(cfg);   // (the same tiles: find_like keeps the block shape)
    }
    // split-K: when even the channel split leaves most CUs idle and the contraction is several channel-group
    // stages deep, the stages are dealt to grid.z workgroups (fp32 partials, summed in fixed order by
    // splitk_finish) so that one workgroup no longer walks all of them in sequence
    t.ksplit = 1;
    p.M_out = (int64_t)out.B * No * Ho * Wo;
    // transposed conv on few tiles: its 4 sub-pixel passes as 4 workgroups (no reduction, any epilogue)
    const int thr = sw.split_wg;
    t.pass_split = (L.transposed && t.total_tiles * t.nsplit <= thr && !sw.on(SW_NO_SPLITK)) ? 1 : 0;
    if (t.pass_split && tp.nstage >= 2 && !sw.on(SW_NO_TEAMS)) {
        // a transposed layer whose passes are workgroups of their own walks its 2-4 channel-group stages one after the other (SPP conv8 at batch 1:
        // 30 us): one stage per team instead, with as few output-channel workgroups per tile as keep the launch to one round of workgroups
        for (int nts = cfg->nt; nts <= pc.nt && nts <= 2; nts *= 2) {
            const TileCfg *team = pc.nt % nts == 0 ? tile_cfg_find_team(cfg, tp.nstage, nts) : nullptr;   // (whole splits only)
            if (!team || team_wgs(team, pc.nt / nts, 4) > sw.team_max_wgs) continue;
            cfg = team;
            t.nsplit = pc.nt / nts;
            set_tiles(cfg);
            break;
        }
    }
    if (!t.pass_split && tile_cfg_has_splitk(cfg) && t.total_tiles * t.nsplit <= thr * 3 / 4 && tp.nstage >= 2 && !o.cls && !o.out_pre && !o.outf && !o.discard && !o.res_bcast && L.cout % 4 == 0 &&
        !sw.on(SW_NO_SPLITK)) {
        // enough splits for ~two workgroups per CU (measured 256 ... 768 at batch 1 / 4 and on one End_to_End stack: 512 is 3-4 %
        // faster than the earlier floor(256 / n), which left 129 ... 192-workgroup launches unsplit)
        const int want = (sw.ksplit_target + t.total_tiles * t.nsplit - 1) / (t.total_tiles * t.nsplit);
        t.ksplit = std::max(1, std::min(std::min(tp.nstage, want), 8));
        // the same split INSIDE the workgroup where a team configuration covers it (round 6): the teams' partial sums meet in LDS, no partials through
        // memory and no splitk_finish launch (5-6 us each behind 28 of a batch-1 forward's 89 launches)
        const TileCfg *team = (t.ksplit > 1 && !sw.on(SW_NO_TEAMS)) ? tile_cfg_find_team(cfg, tp.nstage, cfg->nt) : nullptr;
        if (team) {
            // ... unless the team launch needs several rounds of workgroups (their LDS images allow one or two per CU, and next to the other streams'
            // kernels they take whole CUs): measured per layer at batch 1 / 2 / 4, profiles/r06_batch1_teams.txt
            const int64_t wgs = team_wgs(team, t.nsplit, 1);
            if (wgs < sw.team_min_wgs || wgs > sw.team_max_wgs) team = nullptr;
        }
        if (team) {
            cfg = team;
            t.ksplit = 1;
            set_tiles(cfg);
        }
        if (t.ksplit > 1) {
            t.partial_stride = p.M_out * (int64_t)pc.nt * 16;
            p.partial_bytes = t.ksplit * t.partial_stride * (int64_t)sizeof(float);
            p.finish_bytes = (double)p.M_out * L.cout * (4.0 * t.ksplit + eb * (o.res0 ? 2 : 1));
        }
    }
    // the pixel-pair stem on whole tiles from the fp32 stack: the persistent pipelined kernel (dffw_stem.hip)
    // (stem_pipe has no tile timeline: a traced stem runs on conv_tile)
    p.stem_pipe = stem_pair && !sw.on(SW_NO_STEM_PIPE) && !sw.tracing(name) && stem_pipe_ok(prec, cfg, a, t);
    p.family = F_TILE;
    p.cfg = cfg;
    p.n = 1;
    ConvLaunch &l = p.l[0];
    l.a = a;
    l.suffix = "";
    l.flops = flops;
    l.bytes = in_b + (o.outf ? opx * L.cout * 4.0 : out_b(o.out_pre ? 2 : 1)) + out_b(res(o.res0) + res(o.res1)) + w_b((double)L.kd * L.kh * L.kw);
    if (p.stem_pipe) stem_pipe_kernel_name(a, l.kernel, sizeof l.kernel);
    else conv_tile_kernel_name(prec, cfg, a, t, l.kernel, sizeof l.kernel);
}

// the gather kernels (conv_igemm / conv_small): one launch per variant (a regular conv, or one sub-pixel phase of a transposed one)
void Planner::gather(ConvPlan &p) {
    p.family = F_GATHER;   // (pack_conv makes one variant, or the 2 x 2 sub-pixel phases of a transposed layer: ConvPlan::l holds them)
    for (const Variant &v : pc.variants) {
        a.KC = v.KC;
        a.tab = v.tab;
        a.wpk = v.wpk;
        if (L.transposed) {
            a.Ng = in0.N; a.Hg = in0.H; a.Wg = in0.W;
            a.sy = a.sx = 1;
            a.osy = a.osx = 2;
            a.ooy = v.ooy; a.oox = v.oox;
        } else {
            a.Ng = No; a.Hg = Ho; a.Wg = Wo;
            a.sy = L.sh; a.sx = L.sw;
            a.osy = a.osx = 1;
            a.ooy = a.oox = 0;
        }
        a.M = (int64_t)a.B * a.Ng * a.Hg * a.Wg;
        if (sw.on(SW_NO_SMALL)) a.dbg |= DFFW_ARGS_NO_SMALL;
        ConvLaunch &l = p.l[p.n++];
        l.a = a;
        l.suffix = "";
        conv_kernel_name_for(prec, a, l.kernel, 64);
        const double nv = (double)pc.variants.size();
        const double px = (double)a.M;  // output pixels written by this launch
        l.flops = 2.0 * (double)a.M * v.ntaps * L.cin * L.cout;
        l.bytes = in_b / nv   // input volume read once per layer
                  + px * L.cout * (o.outf ? 4.0 : eb * (o.out_pre ? 2 : 1))
                  + px * L.cout * eb * (res(o.res0) + res(o.res1))
                  + (double)v.ntaps * L.cin * L.cout * eb;
    }
}

// The decision.  `cls`: the packed 1x1x1 layer named by o.cls (null: there is none); `out`: the output volume's geometry and pointer
void plan_conv(const std::string &name, const PackedConv &pc, const PackedConv *cls, const Act &in0, const ConvOpt &o, const Act &out, const Switches &sw,
               int prec, ConvPlan &p) {
    const LayerDef &L = pc.def;
    const int No = out.N, Ho = out.H, Wo = out.W;
    auto reject = [&](const char *fmt, const char *x, const char *y) {
        p.err = DFFW_EINVAL;
        snprintf(p.msg, sizeof p.msg, fmt, x, y);
    };
    if (o.cls && (!cls || !cls->w32 || cls->def.cin != L.cout || cls->def.cout != 1)) return reject("cannot fuse classifier %s into %s", o.cls, name.c_str());
    if (o.res_bcast && !(L.kd == 1 && L.kh == 3 && !L.transposed && L.sh == 1 && L.cout >= 16))
        return reject("slice-broadcast residual is only implemented for the per-slice 1x3x3 convs (layer %s)%s", name.c_str(), "");

    const double eb = 2.0 * prec_parts(prec);
    Planner pl{name, pc, L, in0, o, sw, prec, out, ConvArgs(), No, Ho, Wo, pc.cin_all, eb, (double)out.B * No * Ho * Wo, (double)in0.pixels() * L.cin * eb};
    ConvArgs &a = pl.a;
    memset(&a, 0, sizeof a);
    a.in0 = in0.p;
    a.C0 = in0.C;
    a.in1 = o.in1 ? o.in1->p : in0.p;
    a.C1 = o.in1 ? o.in1->C : 0;
    a.B = in0.B; a.Ni = in0.N; a.Hi = in0.H; a.Wi = in0.W;
    a.No = No; a.Ho = Ho; a.Wo = Wo;
    a.Cout = L.cout;
    a.bias = pc.bias;
    a.res0 = o.res0 ? o.res0->p : nullptr;
    a.res1 = o.res1 ? o.res1->p : nullptr;
    a.res_bcast = o.res_bcast ? 1 : 0;
    a.out = out.p;
    a.out_pre = o.out_pre ? o.out_pre->p : nullptr;
    a.outf = o.outf;
    a.fs32 = o.fs32;
    a.outf_ch = o.outf_ch;
    a.outf_plane = (int64_t)No * Ho * Wo;
    a.cls_w = cls ? cls->w32 : nullptr;
    a.cls_out = o.cls_out;
    a.relu = o.relu;
    a.dbg = (sw.debug_flags & 6) | sw.path_bits();   // ablation switches (2 no MFMA loop, 4 no stores) + the launchers' path switches
    if (o.raw) a.dbg |= DFFW_ARGS_RAW;   // fs32 then points to the RawStack descriptor in device memory
    if (o.sums) {
        if (!conv_sums_ok(pc, sw, in0.B, in0.N, in0.H, in0.W) || o.relu != 1 || o.res0 || o.res1 || o.cls || o.out_pre || o.in1)
            return reject("layer %s has no row-sums kernel for this shape / epilogue%s", name.c_str(), "");
        a.outf = o.sums;
        a.dbg |= DFFW_ARGS_SUMS;
    }

    for (pl.fam = 0; pl.fam < kStreamBeforeStemPair; ++pl.fam)
        if ((pl.*kStream[pl.fam].plan)(p)) return;
    // the stem straight from the focal stack: pixel-pair form (half the MFMAs and LDS reads of the per-pixel kernel)
    const bool stem_pair = o.fs32 && pc.tile_pair.cfg && pc.bias_pair && Wo % pc.tile_pair.cfg->tx == 0 && Ho % pc.tile_pair.cfg->ty == 0 &&
                           !sw.on(SW_NO_STEM_PAIR);
    if (stem_pair) a.bias = pc.bias_pair;
    for (; pl.fam < kStreamCount; ++pl.fam)
        if ((pl.*kStream[pl.fam].plan)(p)) return;

    const int gW = L.transposed ? in0.W : Wo, gH = L.transposed ? in0.H : Ho;
    // the 5 x 8 x 8 block (its packs of layers with more than 4 output tiles split the output channels over grid.y: not with a fused classifier,
    // whose partial dot spans all of a pixel's channels, nor under DFFW_NO_SPLIT), with enough samples / tiles to fill the chip:
    // (a) grids at most 8 x 8 (the 1/32-resolution pyramid layers at 256 x 256, round 4);  (b) round 5: stride-1 layers with 128 output channels on grids up to
    // DFFW_NARROW_MAX (40) wide -- End_to_End's 30 x 40 pyramid level at batch 8: `combine2` / `conv4` ran on the 4 x 4 x 8 block with all 128 output
    // channels per workgroup, re-streaming the filter for 128 grid points at a time (0.24 -> 0.13 ms, `conv4` 0.16 -> 0.09; the 64-output layers of those levels gain 2-8 % on it at that shape and lose as much at others: left alone)
    const bool narrow_splits = pc.tile_narrow.cfg && pc.nt > pc.tile_narrow.cfg->nt;
    const int gN = L.transposed ? in0.N : No;
    bool narrow = !stem_pair && pc.tile_narrow.cfg && !sw.on(SW_NO_NARROW) && !(narrow_splits && (o.cls || sw.on(SW_NO_SPLIT))) &&
                  (int64_t)in0.B * ((gN + 4) / 5) * ((gH + 7) / 8) * ((gW + 7) / 8) * pc.nt >= 256;
    if (narrow && !(gW <= 8 && gH <= 8)) narrow = !L.transposed && pc.nt >= 8 && gW <= sw.narrow_max && gH <= sw.narrow_max;
    const TilePack &tp = stem_pair ? pc.tile_pair : (narrow ? pc.tile_narrow : pc.tile);
    // small grids (the low-resolution pyramid at batch 1): conv_small's one-workgroup-per-(16 points, 16 channels) split of the
    // whole layer beats an LDS tile that a few workgroups walk stage by stage (+ a split-K finish launch)
    const int64_t small_units = ((int64_t)in0.B * gN * gH * gW + 15) / 16 * pc.nt;
    const bool prefer_small = small_units <= sw.small_max_units && !o.cls && !o.fs32 && !sw.on(SW_NO_SMALL) && !stem_pair;
    const bool use_tile = tp.cfg && !sw.on(SW_NO_TILE) && gW * 2 >= tp.cfg->tx && gH * 2 >= tp.cfg->ty &&
                          in0.C % 8 == 0 && (!o.in1 || o.in1->C % 8 == 0) && !prefer_small;
    if (use_tile) pl.tile(p, tp, stem_pair, gH, gW);
    else pl.gather(p);
}

}  // namespace

Act Run::conv(const std::string &name, const Act &in0, const ConvOpt &o) {
    Act out;
    if (!ok()) return out;
    auto it = e->convs.find(name);
    if (it == e->convs.end()) {
        err = fail(DFFW_EINVAL, "no packed layer %s", name.c_str());
        return out;
    }
    const PackedConv &pc = it->second;
    const LayerDef &L = pc.def;
    const int cin = in0.C + (o.in1 ? o.in1->C : 0);
    if (cin != pc.cin_all) {
        err = fail(DFFW_EINVAL, "layer %s expects %d input channels, got %d", name.c_str(), pc.cin_all, cin);
        return out;
    }
    int Ho, Wo;
    if (L.transposed) {
        Ho = in0.H * 2;
        Wo = in0.W * 2;
    } else {
        const int win = (L.kh == 9 && L.cin == 3) ? in0.W - 2 : in0.W;  // stem input is the (W+2)-wide paired volume
        Ho = (in0.H + 2 * L.ph - L.dh * (L.kh - 1) - 1) / L.sh + 1;
        Wo = (win + 2 * L.pw - L.dw * (L.kw - 1) - 1) / L.sw + 1;
    }
    const int No = in0.N + 2 * L.pd - (L.kd - 1);
    if (o.outf == nullptr && !o.discard && !o.sums) out = act(in0.B, No, Ho, Wo, L.cout);
    else { out.B = in0.B; out.N = No; out.H = Ho; out.W = Wo; out.C = L.cout; }
    if (o.out_pre) *o.out_pre = act(in0.B, No, Ho, Wo, L.cout);
    if (!ok()) return out;

    const PackedConv *cls = nullptr;
    if (o.cls) {
        auto ic = e->convs.find(o.cls);
        if (ic != e->convs.end()) cls = &ic->second;
    }
    ConvPlan p;
    plan_conv(name, pc, cls, in0, o, out, sw, e->prec, p);
    if (p.err != DFFW_OK) {
        err = fail(p.err, "%s", p.msg);
        return out;
    }
    // (the dry run that sizes the workspace comes this far: split-K adds a scratch block)
    float *partial = p.partial_bytes ? (float *)raw(p.partial_bytes) : nullptr;
    if (!ok()) return out;
    if (dry) {
        drop_raw(partial);
        return out;
    }

    const uint16_t *zero = zero_page();
    if (!zero) return out;
    if (p.clear_scores) check(hipMemsetAsync(o.cls_out, 0, (size_t)out.pixels() * 4, s), "score memset");
    // debug timeline of one layer (DFFW_TRACE_LAYER=<layer name> DFFW_TRACE_OUT=<file>): conv_tile writes 8 x u64 per tile (s_memtime at start / fill issued /
    // fill landed / contraction done / stores acknowledged, HW_ID), conv_roll its step timeline, the others none
    const StreamFamily *f = p.family < kStreamCount ? &kStream[p.family] : nullptr;
    const size_t trace_words = p.family == F_TILE ? (size_t)p.t.total_tiles * 8 : (f && f->step_trace) ? STEP_TRACE_WORDS : 0;
    p.t.partial = partial;
    for (int i = 0; i < p.n; ++i) {
        ConvLaunch &l = p.l[i];
        l.a.zero = zero;
        launch(l.kernel, name, l.suffix, l.flops, l.bytes, name.c_str(), trace_words, [&](unsigned long long *trace) {
            l.a.trace = trace;
            if (f) return f->go(e->prec, l, s);
            if (p.family == F_GATHER) return launch_conv(e->prec, l.a, s);
            return p.stem_pipe ? launch_stem_pipe(l.a, p.t, sw.roll_wgs, s) : launch_conv_tile(e->prec, p.cfg, l.a, p.t, s);
        });
    }
    if (partial) {
        launch_unnamed("dffw::splitk_finish_kernel", name, " (split-K finish)", 0.0, p.finish_bytes, "splitk_finish", 0, [&](unsigned long long *) {
#if defined(DFFW_ABL_BUILD) && defined(DFFW_EXP_SKIP_FINISH)   // (dev-only timing bound, tools/build_variant_lib.sh: what a split-K without its finish launch could save at most; results are garbage)
            return hipSuccess;
#endif
            return launch_splitk_finish(e->prec, partial, p.t.ksplit, p.t.partial_stride, p.M_out, pc.nt * 16, L.cout, pc.bias, p.l[0].a.res0, o.relu, out.p, s);
        });
        drop_raw(partial);
    }
    trace_end();
    return out;
}

}  // namespace dffw
