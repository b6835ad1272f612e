// Private to the host side of libdffw.so: the workspace arena, the engine object, the DFFW_* switch snapshot and the per-forward
// executor state (Run) that the graphs of dffw_engine.cpp (depth network, C ABI) and dffw_align.cpp (alignment network), the conv
// dispatch of dffw_dispatch.cpp and the single-operator entry points of dffw_ops.cpp share.  No kernel includes this.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/dffw.h"
#include "dffw_align.h"
#include "dffw_conv_roll.h"
#include "dffw_conv_tile.h"
#include "dffw_internal.h"
#include "dffw_pack.h"

// sets dffw_last_conv_kernel() of the calling thread (the thread-local lives in dffw_engine.cpp, as dffw_set_last_op_kernels' does)
void dffw_set_last_conv_kernel(const char *name);

extern "C" char **environ;

namespace dffw {

static constexpr auto &fail = dffw_fail;
// The shape refusals every backward family shares (defined in dffw_grad.cpp), in this order: precision, a dimension below 1, a channel count that
// is no multiple of 8 from 8 to 128 (`channels`: {Cin, Cout}, {C}, or {} for a family with fixed channels), H or W no multiple of `div`, and
// `units` -- the largest count the family's kernels hold in an int, from the family's own unit size -- beyond 31 bits.  DFFW_OK, or the error set
int check_volume(const char *family, int precision, int B, int N, int H, int W, std::initializer_list<int> channels, int div, int64_t units, const char *unit);

// is p a multiple of n (a power of two)?  A null pointer is
inline bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return dffw::fail(DFFW_EHIP, "%s -> %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// ---- workspace arena ---------------------------------------------------------------------------
// Offsets into the caller's workspace; first-fit with coalescing.  The graph is static for a given
// (B,N,H,W), so a dry run of the same code computes the exact peak (dffw_workspace_bytes).
class Arena {
  public:
    explicit Arena(int64_t cap = INT64_MAX) { free_.push_back({0, cap}); }
    int64_t alloc(int64_t bytes) {
        bytes = (bytes + 255) & ~(int64_t)255;
        for (size_t i = 0; i < free_.size(); ++i) {
            if (free_[i].second >= bytes) {
                const int64_t off = free_[i].first;
                free_[i].first += bytes;
                free_[i].second -= bytes;
                if (free_[i].second == 0) free_.erase(free_.begin() + i);
                live_[off] = bytes;
                peak_ = std::max(peak_, off + bytes);
                return off;
            }
        }
        return -1;
    }
    void release(int64_t off) {
        auto it = live_.find(off);
        if (it == live_.end()) return;
        std::pair<int64_t, int64_t> blk{off, it->second};
        live_.erase(it);
        auto pos = std::lower_bound(free_.begin(), free_.end(), blk);
        pos = free_.insert(pos, blk);
        size_t i = pos - free_.begin();
        if (i + 1 < free_.size() && free_[i].first + free_[i].second == free_[i + 1].first) {
            free_[i].second += free_[i + 1].second;
            free_.erase(free_.begin() + i + 1);
        }
        if (i > 0 && free_[i - 1].first + free_[i - 1].second == free_[i].first) {
            free_[i - 1].second += free_[i].second;
            free_.erase(free_.begin() + i);
        }
    }
    int64_t peak() const { return peak_; }

  private:
    int64_t peak_ = 0;
    std::vector<std::pair<int64_t, int64_t>> free_;
    std::map<int64_t, int64_t> live_;
};

}  // namespace dffw

// ---- engine ------------------------------------------------------------------------------------
struct ProfRec {
    std::string kernel, layer;
    double flops = 0, bytes = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

namespace dffw {
struct RepackPlan;   // dffw_repack.h: where every slot of every packed buffer comes from (built at the first dffw_engine_update)
void free_repack_plan(RepackPlan *p);
}  // namespace dffw

struct dffw_engine {
    int device = 0, net = 0, prec = 0;
    std::map<std::string, dffw::PackedConv> convs;
    dffw::RepackPlan *repack = nullptr;
    bool profiling = false;
    std::vector<ProfRec> recs;
    uint16_t *zero_page = nullptr;  // 256 zero bytes: what out-of-volume LDS-DMA lanes read
    // side streams + events for the small-shape regime, where single launches cannot fill the chip and the
    // independent branches of the graph (pyramid scales, regression heads) run next to the main chain
    static constexpr int NSIDE = 2, NEV = 16;
    hipStream_t side[NSIDE] = {nullptr, nullptr};
    hipEvent_t ev[NEV] = {};
    int ensure_side() {
        if (side[0]) return DFFW_OK;
        for (int i = 0; i < NSIDE; ++i) HIPCHK(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
        for (int i = 0; i < NEV; ++i) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        return DFFW_OK;
    }
    int ensure_zero_page() {
        if (zero_page) return DFFW_OK;
        HIPCHK(hipMalloc((void **)&zero_page, 256));
        HIPCHK(hipMemset(zero_page, 0, 256));
        return DFFW_OK;
    }
    void clear_recs() {
        for (auto &r : recs) {
            if (r.e0) (void)hipEventDestroy(r.e0);
            if (r.e1) (void)hipEventDestroy(r.e1);
        }
        recs.clear();
    }
    ~dffw_engine() {
        clear_recs();
        if (zero_page) (void)hipFree(zero_page);
        for (int i = 0; i < NSIDE; ++i)
            if (side[i]) (void)hipStreamDestroy(side[i]);
        for (int i = 0; i < NEV; ++i)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        for (auto &kv : convs) dffw::free_packed(kv.second);
        dffw::free_repack_plan(repack);
    }
};

namespace dffw {

inline bool getenv_flag(const char *name) {
    const char *v = getenv(name);
    return v && *v && *v != '0';
}

// The DFFW_* kernel-path switches, read from the environment ONCE per forward (Run's constructor): the
// graph code below never calls getenv itself, so a forward sees one consistent set and pays for one scan of environ.
#define DFFW_SWITCHES(X)                                                                                                 \
    X(NO_CONCURRENT) X(NO_CONF_FORK) X(NO_FUSED_ATTENTION) X(NO_FUSED_EFD) X(NO_FUSED_OF) X(NO_FUSED_POOL) X(NO_FUSED_SRD) \
    X(NO_FUSED_STEM) X(NO_HEAD_SPLIT) X(NO_ROLL) X(NO_ROLL_S2) X(NO_SPLIT) X(NO_SPLITK)  \
    X(NO_STEM_PAIR) X(NO_TILE) X(NO_SMALL) X(NO_ROLL_S2_WIDE) X(NO_HEAD_SUMS) X(NO_HEAD_SUMS_FUSED) X(NO_HEAD_WARP) X(NO_OF_FIRST) \
    X(NO_LEAN_TILE) X(NO_LEAN_ROLL) X(NO_ROLLX) X(NO_ROLLK) X(NO_ROLLT) X(NO_TEAMS) X(NO_SLICE32) X(NO_REGRESS_FUSED) X(NO_STEM_PIPE) X(NO_POOL3) X(NO_NARROW)
enum SwitchId {
#define X_ID(n) SW_##n,
    DFFW_SWITCHES(X_ID)
#undef X_ID
    SW_COUNT
};
// The integer knobs: X(variable, field, lower bound, default).  A value below the lower bound is ignored (the default holds); INT_MIN: any atoi() result is taken.
// The table is the only place that names a knob or its default: it makes the field of Switches, the line of Switches::read() and the entry of the known names.
#define DFFW_INT_KNOBS(X)                                                                                                                                  \
    X(ROLL_WGS, roll_wgs, 8, 0)                                                                                                                            \
    X(SRD_WGS, srd_wgs, 8, 0)                                                                                                                              \
    /* (256 measured 6 % faster on one 5x224x224 stack, level on 10x256x256 -- but a batch-1 call then differs from the same stack inside a batch by      \
       1.5e-5: off) */                                                                                                                                     \
    X(SMALL_MAX_UNITS, small_max_units, 0, 0)                                                                                                              \
    X(ROLL_ZSPLIT, roll_zsplit, 1, 0)                                                                                                                      \
    X(KSPLIT_TARGET, ksplit_target, 1, 512)                                                                                                                \
    /* redir1 / redir2 on the side streams: 1 always, 0 never, unset: from 2M stack pixels */                                                              \
    X(REDIR_SIDE, redir_side, 0, -1)                                                                                                                       \
    X(TEAM_MIN_WGS, team_min_wgs, 0, 0)                                                                                                                    \
    X(TEAM_MAX_WGS, team_max_wgs, 1, 320)                                                                                                                  \
    /* ... and a stride-1 3x3x3 layer with 64 outputs (End_to_End dres16_* at batch 8: 0.093 -> 0.076 ms on two 2-tile workgroups per tile; 257 = round 4) */ \
    X(SPLIT_S64, split_s64, 1, 1025)                                                                                                                       \
    /* tile count below which a transposed layer with 64 outputs splits its output channels (257 = round 4) */                                             \
    X(SPLIT_T64, split_t64, 1, 1025)                                                                                                                       \
    /* widest grid that may take the 5 x 8 x 8 block when its own block leaves the chip short of workgroups (8 = round 4) */                               \
    X(NARROW_MAX, narrow_max, 1, 40)                                                                                                                       \
    /* conv_tile launches of at most this many (tile, channel-split) workgroups touch the weight lines of their whole contraction walk first              \
       (TileArgs::warm; 0: never).  Measured r03 on 10x256x256 stacks, ms per forward at 0 / 256 / 1024 / always: batch 2 1.29 / 1.17 / 1.17 /            \
       1.17, batch 8 2.74 / 2.65 / 2.63 / 2.63, batch 16 4.71 / 4.66 / 4.62 / 4.66, batch 32 8.58 / 8.57 / 8.57 / 8.70 */                                  \
    X(WARM_MAX_WGS, warm_max_wgs, 0, 1024)                                                                                                                 \
    /* conv_rollk layers with 64 outputs on fewer columns than this run their two output halves as ONE launch (grid.y = 2); 1: never.  Round 6, same-run  \
       layer tables at batch 32: the 16 x 16-grid layers (128 columns: one unit per CU) 0.058 -> 0.050-0.054 ms against conv_tile, dres0.0 0.099 ->       \
       0.090, dres0.2 / dres2.conv2 -1..2 % against two launches */                                                                                        \
    X(ROLLK_MERGE_BELOW, rollk_merge_below, 0, 1 << 30)                                                                                                    \
    /* (column, output half) units the transposed streaming kernel conv_rollt needs in its 8-wave forms, 1.5x that in the 4-wave form                     \
       (DFFW_ROLL_MIN_UNITS lowers it too: read() clamps it) */                                                                                            \
    X(ROLLT_MIN_UNITS, rollt_min_units, 1, 128)                                                                                                            \
    /* columns a layer needs for its persistent streaming kernel (measured 16 ... 256 at batch 1 and 4: 192 is 3.6 % faster than 256 on one 5x224x224     \
       stack, level elsewhere; <= 32 slower) */                                                                                                            \
    X(ROLL_MIN_UNITS, roll_min_units, 1, 192)                                                                                                              \
    /* measured best of 64/128/256/512 at batch 1, 4, 8 */                                                                                                 \
    X(SPLIT_WG, split_wg, INT_MIN, 256)                                                                                                                    \
    /* the weight-gradient kernel: workgroups of a launch over grid.x * grid.y (0: its default), and the units a workgroup's fp32          \
       accumulators sum before they are flushed (tests lower both so that one workgroup walks many units and flushes more than once) */                    \
    X(WGRAD_WGS, wgrad_wgs, 8, 0)                                                                                                                          \
    X(WGRAD_FLUSH_UNITS, wgrad_flush_units, 1, 256)                                                                                                        \
    /* ... and the same two of the 3x1x1 / 1x1x1 weight-gradient kernel: workgroups over grid.x * grid.y, and the steps (32 pixels per     \
       accumulator each) between two flushes, which can only be shortened (above 512: 512) */                                                             \
    X(PWGRAD_WGS, pwgrad_wgs, 8, 0)                                                                                                                        \
    X(PWGRAD_FLUSH_STEPS, pwgrad_flush_steps, 1, 512)                                                                                                      \
    /* ... and of the attention tail's fused backward: workgroups of the launch, steps between two flushes (above 512: 512) */              \
    X(ATTGRAD_WGS, attgrad_wgs, 8, 0)                                                                                                                      \
    X(ATTGRAD_FLUSH_STEPS, attgrad_flush_steps, 1, 512)                                                                                                    \
    /* train-mode BatchNorm: workgroups of each of its streaming launches (0: its default; below 8: 8, one per XCD).  Changes only the     \
       order of the float64 additions */                                                                                                                   \
    X(BN_WGS, bn_wgs, 1, 0)                                                                                                                                \
    /* backward of the score convs: workgroups of each of its launches (0: its default, 512; below 8: 8, one per XCD).  Changes only the  \
       order of the float64 additions of the weight gradient */                                                                                           \
    X(SCORE_WGS, score_wgs, 1, 0)                                                                                                                          \
    X(DEBUG_FLAGS, debug_flags, INT_MIN, 0)
// ... and the two 64-bit ones (any atoll() result is taken): X(variable, field, default)
#define DFFW_INT64_KNOBS(X)                                                                                                                                \
    /* < 0: no limit */                                                                                                                                    \
    X(CONCURRENT_MAX_PIXELS, concurrent_max_pixels, -1)                                                                                                    \
    /* below: one stream (a 5x224x224 stack, 0.25M: 0.799 -> 0.785 ms on one stream; 10x256x256, 0.66M: 0.915 -> 0.905 on three) */                        \
    X(CONCURRENT_MIN_PIXELS, concurrent_min_pixels, 400000)

// A DFFW_* variable in the environment that nothing reads (a retired switch, a typo) is reported once per process: a retired switch that is silently ignored turns an
// A/B script into base against base.
inline void warn_unknown_switches() {
    static const bool once = [] {
        static const char *const known[] = {
#define X_NM(n) "DFFW_" #n,
            DFFW_SWITCHES(X_NM)
#undef X_NM
#define X_NM(n, ...) "DFFW_" #n,
            DFFW_INT_KNOBS(X_NM) DFFW_INT64_KNOBS(X_NM)
#undef X_NM
            // read outside the tables: by Switches::read() itself, by the Python loader, the communicator and the benchmark
            "DFFW_SRD_PIPE", "DFFW_TRACE_LAYER", "DFFW_TRACE_OUT", "DFFW_RCCL_LIB", "DFFW_LIB_PATH", "DFFW_NO_PROBE", "DFFW_PRECISION",
            "DFFW_BENCH_ONE_DEVICE", "DFFW_BENCH_TIMEOUT_S",
            // development builds only (make ABL=1 / TRACE=1)
            "DFFW_SRD_ABL", "DFFW_ROLLX_ABL", "DFFW_ROLLX_NTS", "DFFW_ROLLK_ABL", "DFFW_ROLLK_SKEW"};
        for (char **e = ::environ; e && *e; ++e) {
            if (strncmp(*e, "DFFW_", 5) != 0) continue;
            const char *eq = strchr(*e, '=');
            const size_t n = eq ? (size_t)(eq - *e) : strlen(*e);
            bool ok = false;
            for (const char *k : known) ok = ok || (strlen(k) == n && strncmp(k, *e, n) == 0);
            if (!ok) fprintf(stderr, "libdffw: environment variable %.*s is not a switch this library reads (retired or misspelt?) -- ignored\n", (int)n, *e);
        }
        return true;
    }();
    (void)once;
}

struct Switches {
    bool f[SW_COUNT];
#define X_FIELD(n, field, lo, dflt) int field = dflt;
    DFFW_INT_KNOBS(X_FIELD)
#undef X_FIELD
#define X_FIELD(n, field, dflt) int64_t field = dflt;
    DFFW_INT64_KNOBS(X_FIELD)
#undef X_FIELD
    bool srd_pipe = false;   // DFFW_SRD_PIPE=1: the 16-channel SRD block on srd_pipe16 (one barrier per step) instead of srd_roll16
    const char *trace_layer = nullptr, *trace_out = nullptr;
    bool on(int id) const { return f[id]; }
    bool tracing(const std::string &layer) const { return trace_layer && trace_out && layer == trace_layer; }
    // the switches the kernel launchers consult, as ConvArgs::dbg bits (so that no launcher calls getenv)
    int path_bits() const;
    static Switches read() {
        Switches s;
        int i = 0;
#define X_RD(n) s.f[i++] = getenv_flag("DFFW_" #n);
        DFFW_SWITCHES(X_RD)
#undef X_RD
#define X_RD(n, field, lo, dflt) if (const char *z = getenv("DFFW_" #n)) if (atoi(z) >= lo) s.field = atoi(z);
        DFFW_INT_KNOBS(X_RD)
#undef X_RD
#define X_RD(n, field, dflt) if (const char *z = getenv("DFFW_" #n)) s.field = atoll(z);
        DFFW_INT64_KNOBS(X_RD)
#undef X_RD
        s.rollt_min_units = std::min(s.rollt_min_units, s.roll_min_units);
        s.srd_pipe = getenv_flag("DFFW_SRD_PIPE");
        warn_unknown_switches();
        s.trace_layer = getenv("DFFW_TRACE_LAYER");
        s.trace_out = getenv("DFFW_TRACE_OUT");
        return s;
    }
};

inline int Switches::path_bits() const {
    return (f[SW_NO_LEAN_TILE] ? DFFW_ARGS_NO_LEAN_TILE : 0) | (f[SW_NO_LEAN_ROLL] ? DFFW_ARGS_NO_LEAN_ROLL : 0) | (f[SW_NO_ROLLX] ? DFFW_ARGS_NO_ROLLX : 0) |
           (f[SW_NO_ROLLK] ? DFFW_ARGS_NO_ROLLK : 0) | (f[SW_NO_SLICE32] ? DFFW_ARGS_NO_SLICE32 : 0) | (f[SW_NO_ROLLT] ? DFFW_ARGS_NO_ROLLT : 0);
}

struct ConvOpt {
    const Act *in1 = nullptr;
    const Act *res0 = nullptr, *res1 = nullptr;
    bool res_bcast = false;  // res0 has one slice per sample and is added to every output slice
    int relu = 0;
    Act *out_pre = nullptr;  // receives the pre-residual value (allocated here)
    float *outf = nullptr;   // fp32 planar output (B,outf_ch,N,H,W) instead of an activation volume
    int outf_ch = 1;
    const float *fs32 = nullptr;  // stem: read the fp32 focal stack directly (in0 then only carries the geometry)
    bool raw = false;   // stem: fs32 is a device-side RawStack descriptor (raw uint8 / 0..255 stack, normalised and padded on the fly)
    float *sums = nullptr;      // per-slice 1x3x3 conv + ReLU whose result only feeds plane sums: nothing is stored, `sums` receives per output
                                // row segment of 16 pixels [sum | first pixel | last pixel][Cout] fp32 (conv_tile's row-sums variant;
                                // Run::sums_conv_ok() says when it exists; out is not allocated)
    const char *cls = nullptr;  // name of a 1x1x1 C->1 layer to apply to the final value inside the epilogue
    float *cls_out = nullptr;   // its fp32 score volume
    bool discard = false;       // the activation output itself is not needed (only cls_out / out_pre)
};

// does the LDS-tiled kernel serve the layer for an output grid of gH x gW (same test as in plan_conv())?
inline bool conv_tiled(const PackedConv &pc, const Switches &sw, int gH, int gW) {
    const TileCfg *c = pc.tile.cfg;
    return c && !sw.on(SW_NO_TILE) && gW * 2 >= c->tx && gH * 2 >= c->ty;
}
// conv_tile's row-sums variant serves a per-slice layer on a (B,N,H,W) volume: tiled, an instantiation exists, whole row
// segments of 16 pixels, and enough tiles that the plan will not split the output channels over the grid
inline bool conv_sums_ok(const PackedConv &pc, const Switches &sw, int B, int N, int H, int W) {
    if (!conv_tiled(pc, sw, H, W)) return false;
    const TileCfg *c = pc.tile.cfg;
    if (!tile_cfg_has_sums(c) || W % c->tx) return false;
    const int64_t tiles = (int64_t)B * ((N + c->tz - 1) / c->tz) * ((H + c->ty - 1) / c->ty) * (W / c->tx);
    return tiles >= 256;
}

// the RollArgs of one launch of a streaming kernel over tiles_y x tiles_x columns per sample
inline RollArgs roll_args(const uint16_t *filter, int B, int tiles_y, int tiles_x, int zsplit, int wgs, int pair = 0) {
    RollArgs t;
    memset(&t, 0, sizeof t);
    t.wroll = filter;
    t.tiles_y = tiles_y;
    t.tiles_x = tiles_x;
    t.zsplit = zsplit;
    t.total_tiles = B * zsplit * tiles_y * tiles_x;
    t.wgs = wgs;
    t.pair = pair;
    return t;
}

// the SrdArgs of one launch of a fused block kernel over columns of ty x tx pixels of a (B,N,H,W) grid: c0 / c2 are the block's two 1x3x3
// convs; the caller adds what only its kernel reads (pooled, the attention weights, the shortcut, zero).  of_first has no record volume:
// its `x` is null and the caller puts the planar fp32 focal stack into a.w3, which no alignment kernel uses for weights
inline SrdArgs srd_args(const uint16_t *x, uint16_t *out, const PackedConv &c0, const PackedConv &c2, int B, int N, int H, int W, int ty, int tx, int wgs) {
    SrdArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.out = out;
    a.w0 = c0.wsrd; a.w2 = c2.wsrd;
    a.b0 = c0.bias; a.b2 = c2.bias;
    a.B = B; a.N = N; a.H = H; a.W = W;
    a.tiles_y = H / ty; a.tiles_x = W / tx;
    a.total_tiles = B * a.tiles_y * a.tiles_x;
    a.wgs = wgs;
    return a;
}
// ... and the HeadWarpArgs of head_warp over the 8 x 16 columns of the level features `fe`: `ref` the per-sample reference part, `cur` the [cur | flow] filter
inline HeadWarpArgs head_warp_args(const Act &fe, const uint16_t *ref, uint16_t *out, const PackedConv &cur, const float *alpha, const float *fov, int wgs) {
    HeadWarpArgs a;
    memset(&a, 0, sizeof a);
    a.fe = fe.p; a.ref = ref; a.out = out;
    a.w = cur.wsrd; a.bias = cur.bias;
    a.alpha = alpha; a.fov = fov;
    a.B = fe.B; a.N = fe.N; a.H = fe.H; a.W = fe.W;
    a.tiles_y = fe.H / 8; a.tiles_x = fe.W / 16;
    a.total_tiles = fe.B * a.tiles_y * a.tiles_x;
    a.wgs = wgs;
    return a;
}

struct Run {
    dffw_engine *e;
    hipStream_t s;
    Arena arena;
    bool dry;
    char *ws;
    int err = DFFW_OK;
    const dffw_tap *taps = nullptr;
    int n_taps = 0;

    // ---- branch concurrency (small shapes only; decided from the shape alone so that the dry run that sizes the
    // workspace takes the same allocation path).  Inside a forked section buffers are not recycled: a block released
    // after a launch on one stream must not be handed to a launch on another stream that may run earlier.  Outside
    // it recycling continues as usual — measured: running the whole batch-1 forward without recycling costs 17 %
    // (the working set stops fitting the last-level cache). ----
    hipStream_t main_s;
    bool concurrent = false;
    bool forked = false;
    int ev_next = 0;
    unsigned side_open = 0;   // side streams forked and not yet joined
    std::vector<void *> deferred;

    const Switches sw;   // the DFFW_* switches as they were when this forward started

    Run(dffw_engine *e_, hipStream_t s_, bool dry_, char *ws_, int64_t cap)
        : e(e_), s(s_), arena(cap), dry(dry_), ws(ws_), main_s(s_), sw(Switches::read()) {
        // DFFW_DEBUG_FLAGS bit 0 ("no footprint fill") is withdrawn: kernels then contract uninitialised LDS and the run ended in an abort of the
        // whole process (profiles/r04_ablation_conv_tile_phases.txt) -- an error code instead; bits 1 (no MFMA loop) and 2 (no stores) remain
        if (sw.debug_flags & 1) err = fail(DFFW_EINVAL, "DFFW_DEBUG_FLAGS bit 0 (skip the footprint fill) is not supported; use 2 (no MFMA loop), 4 (no stores) or 6");
    }

    bool ok() const { return err == DFFW_OK; }

    void enable_concurrency() {
        concurrent = true;
        if (!dry && ok() && e->ensure_side() != DFFW_OK) err = DFFW_EHIP;
    }
    void fork(int k) {   // side stream k continues from the current point of the main stream
        if (!concurrent || dry || !ok()) return;
        hipEvent_t v = e->ev[ev_next++ % dffw_engine::NEV];
        check(hipEventRecord(v, main_s), "fork record");
        check(hipStreamWaitEvent(e->side[k], v, 0), "fork wait");
        fork_mark(k);
    }
    void on(int k) { s = (concurrent && !dry && k >= 0) ? e->side[k] : main_s; }   // stream of the following launches
    void fork_mark(int k) { side_open |= 1u << k; }
    void join(int k) {   // the main stream waits for everything queued on side stream k
        if (!concurrent || dry || !e->side[k]) return;
        // (also after an error: kernels already queued on the side stream use the workspace, and the caller is free to
        // recycle it as soon as the main stream is done)
        hipEvent_t v = e->ev[ev_next++ % dffw_engine::NEV];
        const hipError_t h1 = hipEventRecord(v, e->side[k]);
        const hipError_t h2 = h1 == hipSuccess ? hipStreamWaitEvent(main_s, v, 0) : h1;
        side_open &= ~(1u << k);
        if (ok()) check(h2, "join");
    }
    ~Run() {   // a forked section left through an error path: join whatever is still open
        for (int k = 0; k < dffw_engine::NSIDE; ++k)
            if (side_open & (1u << k)) join(k);
    }
    void release_deferred() {
        for (void *p : deferred) arena.release(dry ? (int64_t)(uintptr_t)p - 256 : (int64_t)((char *)p - ws));
        deferred.clear();
    }

    void *raw(int64_t bytes) {
        if (!ok()) return nullptr;
        const int64_t off = arena.alloc(bytes);
        if (off < 0) {
            err = fail(DFFW_ENOMEM, "workspace too small (need more than the %lld bytes given)", (long long)bytes);
            return nullptr;
        }
        return dry ? (void *)(uintptr_t)(off + 256) : (void *)(ws + off);
    }
    void drop_raw(void *p) {
        if (!p) return;
        if (forked) {
            deferred.push_back(p);
            return;
        }
        arena.release(dry ? (int64_t)(uintptr_t)p - 256 : (int64_t)((char *)p - ws));
    }
    Act act(int B, int N, int H, int W, int C) {
        Act a;
        a.B = B; a.N = N; a.H = H; a.W = W; a.C = C;
        a.p = (uint16_t *)raw(a.pixels() * prec_parts(e->prec) * C * (int64_t)sizeof(uint16_t));
        return a;
    }
    void drop(Act &a) {
        drop_raw(a.p);
        a.p = nullptr;
    }
    void check(hipError_t h, const char *what) {
        if (ok() && h != hipSuccess) err = fail(DFFW_EHIP, "%s: %s", what, hipGetErrorString(h));
    }
    // bracket one launch with HIP events on the launch stream (profiling mode only); the record's label is layer + suffix
    void prof_begin(const char *kernel, const std::string &layer, double flops, double bytes, const char *suffix = "") {
        if (!e->profiling || dry || !ok()) return;
        ProfRec pr;
        pr.kernel = kernel;
        pr.layer = layer + suffix;
        pr.flops = flops;
        pr.bytes = bytes;
        check(hipEventCreate(&pr.e0), "hipEventCreate");
        check(hipEventCreate(&pr.e1), "hipEventCreate");
        if (ok()) check(hipEventRecord(pr.e0, s), "hipEventRecord");
        e->recs.push_back(pr);
    }
    void prof_end() {
        if (!e->profiling || dry || !ok() || e->recs.empty()) return;
        check(hipEventRecord(e->recs.back().e1, s), "hipEventRecord");
    }
    double elem_bytes() const { return 2.0 * prec_parts(e->prec); }
    // the shell of one kernel launch: the profile record, `go` (the launcher call; two launches that share a record go into one `go`), the record's end.
    // `trace_words` > 0: the launch of a layer named by DFFW_TRACE_LAYER also gets a zeroed timeline of that many u64, handed to go(); the caller's trace_end() writes it out
    template <class Go>
    void launch_unnamed(const char *kernel, const std::string &layer, const char *suffix, double flops, double bytes, const char *what, size_t trace_words, Go &&go) {
        prof_begin(kernel, layer, flops, bytes, suffix);
        unsigned long long *trace = trace_words ? trace_begin(layer, trace_words) : nullptr;
        check(go(trace), what);
        prof_end();
    }
    // ... of a conv or fused-block kernel: dffw_last_conv_kernel() then reports `kernel` (the data movers, reductions and pools go through launch_unnamed)
    template <class Go>
    void launch(const char *kernel, const std::string &layer, const char *suffix, double flops, double bytes, const char *what, size_t trace_words, Go &&go) {
        dffw_set_last_conv_kernel(kernel);
        launch_unnamed(kernel, layer, suffix, flops, bytes, what, trace_words, go);
    }
    // the engine's page of zeros (what out-of-volume LDS-DMA lanes read), made at first use; null with `err` set when that fails
    const uint16_t *zero_page() {
        if (e->ensure_zero_page() != DFFW_OK) err = DFFW_EHIP;
        return ok() ? e->zero_page : nullptr;
    }
    // the packed layer `name`, or null
    const PackedConv *layer(const std::string &name) const {
        auto it = e->convs.find(name);
        return it == e->convs.end() ? nullptr : &it->second;
    }

    // step timeline of a persistent streaming kernel (library built with `make TRACE=1`; DFFW_TRACE_LAYER=<layer> DFFW_TRACE_OUT=<file>):
    // [workgroup][wave][32 steps][8] u64 of s_memtime stamps (StepTrace, dffw_device.h; tools/trace_steps.py)
    unsigned long long *trace_dev = nullptr;
    size_t trace_n = 0;
    static constexpr size_t STEP_TRACE_WORDS = (size_t)1024 * 4 * 32 * 8;   // 1024 workgroups of 4 waves
    unsigned long long *trace_begin(const std::string &layer, size_t words) {
        if (dry || !ok() || !sw.tracing(layer)) return nullptr;
        trace_n = words;
        check(hipMalloc((void **)&trace_dev, trace_n * 8), "trace alloc");
        if (ok()) check(hipMemsetAsync(trace_dev, 0, trace_n * 8, s), "trace memset");
        return ok() ? trace_dev : nullptr;
    }
    void trace_end() {
        if (!trace_dev) return;
        if (ok()) {
            std::vector<unsigned long long> host(trace_n);
            check(hipStreamSynchronize(s), "trace sync");
            check(hipMemcpy(host.data(), trace_dev, trace_n * 8, hipMemcpyDeviceToHost), "trace copy");
            if (FILE *f = fopen(sw.trace_out, "wb")) {
                fwrite(host.data(), 8, host.size(), f);
                fclose(f);
            }
        }
        (void)hipFree(trace_dev);
        trace_dev = nullptr;
    }

    // does the LDS-tiled kernel serve layer `name` for an output grid of gH x gW (same test as in conv())?
    bool tiled(const std::string &name, int gH, int gW) const {
        const PackedConv *pc = layer(name);
        return pc && conv_tiled(*pc, sw, gH, gW);
    }
    bool sums_conv_ok(const std::string &name, int B, int N, int H, int W) const {
        const PackedConv *pc = layer(name);
        return pc && conv_sums_ok(*pc, sw, B, N, H, W);
    }

    Act conv(const std::string &name, const Act &in0, const ConvOpt &o = ConvOpt());   // dffw_dispatch.cpp

    Act pool(const Act &x, int mode, int k) {
        Act out = act(x.B, x.N, x.H / k, x.W / k, x.C);
        if (ok() && !dry) {
            char kn[48];
            snprintf(kn, sizeof kn, "dffw::pool_kernel<%d>", e->prec);
            launch_unnamed(kn, mode == 0 ? "maxpool" : "avgpool", "", 0.0, (double)(x.pixels() + out.pixels()) * x.C * elem_bytes(), "pool", 0,
                           [&](unsigned long long *) { return launch_pool(e->prec, mode, k, x.p, out.p, x.B, x.N, x.H, x.W, x.C, s); });
        }
        return out;
    }
    // the three average pools (1,2,2), (1,4,4), (1,8,8) of x in one pass (pool3_kernel; H and W multiples of 8): the pyramid's and dffw_op_pool3's one launch
    void pool3(const Act &x, Act &p2, Act &p4, Act &p8) {
        p2 = act(x.B, x.N, x.H / 2, x.W / 2, x.C);
        p4 = act(x.B, x.N, x.H / 4, x.W / 4, x.C);
        p8 = act(x.B, x.N, x.H / 8, x.W / 8, x.C);
        if (ok() && !dry) {
            char kn[48];
            snprintf(kn, sizeof kn, "dffw::pool3_kernel<%d>", e->prec);
            launch_unnamed(kn, "avgpool (1,2,2)+(1,4,4)+(1,8,8)", "", 0.0, (double)(x.pixels() + p2.pixels() + p4.pixels() + p8.pixels()) * x.C * elem_bytes(), "pool3", 0,
                           [&](unsigned long long *) { return launch_pool3(e->prec, x.p, p2.p, p4.p, p8.p, x.B, x.N, x.H, x.W, x.C, s); });
        }
    }

    void tap(const char *name, const Act &a) {
        if (!ok() || dry) return;
        for (int i = 0; i < n_taps; ++i)
            if (!strcmp(taps[i].name, name)) {
                const int64_t n = a.pixels() * a.C;
                if (taps[i].numel != n) {
                    err = fail(DFFW_EINVAL, "tap %s holds %lld elements, caller gave %lld", name, (long long)n, (long long)taps[i].numel);
                    return;
                }
                check(launch_to_ncdhw(e->prec, a.p, taps[i].dst, a.B, a.C, a.N, a.H, a.W, s), name);
            }
    }
    void tap_f32(const char *name, const float *p, int64_t n) {
        if (!ok() || dry) return;
        for (int i = 0; i < n_taps; ++i)
            if (!strcmp(taps[i].name, name)) {
                if (taps[i].numel != n) {
                    err = fail(DFFW_EINVAL, "tap %s holds %lld elements, caller gave %lld", name, (long long)n, (long long)taps[i].numel);
                    return;
                }
                check(hipMemcpyAsync(taps[i].dst, p, n * sizeof(float), hipMemcpyDeviceToDevice, s), name);
            }
    }
};

// the graphs: the depth network (dffw_engine.cpp) and, in front of it, the alignment network of End_to_End (dffw_align.cpp)
int run_depth(Run &r, const float *FS, const float *fd, const int64_t fst[4], int B, int N, int H, int W, float *const out[4], const RawStack *raw = nullptr);
int run_e2e(Run &r, const float *FS, const float *fd, const int64_t fst[4], const float *fov, int B, int N, int H, int W, float *const out[4], float *aligned);
Act of_block(Run &r, const std::string &p, const Act &x);
Act of_first_block(Run &r, const std::string &p0, const float *FS, int B, int N, int H, int W);
// the first conv of an alpha head `hp` over [warped ref | warped cur | flow] of the level features fe (consumed), warped by alpha (B,3,N) and
// fov (B,N): y0 = relu(BN(conv)), in the warp, split or whole form (dffw_align.cpp)
Act head_first_conv(Run &r, const std::string &hp, const std::string &label, Act &fe, const float *alpha, const float *fov);
// an alpha head `hp` from its first conv's output y0 (consumed) to alpha += damped plane means, rawh = the undamped ones (`label` names the
// level in the profile); head_tail_stored: its end alone, from a stored y2 (consumed)
void head_tail(Run &r, const std::string &hp, const std::string &label, Act &y0, float *alpha, float *rawh);
void head_tail_stored(Run &r, const std::string &hp, const std::string &label, Act &y2, float *alpha, float *rawh);
// the front end's blocks (dffw_engine.cpp).  srd: pooled (optional) receives max_pool(1,2,2) of the output when the fused kernel writes it on the way;
// efd: pooled (optional) is that copy of x, at hand
Act srd(Run &r, const std::string &p, Act &x, bool drop_x, Act *pooled = nullptr);
Act efd(Run &r, const std::string &p, const Act &x, Act *pooled = nullptr);
// the layers of one block under prefix p, as the layer table of dffw_engine.cpp defines them
std::vector<LayerDef> srd_layers(const std::string &p, int c);
std::vector<LayerDef> efd_layers(const std::string &p, int cin, int cout);
std::vector<LayerDef> of_block_layers(const std::string &p, int cin, int cout, int s);
std::vector<LayerDef> alpha_head_layers(const std::string &p, int cin, int c);

}  // namespace dffw
