// Repacking conv weights on the GPU: the contract between the plan the packer records (dffw_pack.cpp), the two kernels of
// dffw_repack.hip and the C ABI of dffw_repack.cpp (dffw_engine_update, dffw_engine_repack_stats, dffw_engine_packed_bytes, dffw_engine_packed_read).
//
// Every weight-derived device buffer of a PackedConv is a fixed function of the layer's parameters.  The FOLD kernel writes, per packed layer,
//     scratch = [ wf: n_w scaled weights | n_sc unscaled shortcut weights | cout shifts | cout raw conv biases (biased layers) ]
// in the host packer's float64 operation order, and the GATHER kernel fills every buffer from that scratch through a source map of int32 indices
// into it (-1: the slot stays zero).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace dffw {

struct LayerDef;

// ---- the plan (host side, recorded by pack_conv in plan mode) -------------------------------------------------------------------------
enum RepackKind {
    RK_CONST = 0,   // no weight in it (tap tables): never rewritten
    RK_FRAGS = 1,   // pack_frags layout [fragment][part][64 lanes][8]: one map entry per (fragment, lane, j), both parts come from it
    RK_SLOTS = 2,   // 16-bit slots written through put(): one entry per slot, 2 * source + part
    RK_F32 = 3,     // fp32 buffer: one entry per float
};
struct BufPlan {
    int kind = RK_CONST;
    size_t bytes = 0;             // size of the device buffer this entry describes
    std::vector<int32_t> map;     // empty for RK_CONST
};
struct LayerPlan {
    std::vector<BufPlan> bufs;    // in PackedConv::owned order
    int64_t n_w = 0, n_sc = 0;    // own weights, folded shortcut's weights
    int cout = 0;
    bool has_bias = false;
    int64_t scratch_floats() const { return n_w + n_sc + cout + (has_bias ? cout : 0); }
};

// ---- FOLD: the layer table travels as the kernel's argument -----------------------------------------------------------------------------
constexpr int FOLD_BLOCK = 256;
constexpr int FOLD_CHUNK = 1024;          // elements of [wf | shortcut] per workgroup; a chunk never spans two layers
constexpr int FOLD_MAX_COUT = 256;        // per-channel scales of a layer live in LDS as doubles
constexpr int FOLD_LAYERS_PER_LAUNCH = 38;
struct FoldLayer {
    const float *w;           // the layer's (or, for an alignment head's #ref / #cur sub-layer, its parent's) weight
    const float *sc;          // folded 1x1x1 shortcut's weight (cout, n_sc / cout), or null
    const float *cb;          // conv bias, or null
    const float *g, *b, *m, *v;   // BatchNorm gamma, beta, running mean, running var; g null: no BatchNorm
    int n_w, n_sc, cout;
    int row;                  // cin * kvol of the packed layer
    int kvol;
    int src_row, src_off;     // element i = (co, r) of the packed layer reads w[co * src_row + src_off + r] (a channel slice of the parent; else row, 0)
    int flags;                // FOLD_TRANSPOSED | FOLD_ZERO_SHIFT
    int scratch_off;          // floats from FoldTable::scratch
    int block_start;          // first workgroup of the layer in this launch
};
constexpr int FOLD_TRANSPOSED = 1;   // ConvTranspose3d weight (cin, cout, kvol): cout(i) = (i / kvol) % cout
constexpr int FOLD_ZERO_SHIFT = 2;   // BatchNorm scale only: beta = mean = 0 (the `#ref` half of a split alignment head)
struct FoldTable {
    FoldLayer layer[FOLD_LAYERS_PER_LAUNCH];
    float *scratch;
    int n_layers;
    int n_blocks;
};
static_assert(sizeof(FoldTable) <= 4096 - 256, "the fold table and the launch's hidden arguments must fit 4 KB of kernarg");

// ---- GATHER: one static device table, built with the plan -----------------------------------------------------------------------------
constexpr int GATHER_BLOCK = 256;
struct GatherJob {
    void *dst;
    const int32_t *map;
    const float *src;      // the layer's scratch
    int units;             // RK_FRAGS: lanes (8 elements each); RK_SLOTS: groups of 8 slots; RK_F32: floats
    int kind;
    int block_start;       // first workgroup of the job; a workgroup never spans two jobs
    int pad;
};
static_assert(sizeof(GatherJob) == 40, "GatherJob is read by the kernel as laid out here");

const char *fold_kernel_name();
const char *gather_kernel_name();
hipError_t launch_repack_fold(const FoldTable &t, hipStream_t s);
hipError_t launch_repack_gather(int prec, const GatherJob *jobs, int n_jobs, int n_blocks, hipStream_t s);

// ---- per engine ---------------------------------------------------------------------------------------------------------------------------
struct RepackLayer {
    std::string name;          // key of dffw_engine::convs
    int64_t scratch_off = 0;   // floats
    LayerPlan plan;            // maps are dropped once uploaded
};
struct RepackPlan {
    std::vector<RepackLayer> layers;   // in dffw_engine::convs order
    std::vector<void *> owned;         // device: scratch, maps, job table
    float *scratch = nullptr;
    int64_t scratch_floats = 0;
    GatherJob *jobs = nullptr;
    int n_jobs = 0, n_blocks = 0;
    int64_t device_bytes = 0;                     // what the plan holds on the device: scratch, maps, job table
    int64_t map_bytes = 0, buffer_bytes = 0;      // what one gather reads (source maps) and writes (every weight-derived buffer)
    int64_t fold_bytes = 0;                       // what the fold launches read (parameters) and write (scratch)
};
void free_repack_plan(RepackPlan *p);

// pack_conv in plan mode for the packed layer `def` (dffw_pack.cpp): which source each slot of each buffer has
int plan_conv(const LayerDef &def, int prec, int shortcut_cin, LayerPlan &out);

// the layer table of a net (dffw_engine.cpp)
const std::vector<LayerDef> &net_layers(int net);

}  // namespace dffw
