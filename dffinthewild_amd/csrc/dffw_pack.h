// Weight packing of libdffw.so: a PyTorch conv filter (BatchNorm folded) in the operand layout of every kernel that may
// serve the layer (dffw_pack.cpp), and the device buffers that hold it.
#pragma once
#include <string>
#include <vector>

#include "dffw_conv_tile.h"
#include "dffw_internal.h"

namespace dffw {

struct LayerDef {
    std::string conv, bn;  // state-dict prefixes ("" = no BatchNorm)
    int cin, cout;
    int kd, kh, kw;
    int sh, sw;            // stride over rows/cols (slice stride is always 1 in this network)
    int pd, ph, pw;
    int dh, dw;            // dilation over rows/cols
    bool transposed;       // ConvTranspose3d k3 s(1,2,2) p1 op(0,1,1)
    bool live;
    bool bias;
    std::string shortcut = "";  // prefix of a bias-free 1x1x1 stride-1 conv over a SECOND input whose result is added to this
                                // layer's: folded into this layer's weights as centre-tap columns of a channel concat
    bool folded = false;        // this layer is such a shortcut: it is never launched on its own
    int head_split = 0;         // > 0: first conv of an alignment head over [ref (C) | cur (C) | flow (2)], C = head_split:
                                // also packed as "<name>#ref" (ref channels, BatchNorm scale only) and "<name>#cur" (the rest)
};

// ---- packed conv layer -------------------------------------------------------------------------
struct Tap {
    int dz, dy, dx;  // input offset
    int kz, ky, kx;  // which filter element
};

struct Variant {      // one launch: a regular conv, or one sub-pixel phase of a transposed conv
    int KC = 0;
    int ntaps = 0;
    int ooy = 0, oox = 0;
    TapEntry *tab = nullptr;  // device
    uint16_t *wpk = nullptr;  // device
};

struct TilePack {            // weights/taps in conv_tile's order (per pass: [stage][KC][NT][part][64][8])
    const TileCfg *cfg = nullptr;
    int nstage = 0;
    int npass = 0;
    int KC[4] = {0, 0, 0, 0};
    int ntaps[4] = {0, 0, 0, 0};
    int ooy[4] = {0, 0, 0, 0}, oox[4] = {0, 0, 0, 0};
    int *tab[4] = {nullptr, nullptr, nullptr, nullptr};
    uint16_t *wpk[4] = {nullptr, nullptr, nullptr, nullptr};
};

// The device pointers below borrow from `owned`: every buffer pack_conv uploads is listed there once, and free_packed frees that list.
struct PackedConv {
    LayerDef def;
    std::vector<void *> owned;
    std::vector<size_t> owned_bytes;   // size of owned[i]
    int nt = 1;
    float *bias = nullptr;  // device, nt*16 floats
    std::vector<Variant> variants;
    TilePack tile;
    TilePack tile_narrow;   // 3x3x3 stride-1 / transposed layers once more on the 5 x 8 x 8 block (grids at most 8 wide, Run::conv decides per call)
    TilePack tile_pair;     // the stem once more, for the pixel-pair kernel (G2P); bias_pair = its BatchNorm shift for both pixels' rows
    float *bias_pair = nullptr;
    float *w32 = nullptr;  // device fp32 [kz][cin][cout] (BatchNorm folded) for kh = kw = 1 layers: fused VALU kernels
    float *whead = nullptr;   // device fp32: the last conv of an alpha head (biased 1x3x3, 3 outputs) as [3][cin][9] weights then [3] bias,
                              // for head_tail_finish_kernel (conv + plane mean collapsed into plane sums)
    uint16_t *wroll = nullptr;  // device: the filter in conv_roll's fragment order (3x3x3 stride 1, 16 input channels, <= 16 outputs)
    bool roll_pair = false;     // ... packed for its pixel-pair variant (<= 8 output channels)
    uint16_t *wroll_k2 = nullptr;  // device: a 3x3x3 stride-1 32 -> 16 filter in conv_rollx_k2's order: [input half][conv_roll's 15 chunks]
    uint16_t *wslice32 = nullptr;  // device: a 1x3x3 32 -> 32 filter in conv_slice32's order: [9 taps][output tile][part]
    bool slice_cat = false;        // wslice64 holds a 32 -> 32 filter + folded 1x1x1 shortcut over a second 32-channel tensor in conv_slice32_cat's order
    uint16_t *wslice64 = nullptr;  // device: a 1x3x3 64 -> 64 filter in conv_slice64's order: [output tile][chunk = tap * 2 + channel half][part]; or (a 34 -> 64 `#cur` layer of
                                   // an alignment head) in its HEAD order: [output tile][9 feature chunks + 3 chunks over the flow octet][part]
    uint16_t *wrollk = nullptr;    // device: a 3x3x3 stride-1 32 / 64 -> 32 / 64 filter in conv_rollk's order: [32-channel output pair][wave][7 chunks][output tile]
    uint16_t *wrollt = nullptr;    // device: a transposed 3x3x3 32 / 64 -> 32 / 64 filter in conv_rollt's order: [32-channel output half][wave][rollt::MAXU units][part]
    uint16_t *wroll_t = nullptr;   // device: the filter in conv_roll_t's order (transposed 3x3x3, 16 -> 8 channels)
    uint16_t *wroll8 = nullptr;    // device: a 3x3x3 8 -> 16 filter (stride 1 or (1,2,2)) in conv_roll_efd's order
    uint16_t *wroll_s2 = nullptr;  // device: a 3x3x3 stride-(1,2,2) 16 -> 16 / 32 filter in conv_roll_s2's order (15 chunks per 16-channel output tile)
    uint16_t *wroll15 = nullptr;   // device: a 3x3x3 stride-1 16 -> 32 filter in the same order (the pooled branch of the fused 16-channel EFD block, conv_efd16)
    uint16_t *wroll_t32 = nullptr; // device: a transposed 3x3x3 32 -> 16 filter in conv_roll_t32's order (row phase 0: 9 chunks, then phase 1: 18)
    uint16_t *wsrd = nullptr;      // device: a 1x3x3 8 -> 8 filter in srd_roll's order (3 chunks of 4 taps x 8 channels)
    uint16_t *watt = nullptr;      // device: an 8 -> 8 attention conv (3x1x1 or 1x1x1) as srd_roll's stage-C fragments
    int cin_all = 0;       // input channels the packed layer contracts over: own (padded to 8) + folded shortcut's (padded to 8)
};

void free_packed(PackedConv &pc);

// weight: PyTorch layout.  bn: gamma|beta|mean|var (4*cout) or null.  conv_bias: cout or null.
// shortcut_w: (cout, shortcut_cin) weights of a folded 1x1x1 shortcut over a second input, or null.
int pack_conv(const LayerDef &L, int prec, const float *weight, const float *bn, const float *conv_bias,
              PackedConv &pc, const float *shortcut_w = nullptr, int shortcut_cin = 0);
// The two halves of a layer with head_split > 0 (and a BatchNorm): `ref` = "<name>#ref" over the first head_split input channels with the
// BatchNorm scale only, `cur` = "<name>#cur" over the rest with the whole BatchNorm.  weight, bn: the whole layer's, as for pack_conv.
int pack_head_split(const LayerDef &L, int prec, const float *weight, const float *bn, PackedConv &ref, PackedConv &cur);

}  // namespace dffw
