// What the regression heads' two backward files share (dffw_loss.hip: the heads welded to the training scripts' loss, DESIGN.md 12;
// dffw_heads_grad.hip: the heads under any upstream gradient): one output pixel's view of a low-resolution score plane,
// the weight of an output coordinate in a low-resolution element, the tiles of the gather-form adjoint and the scale of a head.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

constexpr int LOSS_NCH = 10;           // slices whose adjoints of a tile are in LDS at a time

// ---- one output pixel's view of a low-resolution score plane: regress_kernel's index rule and its arithmetic, operation for operation
// (the compiled regress_kernel evaluates hy*u + ly*v with both products rounded and num + f*p with the product rounded; in the first two
// slices of each of its blocks of five u = fma(lx, s01, hx*s00), v = fma(hx, s10, lx*s11), in the other three u = fma(hx, s00, lx*s01),
// v = fma(lx, s11, hx*s10).  Contraction is off in this file and the fused operations are written out, `alt` = slice % 5 >= 2, so that the
// predictions are the bits dffw_op_regress gives; tests/test_gpu_loss.py::test_bit_identity holds the two together) ----
struct Taps {
    int o00, o01, o10, o11;
    float hx, lx, hy, ly;
};
__device__ __forceinline__ Taps make_taps(int X, int Y, int h, int w, float sch, float scw) {
#pragma clang fp contract(off)
    float sy = ((float)Y + 0.5f) * sch - 0.5f;
    float sx = ((float)X + 0.5f) * scw - 0.5f;
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    Taps t;
    t.ly = sy - (float)y0;
    t.lx = sx - (float)x0;
    t.hy = 1.f - t.ly;
    t.hx = 1.f - t.lx;
    t.o00 = y0 * w + x0;
    t.o01 = y0 * w + x1;
    t.o10 = y1 * w + x0;
    t.o11 = y1 * w + x1;
    return t;
}
__device__ __forceinline__ float tap_value(const float *__restrict__ pl, const Taps &t, bool alt) {
#pragma clang fp contract(off)
    const float s00 = pl[t.o00], s01 = pl[t.o01], s10 = pl[t.o10], s11 = pl[t.o11];
    const float u = alt ? __builtin_fmaf(t.hx, s00, t.lx * s01) : __builtin_fmaf(t.lx, s01, t.hx * s00);
    const float v = alt ? __builtin_fmaf(t.lx, s11, t.hx * s10) : __builtin_fmaf(t.hx, s10, t.lx * s11);
    return t.hy * u + t.ly * v;
}
static_assert(LOSS_NCH % 5 == 0, "a slice chunk starts a block of five");
// weight with which output coordinate X (any integer: the footprint of a border tile reaches past the image, where the adjoints are zero)
// enters low-resolution element i along one axis: the sum of its taps that land on i (both, at the clamped far border)
__device__ __forceinline__ float tap_weight(int X, int i, int w, float sc) {
#pragma clang fp contract(off)
    float sx = ((float)X + 0.5f) * sc - 0.5f;
    sx = sx < 0.f ? 0.f : sx;
    const int x0 = (int)sx, x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float lx = sx - (float)x0;
    return (x0 == i ? 1.f - lx : 0.f) + (x1 == i ? lx : 0.f);
}

// tile of the low-resolution grid per scale: footprints of 24x40, 28x32 and 30x32 output pixels (<= 1024 = four per thread)
template <int S> struct LossTile;
template <> struct LossTile<8> { static constexpr int TY = 2, TX = 4; };
template <> struct LossTile<4> { static constexpr int TY = 6, TX = 7; };
template <> struct LossTile<2> { static constexpr int TY = 14, TX = 15; };

static int head_scale(int H, int W, int h, int w) {
    for (int s = 1; s <= 8; s *= 2)
        if ((int64_t)h * s == H && (int64_t)w * s == W) return s;
    return 0;
}
static int64_t tile_count(int s, int h, int w) {
    const int ty = s == 8 ? LossTile<8>::TY : s == 4 ? LossTile<4>::TY : LossTile<2>::TY;
    const int tx = s == 8 ? LossTile<8>::TX : s == 4 ? LossTile<4>::TX : LossTile<2>::TX;
    return (int64_t)((h + ty - 1) / ty) * ((w + tx - 1) / tx);
}

}  // namespace dffw
