// Backward of the pools on activation records: the adjoints of pool_kernel (max (1,2,2), average (1,k,k)) and of pool3_kernel
// (the pyramid's three average pools in one pass), each optionally added to a second gradient b of the same tensor.
//
//   max   out[p] = [p is the first maximum of its 2x2 window of the STORED x, row-major (dy, then dx), strict >] g[win(p)]   (+ b[p])
//   avg   out[p] = g[p / k] * k^-2                                                                                          (+ b[p])
//   pyr   out[p] = ((g8[p / 8] * 2^-6 + g4[p / 4] * 2^-4) + g2[p / 2] * 2^-2)                                               (+ b[p])
//
// In the frame of dffw_bn.hip: 16-byte accesses per part and operand, a thread owns one octet of channels, units of bn::UNIT_PIX input pixels
// dealt by persistent_range.  No atomics, no workspace: every element of out is written exactly once, so out need not be cleared, and two
// runs or two grids give identical bits.  Without b a max gradient passes bit for bit (or becomes +0); every sum is formed in fp32 in the
// order written above and split once.  A thread reads everything it needs before its first store, and nobody else touches the pixels it
// writes, so out may alias b.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_bn.h"
#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"
#include "dffw_pool_grad.h"

namespace dffw {

using namespace bn;

// the parts of one octet of one pixel as stored
struct Raw8 {
    uint4 hi, lo;
};
template <int PREC>
__device__ __forceinline__ Raw8 load_raw8(const uint16_t *p, int C) {
    Raw8 r;
    r.hi = *reinterpret_cast<const uint4 *>(p);
    r.lo = make_uint4(0, 0, 0, 0);
    if constexpr (Fmt<PREC>::PARTS == 2) r.lo = *reinterpret_cast<const uint4 *>(p + C);
    return r;
}
template <int PREC>
__device__ __forceinline__ void store_raw8(uint16_t *p, int C, const Raw8 &r) {
    *reinterpret_cast<uint4 *>(p) = r.hi;
    if constexpr (Fmt<PREC>::PARTS == 2) *reinterpret_cast<uint4 *>(p + C) = r.lo;
}
template <int PREC>
__device__ __forceinline__ void join8(const Raw8 &r, float (&v)[8]) {
    Fmt<PREC>::join2(r.hi.x, r.lo.x, v[0], v[1]);
    Fmt<PREC>::join2(r.hi.y, r.lo.y, v[2], v[3]);
    Fmt<PREC>::join2(r.hi.z, r.lo.z, v[4], v[5]);
    Fmt<PREC>::join2(r.hi.w, r.lo.w, v[6], v[7]);
}
template <int PREC>
__device__ __forceinline__ Raw8 split8(const float (&v)[8]) {
    Raw8 r;
    Fmt<PREC>::split2(v[0], v[1], r.hi.x, r.lo.x);
    Fmt<PREC>::split2(v[2], v[3], r.hi.y, r.lo.y);
    Fmt<PREC>::split2(v[4], v[5], r.hi.z, r.lo.z);
    Fmt<PREC>::split2(v[6], v[7], r.hi.w, r.lo.w);
    return r;
}
// the octet another lane of the wave holds (the parts a format does not have stay zero)
template <int PREC>
__device__ __forceinline__ Raw8 shfl_raw8(const Raw8 &r, int src) {
    Raw8 q;
    q.hi = make_uint4(__shfl(r.hi.x, src), __shfl(r.hi.y, src), __shfl(r.hi.z, src), __shfl(r.hi.w, src));
    q.lo = make_uint4(0, 0, 0, 0);
    if constexpr (Fmt<PREC>::PARTS == 2) q.lo = make_uint4(__shfl(r.lo.x, src), __shfl(r.lo.y, src), __shfl(r.lo.z, src), __shfl(r.lo.w, src));
    return q;
}

// max: a work item is (2x2 window, channel octet), a unit UNIT_PIX / 4 consecutive windows: x, b and g are read once, out is written once.
// avg: a work item is (input pixel, channel octet), a unit UNIT_PIX consecutive pixels, as in grad_combine_kernel; the k x k items of a window
// read the same record of g (k of them side by side in one access of the wave, the other rows from the cache).
template <int PREC, int MODE, int K, int ADD>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const PoolGradArgs a) {
    static_assert(MODE == POOL_AVG ? (K == 2 || K == 4 || K == 8) : (MODE == POOL_MAX && K == 2), "max serves k = 2, avg k = 2, 4, 8");
    constexpr int PARTS = Fmt<PREC>::PARTS;
    const int no = a.C >> 3, Wo = a.W / K;
    const int64_t stride = (int64_t)PARTS * a.C;
    const UnitRange rg = persistent_range(a.total_units);
    if constexpr (MODE == POOL_MAX) {
        constexpr int UNIT_WIN = UNIT_PIX / 4;
        const int Mo = a.M >> 2;
        for (int u = rg.first; u < rg.end; u += rg.step) {
            const int w0 = u * UNIT_WIN;
            const int items = min(UNIT_WIN, Mo - w0) * no;
            for (int j = threadIdx.x; j < items; j += 256) {
                const int wl = j / no, o = j - wl * no;
                const int w = w0 + wl;
                const int t = w / Wo, ox = w - t * Wo;          // t = (sample, slice, pooled row): input rows 2t and 2t + 1
                const int64_t p00 = (int64_t)t * 2 * a.W + 2 * ox;
                const int64_t off[4] = {p00 * stride + o * 8, (p00 + 1) * stride + o * 8, (p00 + a.W) * stride + o * 8, (p00 + a.W + 1) * stride + o * 8};
                float v[4][8];
#pragma unroll
                for (int q = 0; q < 4; ++q) load8<PREC>(a.x + off[q], a.C, v[q]);
                const Raw8 g = load_raw8<PREC>(a.g + (int64_t)w * stride + o * 8, a.C);
                Raw8 b[4];
                if constexpr (ADD) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) b[q] = load_raw8<PREC>(a.b + off[q], a.C);
                }
                int first[8];   // the window's first maximum per channel: a later element wins only where it is greater
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float best = v[0][k];
                    first[k] = 0;
#pragma unroll
                    for (int q = 1; q < 4; ++q) {
                        if (v[q][k] > best) {
                            best = v[q][k];
                            first[k] = q;
                        }
                    }
                }
                if constexpr (ADD) {
                    float gv[8];
                    join8<PREC>(g, gv);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float r[8];
                        join8<PREC>(b[q], r);
#pragma unroll
                        for (int k = 0; k < 8; ++k) r[k] = (first[k] == q ? gv[k] : 0.f) + r[k];
                        store8<PREC>(a.out + off[q], a.C, r);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t m[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) m[k] = (first[2 * k] == q ? 0xFFFFu : 0u) | (first[2 * k + 1] == q ? 0xFFFF0000u : 0u);
                        Raw8 r;
                        r.hi = make_uint4(g.hi.x & m[0], g.hi.y & m[1], g.hi.z & m[2], g.hi.w & m[3]);
                        r.lo = make_uint4(g.lo.x & m[0], g.lo.y & m[1], g.lo.z & m[2], g.lo.w & m[3]);
                        store_raw8<PREC>(a.out + off[q], a.C, r);
                    }
                }
            }
        }
    } else {
        constexpr float scale = 1.0f / (float)(K * K);   // a power of two: the product is exact
        for (int u = rg.first; u < rg.end; u += rg.step) {
            const int64_t p0 = (int64_t)u * UNIT_PIX;
            const int items = (int)min((int64_t)UNIT_PIX, (int64_t)a.M - p0) * no;
#pragma unroll 2
            for (int j = threadIdx.x; j < items; j += 256) {
                const int px = j / no, o = j - px * no;
                const int p = (int)p0 + px;
                const int row = p / a.W, xx = p - row * a.W;     // row = (sample, slice) * H + y, and H = K * Ho: the pooled row is row / K
                const int64_t gp = (int64_t)(row / K) * Wo + xx / K;
                const int64_t off = (int64_t)p * stride + o * 8;
                float v[8], w[8];
                load8<PREC>(a.g + gp * stride + o * 8, a.C, v);
                if constexpr (ADD) load8<PREC>(a.b + off, a.C, w);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    v[k] *= scale;
                    if constexpr (ADD) v[k] += w[k];
                }
                store8<PREC>(a.out + off, a.C, v);
            }
        }
    }
}

// pool3_kernel's decomposition: a work item is (8 x 8 block, channel octet) on 8 adjacent lanes, lane dy owns row dy of the block; a unit is
// UNIT_PIX / 64 = 8 consecutive blocks.  The block's 16 + 4 + 1 records of g2, g4, g8 are loaded once -- lanes 0, 2, 4, 6 take a row of g2 each,
// lanes 1 and 5 a row of g4, lane 3 the record of g8 -- and handed round with __shfl (a group's 8 lanes enter and leave the loops together);
// every lane reads its row of b once and writes its row of out once.
template <int PREC, int ADD>
__global__ __launch_bounds__(256) void pool3_bwd_kernel(const Pool3GradArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr int UNIT_BLK = UNIT_PIX / 64;
    const int no = a.C >> 3, W8 = a.W >> 3, nblk = a.M >> 6;
    const int64_t stride = (int64_t)PARTS * a.C;
    const int lane0 = (threadIdx.x & 63) & ~7;   // the group's first lane in the wave
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int b0 = u * UNIT_BLK;
        const int items = min(UNIT_BLK, nblk - b0) * no * 8;
        for (int j = threadIdx.x; j < items; j += 256) {
            const int dy = j & 7, i = j >> 3;
            const int bl = i / no, o = i - bl * no;
            const int blk = b0 + bl;
            const int t = blk / W8, bx = blk - t * W8;       // t = (sample, slice, block row)
            Raw8 ld[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) ld[q].hi = ld[q].lo = make_uint4(0, 0, 0, 0);
            if ((dy & 1) == 0) {          // row dy / 2 of the block's 4 x 4 pixels of g2
                const uint16_t *p = a.g2 + (((int64_t)t * 4 + (dy >> 1)) * (a.W >> 1) + bx * 4) * stride + o * 8;
#pragma unroll
                for (int q = 0; q < 4; ++q) ld[q] = load_raw8<PREC>(p + q * stride, a.C);
            } else if ((dy & 3) == 1) {   // row dy / 4 of the block's 2 x 2 pixels of g4
                const uint16_t *p = a.g4 + (((int64_t)t * 2 + (dy >> 2)) * (a.W >> 2) + bx * 2) * stride + o * 8;
                ld[0] = load_raw8<PREC>(p, a.C);
                ld[1] = load_raw8<PREC>(p + stride, a.C);
            } else if (dy == 3) {
                ld[0] = load_raw8<PREC>(a.g8 + (int64_t)blk * stride + o * 8, a.C);
            }
            const int64_t off = (((int64_t)t * 8 + dy) * a.W + bx * 8) * stride + o * 8;
            Raw8 b[8];
            if constexpr (ADD) {
#pragma unroll
                for (int q = 0; q < 8; ++q) b[q] = load_raw8<PREC>(a.b + off + q * stride, a.C);
            }
            // what this lane's row needs: the record of g8, the 2 records of its row of g4, the 4 of its row of g2
            float s84[2][8], s[4][8], v[8];
            join8<PREC>(shfl_raw8<PREC>(ld[0], lane0 + 3), v);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float g4v[8];
                join8<PREC>(shfl_raw8<PREC>(ld[h], lane0 + (dy & 4) + 1), g4v);
#pragma unroll
                for (int k = 0; k < 8; ++k) s84[h][k] = v[k] * 0.015625f + g4v[k] * 0.0625f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float g2v[8];
                join8<PREC>(shfl_raw8<PREC>(ld[c], lane0 + (dy & 6)), g2v);
#pragma unroll
                for (int k = 0; k < 8; ++k) s[c][k] = s84[c >> 1][k] + g2v[k] * 0.25f;
            }
            if constexpr (ADD) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    join8<PREC>(b[q], v);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = s[q >> 1][k] + v[k];
                    store8<PREC>(a.out + off + q * stride, a.C, v);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {   // two pixels of the row share one record
                    const Raw8 r = split8<PREC>(s[c]);
                    store_raw8<PREC>(a.out + off + (2 * c) * stride, a.C, r);
                    store_raw8<PREC>(a.out + off + (2 * c + 1) * stride, a.C, r);
                }
            }
        }
    }
}

using PoolGradRow = KernelRow<PoolGradArgs>;
// [precision][max 2, avg 2, avg 4, avg 8][add]
#define DFFW_POOL_BWD_ROWS(P)                                                                                                       \
    DFFW_ROW(256, pool_bwd_kernel, P, 0, 2, 0), DFFW_ROW(256, pool_bwd_kernel, P, 0, 2, 1), DFFW_ROW(256, pool_bwd_kernel, P, 1, 2, 0), \
        DFFW_ROW(256, pool_bwd_kernel, P, 1, 2, 1), DFFW_ROW(256, pool_bwd_kernel, P, 1, 4, 0), DFFW_ROW(256, pool_bwd_kernel, P, 1, 4, 1), \
        DFFW_ROW(256, pool_bwd_kernel, P, 1, 8, 0), DFFW_ROW(256, pool_bwd_kernel, P, 1, 8, 1)
static const PoolGradRow POOL_BWD_ROWS[] = {DFFW_POOL_BWD_ROWS(0), DFFW_POOL_BWD_ROWS(1), DFFW_POOL_BWD_ROWS(2)};
static_assert(POOL_MAX == 0 && POOL_AVG == 1, "the rows spell the modes as numerals");

static const PoolGradRow *pool_bwd_row(int prec, int mode, int k, int add) {
    int form;
    if (mode == POOL_MAX && k == 2) form = 0;
    else if (mode == POOL_AVG && (k == 2 || k == 4 || k == 8)) form = k == 2 ? 1 : k == 4 ? 2 : 3;
    else return nullptr;
    return prec_row(POOL_BWD_ROWS, prec, 8, 2 * form + !!add);
}

using Pool3GradRow = KernelRow<Pool3GradArgs>;
// [precision][add]
static const Pool3GradRow POOL3_BWD_ROWS[] = {
    DFFW_ROW(256, pool3_bwd_kernel, 0, 0), DFFW_ROW(256, pool3_bwd_kernel, 0, 1), DFFW_ROW(256, pool3_bwd_kernel, 1, 0),
    DFFW_ROW(256, pool3_bwd_kernel, 1, 1), DFFW_ROW(256, pool3_bwd_kernel, 2, 0), DFFW_ROW(256, pool3_bwd_kernel, 2, 1),
};

static int want_of(int wgs) { return wgs > 0 ? wgs : DEFAULT_WGS; }

const char *pool_bwd_kernel_name(int prec, int mode, int k, int add) {
    const PoolGradRow *row = pool_bwd_row(prec, mode, k, add);
    return row ? row->name : nullptr;
}

hipError_t launch_pool_bwd(int prec, int mode, int k, const PoolGradArgs &a, int wgs, hipStream_t s) {
    return launch_row(pool_bwd_row(prec, mode, k, a.b != nullptr), a.total_units, want_of(wgs), 1, s, a);
}

const char *pool3_bwd_kernel_name(int prec, int add) {
    const Pool3GradRow *row = prec_row(POOL3_BWD_ROWS, prec, 2, !!add);
    return row ? row->name : nullptr;
}

hipError_t launch_pool3_bwd(int prec, const Pool3GradArgs &a, int wgs, hipStream_t s) {
    return launch_row(prec_row(POOL3_BWD_ROWS, prec, 2, a.b != nullptr), a.total_units, want_of(wgs), 1, s, a);
}

}  // namespace dffw
