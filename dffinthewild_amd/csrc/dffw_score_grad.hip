// Backward of the score convs: Conv3d(Cin, 1, 1) and Conv3d(Cin, 1, 3, padding=1), stride 1, no bias -- the four convs that produce
// the fp32 score volumes conf, cost1, cost2, cost3 the training loss differentiates.
//
//   grad_x[b,n,y,x,c]  = sum_{kz,ky,kx} w[c,kz,ky,kx] g[b, n+1-kz, y+1-ky, x+1-kx]  (+ b[b,n,y,x,c])     taps outside the volume contribute 0
//   grad_w[c,kz,ky,kx] = sum_{b,n,y,x}  g[b,n,y,x] x[b, n+kz-1, y+ky-1, x+kx-1, c]                        x: the stored record value
//
// With one output channel there is no matrix product: the data gradient is an outer product of the fp32 planar g with the filter, the weight
// gradient a reduction over the volume.  Plain HIP in §14's frame: records move as 16-byte accesses, a thread owns one octet of channels, units are
// dealt by the persistent-grid rule of dffw_persist.h.  k111: a unit is 512 consecutive pixels.  k333: a unit is a TY x TX tile of one slice of one
// sample; its halo of g (3 slices x (TY + 2) x (TX + 2)) goes to LDS with everything outside the volume written as zero, so no tap ever reads the
// neighbouring sample, slice, row or column.  The weight gradients keep float64 sums of the exact products g * x per thread, add them over the
// workgroup in a fixed order and store them to the workgroup's own slot of the workspace (a plain store, also without a unit: the workspace need
// not be cleared); the finish kernel adds the slots in workgroup order.  No atomics: two runs give identical bits, and another grid
// (DFFW_SCORE_WGS) changes only the order of float64 additions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_bn.h"
#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"
#include "dffw_score_grad.h"

namespace dffw {

using namespace score;

// a thread's place in a k111 workgroup: octet `o` of the C/8, pixel lane `r` of the `pp` = 256 / (C/8) pixels a pass covers.  C/8 need not be a
// power of two: the 256 - pp * (C/8) threads left over have no pixel lane (`on` is false)
struct ScoreLane {
    int no, o, r, pp;
    bool on;
    __device__ __forceinline__ explicit ScoreLane(int C) {
        no = C >> 3;
        pp = 256 / no;
        o = threadIdx.x % no;
        r = threadIdx.x / no;
        on = r < pp;
    }
};

// this workgroup's pixels, unit by unit, pixel lane by pixel lane: f(pixel) for every pixel of the thread
template <class F>
__device__ __forceinline__ void for_score_pixels(const ScoreArgs &a, const ScoreLane &t, F &&f) {
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int64_t p0 = (int64_t)u * bn::UNIT_PIX, p1 = min((int64_t)a.M, p0 + bn::UNIT_PIX);
#pragma unroll 2
        for (int64_t p = p0 + t.r; p < p1; p += t.pp) f(p);
    }
}

// unit u of a k333 launch: tiles are numbered x fastest, then y, slice, sample
struct ScoreTile {
    int b, n, y0, x0;
    __device__ __forceinline__ ScoreTile(int u, const ScoreArgs &a) {
        const int txi = u % a.tiles_x;
        int tt = u / a.tiles_x;
        const int tyi = tt % a.tiles_y;
        tt /= a.tiles_y;
        n = tt % a.N;
        b = tt / a.N;
        y0 = tyi * TY;
        x0 = txi * TX;
    }
    // element offset of pixel (y, x) of the tile's slice, in pixels
    __device__ __forceinline__ int64_t pixel(const ScoreArgs &a, int y, int x) const { return (((int64_t)b * a.N + n) * a.H + y) * a.W + x; }
};

// the tile's halo of g: slot [dz][hy][hx] holds g[b, n + dz - 1, y0 + hy - 1, x0 + hx - 1], zero outside 0 <= . < N, H, W
__device__ __forceinline__ void load_halo(const ScoreArgs &a, const ScoreTile &t, float *halo) {
    for (int i = threadIdx.x; i < HALO; i += 256) {
        const int dz = i / ((TY + 2) * (TX + 2)), rem = i - dz * ((TY + 2) * (TX + 2));
        const int hy = rem / (TX + 2), hx = rem - hy * (TX + 2);
        const int nn = t.n + dz - 1, y = t.y0 + hy - 1, x = t.x0 + hx - 1;
        float v = 0.f;
        if (nn >= 0 && nn < a.N && y >= 0 && y < a.H && x >= 0 && x < a.W) v = a.g[(((int64_t)t.b * a.N + nn) * a.H + y) * a.W + x];
        halo[i] = v;
    }
}
// g at the offset tap (kz, ky, kx) names for tile pixel (ty, tx): p + 1 - k
__device__ __forceinline__ float halo_at(const float *halo, int ty, int tx, int kz, int ky, int kx) {
    return halo[((2 - kz) * (TY + 2) + (ty + 2 - ky)) * (TX + 2) + (tx + 2 - kx)];
}

// ---- data gradient ----
// k111: out = w g (+ b): one fp32 rounding (w * g, or fmaf(w, g, b)), then the split
template <int PREC, int ADD>
__device__ __forceinline__ void score_dgrad_k111(const ScoreArgs &a) {
    const ScoreLane t(a.C);
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * a.C;
    const int c0 = t.o * 8;
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = a.w[c0 + k];
    if (!t.on) return;   // (no barrier below)
    for_score_pixels(a, t, [&](int64_t p) {
        const int64_t off = p * stride + c0;
        const float gv = a.g[p];
        float v[8];
        if constexpr (ADD) {
            load8<PREC>(a.b + off, a.C, v);   // read before the store: out may alias b
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fmaf(w[k], gv, v[k]);
        } else {
            // (the product is rounded to fp32 before the split: uncontracted, or the split's v - hi would be fused with it into fmaf(w, g, -hi))
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = w[k] * gv;
        }
        store8<PREC>(a.out + off, a.C, v);
    });
}

// k333: a thread computes (pixel, octet) of the tile: 27 fmaf per channel in row-major (kz, ky, kx) order from 0, then + b, then the split
template <int PREC, int ADD>
__device__ __forceinline__ void score_dgrad_k333(const ScoreArgs &a) {
    __shared__ float halo[HALO];
    __shared__ __attribute__((aligned(16))) float wl[27 * MAX_C];   // the filter as [tap][c]: a thread's octet is two 16-byte reads
    const int C = a.C, no = C >> 3;
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * C;
    for (int i = threadIdx.x; i < 27 * C; i += 256) {
        const int tap = i / C, c = i - tap * C;
        wl[i] = a.w[c * 27 + tap];
    }
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const ScoreTile t(u, a);
        __syncthreads();   // the previous unit's reads of the halo are done (first unit: the filter is written)
        load_halo(a, t, halo);
        __syncthreads();
        for (int j = threadIdx.x; j < TILE_PIX * no; j += 256) {
            const int px = j / no, o = j - px * no;
            const int ty = px / TX, tx = px - ty * TX;
            float acc[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 27; ++tap) {
                const float gv = halo_at(halo, ty, tx, tap / 9, (tap / 3) % 3, tap % 3);
                const float4 w0 = *reinterpret_cast<const float4 *>(wl + tap * C + o * 8), w1 = *reinterpret_cast<const float4 *>(wl + tap * C + o * 8 + 4);
                acc[0] = fmaf(w0.x, gv, acc[0]);
                acc[1] = fmaf(w0.y, gv, acc[1]);
                acc[2] = fmaf(w0.z, gv, acc[2]);
                acc[3] = fmaf(w0.w, gv, acc[3]);
                acc[4] = fmaf(w1.x, gv, acc[4]);
                acc[5] = fmaf(w1.y, gv, acc[5]);
                acc[6] = fmaf(w1.z, gv, acc[6]);
                acc[7] = fmaf(w1.w, gv, acc[7]);
            }
            const int y = t.y0 + ty, x = t.x0 + tx;
            if (y < a.H && x < a.W) {   // a ragged tile: its pixels outside the slice are neither read nor stored
                const int64_t off = t.pixel(a, y, x) * stride + o * 8;
                if constexpr (ADD) {
                    float bv[8];
                    load8<PREC>(a.b + off, C, bv);   // read before the store: out may alias b
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] += bv[k];
                }
                store8<PREC>(a.out + off, C, acc);
            }
        }
    }
}

template <int PREC, int K, int ADD>
__global__ __launch_bounds__(256) void score_dgrad_kernel(const ScoreArgs a) {
    static_assert(K == 1 || K == 3, "k111 or k333");
    if constexpr (K == 1) score_dgrad_k111<PREC, ADD>(a);
    else score_dgrad_k333<PREC, ADD>(a);
}

// ---- weight gradient ----
// k111: float64 sums of g * x for the thread's 8 channels (both factors are fp32 values: the product is exact in float64), added over the threads of
// the same octet in a fixed tree -- pixel lane r takes r + h for h = the largest power of two below pp, ..., 1, where r + h is a lane -- and stored
// to the workgroup's slot [C]
template <int PREC>
__device__ __forceinline__ void score_wgrad_k111(const ScoreArgs &a) {
    __shared__ double red[256][8];
    const ScoreLane t(a.C);
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * a.C;
    const int c0 = t.o * 8, tid = threadIdx.x;
    double s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = 0.0;
    if (t.on)
        for_score_pixels(a, t, [&](int64_t p) {
            float v[8];
            load8<PREC>(a.x + p * stride + c0, a.C, v);
            const double gv = (double)a.g[p];
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] = fma(gv, (double)v[k], s[k]);
        });
#pragma unroll
    for (int k = 0; k < 8; ++k) red[tid][k] = s[k];
    int h = 1;
    while (2 * h < t.pp) h *= 2;
    for (; h >= 1; h >>= 1) {
        __syncthreads();
        if (t.on && t.r < h && t.r + h < t.pp) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[tid][k] += red[tid + h * t.no][k];
        }
    }
    if (t.r == 0) {   // its own last addition: no barrier needed
        double *slot = a.partial + (int64_t)blockIdx.x * a.C;
#pragma unroll
        for (int k = 0; k < 8; ++k) slot[c0 + k] = red[tid][k];
    }
}

// k333: the x tile (converted once to fp32; zeros outside a ragged tile's extent) and the halo of g are in LDS.  A thread owns (tap, octet) pairs
// with 8 float64 accumulators each, pair = tap * (C/8) + octet.  Up to 256 pairs (C <= 72): one pair per thread and S = 256 / pairs threads per
// pair, thread `part` of them walks the tile's pixels [part * 64 / S, (part + 1) * 64 / S) in order; the parts are added 0 + 1 + ... + (S - 1).
// More pairs: thread tid owns pairs tid and tid + 256 and walks all 64 pixels.
template <int PREC>
__device__ __forceinline__ void score_wgrad_k333(const ScoreArgs &a) {
    __shared__ float halo[HALO];
    __shared__ __attribute__((aligned(16))) float xs[TILE_PIX * MAX_C];
    __shared__ double red[256][8];
    const int C = a.C, no = C >> 3, tid = threadIdx.x;
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * C;
    const int pairs = 27 * no;
    const bool shared_pairs = pairs <= 256;
    const int S = shared_pairs ? 256 / pairs : 1;
    const int part = shared_pairs ? tid / pairs : 0;
    const int q0 = part * TILE_PIX / S, q1 = (part + 1) * TILE_PIX / S;
    double acc[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[r][k] = 0.0;
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const ScoreTile t(u, a);
        __syncthreads();   // the previous unit's reads are done
        load_halo(a, t, halo);
        for (int j = tid; j < TILE_PIX * no; j += 256) {
            const int px = j / no, o = j - px * no;
            const int ty = px / TX, tx = px - ty * TX;
            const int y = t.y0 + ty, x = t.x0 + tx;
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = 0.f;
            if (y < a.H && x < a.W) load8<PREC>(a.x + t.pixel(a, y, x) * stride + o * 8, C, v);
            *reinterpret_cast<float4 *>(xs + px * C + o * 8) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4 *>(xs + px * C + o * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int pair = shared_pairs ? tid % pairs : tid + 256 * r;
            const bool on = shared_pairs ? (r == 0 && part < S) : pair < pairs;
            if (!on) continue;
            const int tap = pair / no, o = pair - tap * no;
            const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
            for (int q = q0; q < q1; ++q) {
                const double gv = (double)halo_at(halo, q / TX, q % TX, kz, ky, kx);
                const float4 x0 = *reinterpret_cast<const float4 *>(xs + q * C + o * 8), x1 = *reinterpret_cast<const float4 *>(xs + q * C + o * 8 + 4);
                acc[r][0] = fma(gv, (double)x0.x, acc[r][0]);
                acc[r][1] = fma(gv, (double)x0.y, acc[r][1]);
                acc[r][2] = fma(gv, (double)x0.z, acc[r][2]);
                acc[r][3] = fma(gv, (double)x0.w, acc[r][3]);
                acc[r][4] = fma(gv, (double)x1.x, acc[r][4]);
                acc[r][5] = fma(gv, (double)x1.y, acc[r][5]);
                acc[r][6] = fma(gv, (double)x1.z, acc[r][6]);
                acc[r][7] = fma(gv, (double)x1.w, acc[r][7]);
            }
        }
    }
    double *slot = a.partial + (int64_t)blockIdx.x * 27 * C;
    if (shared_pairs) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red[tid][k] = acc[0][k];
        __syncthreads();
        if (tid < pairs) {
            for (int p = 1; p < S; ++p)
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[0][k] += red[tid + p * pairs][k];
            const int tap = tid / no, o = tid - tap * no;
#pragma unroll
            for (int k = 0; k < 8; ++k) slot[tap * C + o * 8 + k] = acc[0][k];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int pair = tid + 256 * r;
            if (pair >= pairs) continue;
            const int tap = pair / no, o = pair - tap * no;
#pragma unroll
            for (int k = 0; k < 8; ++k) slot[tap * C + o * 8 + k] = acc[r][k];
        }
    }
}

template <int PREC, int K>
__global__ __launch_bounds__(256) void score_wgrad_kernel(const ScoreArgs a) {
    static_assert(K == 1 || K == 3, "k111 or k333");
    if constexpr (K == 1) score_wgrad_k111<PREC>(a);
    else score_wgrad_k333<PREC>(a);
}

// grid taps * C / 4: output j = c * taps + tap of grad_w (1,C,kd,kh,kw) is the sum of the workgroups' slots [tap][c] in workgroup order: the wave
// loads 64 slots at a time, lane 0 adds them one by one
__global__ __launch_bounds__(256) void score_wgrad_finish_kernel(const double *__restrict__ partial, int nwg, int C, int taps, float *__restrict__ grad_w) {
    __shared__ double sh[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = blockIdx.x * 4 + wave;
    const int c = j / taps, tap = j - c * taps;
    const int64_t slot = (int64_t)taps * C;
    double S = 0.0;
    for (int base = 0; base < nwg; base += 64) {
        const int w = base + lane;
        const double v = w < nwg ? partial[w * slot + tap * C + c] : 0.0;
        __syncthreads();   // the previous round's reads are done
        sh[wave][lane] = v;
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < 64; ++i) S += sh[wave][i];
    }
    if (lane == 0) grad_w[j] = (float)S;
}

using ScoreRow = KernelRow<ScoreArgs>;
// [precision][k111, k333][add]
static const ScoreRow DGRAD_ROWS[] = {
    DFFW_ROW(256, score_dgrad_kernel, 0, 1, 0), DFFW_ROW(256, score_dgrad_kernel, 0, 1, 1), DFFW_ROW(256, score_dgrad_kernel, 0, 3, 0), DFFW_ROW(256, score_dgrad_kernel, 0, 3, 1),
    DFFW_ROW(256, score_dgrad_kernel, 1, 1, 0), DFFW_ROW(256, score_dgrad_kernel, 1, 1, 1), DFFW_ROW(256, score_dgrad_kernel, 1, 3, 0), DFFW_ROW(256, score_dgrad_kernel, 1, 3, 1),
    DFFW_ROW(256, score_dgrad_kernel, 2, 1, 0), DFFW_ROW(256, score_dgrad_kernel, 2, 1, 1), DFFW_ROW(256, score_dgrad_kernel, 2, 3, 0), DFFW_ROW(256, score_dgrad_kernel, 2, 3, 1),
};
// [precision][k111, k333]
static const ScoreRow WGRAD_ROWS[] = {
    DFFW_ROW(256, score_wgrad_kernel, 0, 1), DFFW_ROW(256, score_wgrad_kernel, 0, 3), DFFW_ROW(256, score_wgrad_kernel, 1, 1),
    DFFW_ROW(256, score_wgrad_kernel, 1, 3), DFFW_ROW(256, score_wgrad_kernel, 2, 1), DFFW_ROW(256, score_wgrad_kernel, 2, 3),
};
static const ScoreRow *dgrad_row(int prec, int k, int add) { return k == 1 || k == 3 ? prec_row(DGRAD_ROWS, prec, 4, (k == 3) * 2 + !!add) : nullptr; }
static const ScoreRow *wgrad_row(int prec, int k) { return k == 1 || k == 3 ? prec_row(WGRAD_ROWS, prec, 2, k == 3) : nullptr; }

const char *score_dgrad_kernel_name(int prec, int k, int add) {
    const ScoreRow *row = dgrad_row(prec, k, add);
    return row ? row->name : nullptr;
}
const char *score_wgrad_kernel_name(int prec, int k) {
    const ScoreRow *row = wgrad_row(prec, k);
    return row ? row->name : nullptr;
}

static int want_of(int wgs) { return wgs > 0 ? wgs : DEFAULT_WGS; }

int score_units(int k, int B, int N, int H, int W) {
    if (k == 1) return (int)(((int64_t)B * N * H * W + bn::UNIT_PIX - 1) / bn::UNIT_PIX);
    return B * N * ((H + TY - 1) / TY) * ((W + TX - 1) / TX);   // at most B*N*H*W
}

unsigned score_grid(int total_units, int wgs) { return persistent_grid(total_units, want_of(wgs)); }

hipError_t launch_score_dgrad(int prec, int k, const ScoreArgs &a, int wgs, hipStream_t s) {
    return launch_row(dgrad_row(prec, k, a.b != nullptr), a.total_units, want_of(wgs), 1, s, a);
}

hipError_t launch_score_wgrad(int prec, int k, const ScoreArgs &a, int wgs, float *grad_w, hipStream_t s) {
    const unsigned grid = score_grid(a.total_units, wgs);
    const int taps = k * k * k;
    return launch_row_then(wgrad_row(prec, k), dim3(grid), a, s, score_wgrad_finish_kernel, taps * a.C / 4, a.partial, (int)grid, a.C, taps, grad_w);
}

}  // namespace dffw
