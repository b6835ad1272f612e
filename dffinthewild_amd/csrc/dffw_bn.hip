// Train-mode BatchNorm3d on activation records: batch statistics, normalise (+ residual, ReLU), and the backward.
//
//   mean = sum x / M     var = sum (x - mean)^2 / M     invstd = 1 / sqrt(var + eps)         M = B*N*H*W pixels per channel
//   y  = [relu]( (x - mean) * gamma * invstd + beta [+ res] )
//   g  = relu ? gy * [y > 0] : gy      dbeta = sum g      dgamma = invstd * sum g (x - mean)
//   gx = gamma * invstd * ( g - dbeta / M - (x - mean) * invstd * dgamma / M )              grad_res = g
//
// Every kernel streams channels-last records [pixel][part][channel] with 16-byte accesses: a thread owns one octet of channels (tid % (C/8)) and
// walks pixels; a unit is 512 consecutive pixels, dealt to the workgroups by the persistent-grid rule of dffw_persist.h.  The two reductions keep
// float64 sums of the record values (exact in fp32) and of their exact products per thread, add them over the workgroup in a fixed LDS tree and
// store them to the workgroup's own slot of the workspace (a plain store: the workspace need not be cleared); the finish kernels add the slots
// in workgroup order.  No atomics: two runs give identical bits, and another grid (DFFW_BN_WGS) changes only the order of float64 additions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_bn.h"
#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"

namespace dffw {

using namespace bn;

// a thread's place in the workgroup: octet `o` of the C/8, pixel lane `r` of the `pp` = 256 / (C/8) pixels a pass covers
struct BnLane {
    int no, lg, o, r, pp;
    __device__ __forceinline__ explicit BnLane(int C) {
        no = C >> 3;
        lg = __ffs(no) - 1;
        o = threadIdx.x & (no - 1);
        r = threadIdx.x >> lg;
        pp = 256 >> lg;
    }
};

// this workgroup's pixels, unit by unit, pixel lane by pixel lane: f(pixel) for every pixel of the thread
template <class F>
__device__ __forceinline__ void for_pixels(const BnArgs &a, const BnLane &t, F &&f) {
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int64_t p0 = (int64_t)u * UNIT_PIX, p1 = min((int64_t)a.M, p0 + UNIT_PIX);
#pragma unroll 2
        for (int64_t p = p0 + t.r; p < p1; p += t.pp) f(p);
    }
}

// s[0..7] / s[8..15]: the thread's two sums of its 8 channels.  Added over the threads of the same octet in a fixed tree (pixel lane r takes
// r + h for h = pp/2 ... 1), then stored to the workgroup's slot [2][C]
__device__ __forceinline__ void block_sums(const BnArgs &a, const BnLane &t, const double (&s)[16], double (*red)[16]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 16; ++k) red[tid][k] = s[k];
    for (int h = t.pp >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        if (t.r < h) {
#pragma unroll
            for (int k = 0; k < 16; ++k) red[tid][k] += red[tid + h * t.no][k];
        }
    }
    if (t.r == 0) {   // its own last addition: no barrier needed
        double *slot = a.partial + (int64_t)blockIdx.x * 2 * a.C;
#pragma unroll
        for (int k = 0; k < 16; ++k) slot[(k >> 3) * a.C + t.o * 8 + (k & 7)] = red[tid][k];
    }
}

template <int PREC>
__global__ __launch_bounds__(256) void bn_stats_kernel(const BnArgs a) {
    __shared__ double red[256][16];
    const BnLane t(a.C);
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * a.C;
    double s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.0;
    for_pixels(a, t, [&](int64_t p) {
        float v[8];
        load8<PREC>(a.x + p * stride + t.o * 8, a.C, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double d = (double)v[k];
            s[k] += d;
            s[8 + k] = fma(d, d, s[8 + k]);   // d * d is exact in float64
        }
    });
    block_sums(a, t, s, red);
}

// The workgroups' slots of channel c = 4 * blockIdx.x + wave, added in workgroup order: the wave loads 64 slots at a time, lane 0 adds them one by one.
// Returns the two sums in lane 0 (the other lanes get zeros).  Every thread of the block must call it (barriers)
__device__ __forceinline__ void ordered_sums(const double *__restrict__ partial, int nwg, int C, double &S0, double &S1) {
    __shared__ double sh[4][64][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = blockIdx.x * 4 + wave;
    S0 = 0.0;
    S1 = 0.0;
    for (int base = 0; base < nwg; base += 64) {
        const int w = base + lane;
        double v0 = 0.0, v1 = 0.0;
        if (w < nwg) {
            v0 = partial[(int64_t)w * 2 * C + c];
            v1 = partial[(int64_t)w * 2 * C + C + c];
        }
        __syncthreads();   // the previous round's reads are done
        sh[wave][lane][0] = v0;
        sh[wave][lane][1] = v1;
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < 64; ++i) {
                S0 += sh[wave][i][0];
                S1 += sh[wave][i][1];
            }
    }
}

// grid C / 4: save_mean, save_invstd, and the running statistics in place (momentum m, unbiased variance) where given
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double *__restrict__ partial, int nwg, int C, int M, double eps, double m,
                                                               float *running_mean, float *running_var, float *__restrict__ save_mean,
                                                               float *__restrict__ save_invstd) {
    double S0, S1;
    ordered_sums(partial, nwg, C, S0, S1);
    if ((threadIdx.x & 63) != 0) return;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const double mean = S0 / M;
    const double var = fmax(S1 / M - mean * mean, 0.0);
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + eps));
    if (running_mean) running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
    if (running_var) running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (var * M / (M - 1)));
}

// y = [relu]((x - mean) * (gamma * invstd) + beta [+ res]).  The shift stays unfolded: beta - mean * gamma * invstd would cancel against x * gamma * invstd
// with the rounding of the LARGE terms left over (|mean| >> sigma), and a constant channel would not give beta exactly
template <int PREC, int RELU, int RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const BnArgs a) {
    const BnLane t(a.C);
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * a.C;
    const int c0 = t.o * 8;
    float sc[8], mu[8], be[8];   // the thread's channel constants, formed once
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sc[k] = a.gamma[c0 + k] * a.invstd[c0 + k];
        mu[k] = a.mean[c0 + k];
        be[k] = a.beta[c0 + k];
    }
    for_pixels(a, t, [&](int64_t p) {
        const int64_t off = p * stride + c0;
        float v[8], r[8];
        load8<PREC>(a.x + off, a.C, v);
        if constexpr (RES) load8<PREC>(a.in2 + off, a.C, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float z = fmaf(v[k] - mu[k], sc[k], be[k]);
            if constexpr (RES) z += r[k];
            if constexpr (RELU) z = z < 0.f ? 0.f : z;   // (a NaN stays a NaN)
            v[k] = z;
        }
        store8<PREC>(a.out + off, a.C, v);
    });
}

// sum g and sum g (x - mean) per channel, g = gy masked by the STORED y > 0
template <int PREC, int RELU>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const BnArgs a) {
    __shared__ double red[256][16];
    const BnLane t(a.C);
    const int64_t stride = (int64_t)Fmt<PREC>::PARTS * a.C;
    const int c0 = t.o * 8;
    float mu[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) mu[k] = a.mean[c0 + k];
    double s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.0;
    for_pixels(a, t, [&](int64_t p) {
        const int64_t off = p * stride + c0;
        float v[8], g[8], y[8];
        load8<PREC>(a.x + off, a.C, v);
        load8<PREC>(a.in2 + off, a.C, g);
        if constexpr (RELU) load8<PREC>(a.y + off, a.C, y);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float gk = g[k];
            if constexpr (RELU) gk = y[k] > 0.f ? gk : 0.f;
            const double d = (double)gk;
            s[k] += d;
            s[8 + k] = fma(d, (double)(v[k] - mu[k]), s[8 + k]);
        }
    });
    block_sums(a, t, s, red);
}

// grid C / 4: grad_beta = sum g, grad_gamma = invstd * sum g (x - mean)
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double *__restrict__ partial, int nwg, int C, const float *__restrict__ invstd,
                                                             float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    double S0, S1;
    ordered_sums(partial, nwg, C, S0, S1);
    if ((threadIdx.x & 63) != 0) return;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    grad_beta[c] = (float)S0;
    grad_gamma[c] = (float)(S1 * (double)invstd[c]);
}

// gx = gamma invstd (g - dbeta / M - (x - mean) invstd dgamma / M); grad_res = g: the records of grad_y where the mask passes, zeros elsewhere
template <int PREC, int RELU, int RES>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnArgs a) {
    const BnLane t(a.C);
    constexpr int PARTS = Fmt<PREC>::PARTS;
    const int64_t stride = (int64_t)PARTS * a.C;
    const int c0 = t.o * 8;
    float sc[8], mu[8], k1[8], k2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float is = a.invstd[c0 + k];
        sc[k] = a.gamma[c0 + k] * is;
        mu[k] = a.mean[c0 + k];
        k1[k] = (float)((double)a.dbeta[c0 + k] / a.M);
        k2[k] = (float)((double)a.dgamma[c0 + k] * (double)is / a.M);
    }
    for_pixels(a, t, [&](int64_t p) {
        const int64_t off = p * stride + c0;
        float v[8], g[8], y[8];
        load8<PREC>(a.x + off, a.C, v);
        load8<PREC>(a.in2 + off, a.C, g);
        if constexpr (RELU) load8<PREC>(a.y + off, a.C, y);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if constexpr (RELU) g[k] = y[k] > 0.f ? g[k] : 0.f;
            v[k] = fmaf(-(v[k] - mu[k]), k2[k], g[k] - k1[k]) * sc[k];
        }
        store8<PREC>(a.out + off, a.C, v);
        if constexpr (RES) store8<PREC>(a.out2 + off, a.C, g);   // g is a record value: the split gives its parts back
    });
}

// ---- gradient mask-and-add on records: out = [y > 0] a (+ b), the ReLU mask and the fan-in sum of the convs that have no BatchNorm ----
// One thread owns an octet of channels of a pixel (any multiple of 8 channels: the octets of a unit's pixels are dealt to the threads one by one).
// Without b the record of a passes bit for bit (or becomes +0); with b the two record values are added in fp32 and split again.  Every thread reads
// its octet of a, y and b before it writes that octet of out, so out may alias any of them
template <int PREC, int MASK, int ADD>
__global__ __launch_bounds__(256) void grad_combine_kernel(const CombineArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    const int no = a.C >> 3;
    const int64_t stride = (int64_t)PARTS * a.C;
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int64_t p0 = (int64_t)u * UNIT_PIX;
        const int items = (int)min((int64_t)UNIT_PIX, (int64_t)a.M - p0) * no;
#pragma unroll 2
        for (int j = threadIdx.x; j < items; j += 256) {
            const int px = j / no, o = j - px * no;
            const int64_t off = (p0 + px) * stride + o * 8;
            float y[8];
            if constexpr (MASK) load8<PREC>(a.y + off, a.C, y);
            if constexpr (ADD) {
                float v[8], w[8];
                load8<PREC>(a.a + off, a.C, v);
                load8<PREC>(a.b + off, a.C, w);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if constexpr (MASK) v[k] = y[k] > 0.f ? v[k] : 0.f;
                    v[k] += w[k];
                }
                store8<PREC>(a.out + off, a.C, v);
            } else {   // (MASK only: the launcher has no row without both)
                uint32_t m[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) m[k] = (y[2 * k] > 0.f ? 0xFFFFu : 0u) | (y[2 * k + 1] > 0.f ? 0xFFFF0000u : 0u);
#pragma unroll
                for (int part = 0; part < PARTS; ++part) {
                    uint4 r = *reinterpret_cast<const uint4 *>(a.a + off + part * a.C);
                    r.x &= m[0];
                    r.y &= m[1];
                    r.z &= m[2];
                    r.w &= m[3];
                    *reinterpret_cast<uint4 *>(a.out + off + part * a.C) = r;
                }
            }
        }
    }
}

using BnRow = KernelRow<BnArgs>;
// [precision]
static const BnRow STATS_ROWS[] = {DFFW_ROW(256, bn_stats_kernel, 0), DFFW_ROW(256, bn_stats_kernel, 1), DFFW_ROW(256, bn_stats_kernel, 2)};
// [precision][relu][res]
static const BnRow APPLY_ROWS[] = {
    DFFW_ROW(256, bn_apply_kernel, 0, 0, 0), DFFW_ROW(256, bn_apply_kernel, 0, 0, 1), DFFW_ROW(256, bn_apply_kernel, 0, 1, 0), DFFW_ROW(256, bn_apply_kernel, 0, 1, 1),
    DFFW_ROW(256, bn_apply_kernel, 1, 0, 0), DFFW_ROW(256, bn_apply_kernel, 1, 0, 1), DFFW_ROW(256, bn_apply_kernel, 1, 1, 0), DFFW_ROW(256, bn_apply_kernel, 1, 1, 1),
    DFFW_ROW(256, bn_apply_kernel, 2, 0, 0), DFFW_ROW(256, bn_apply_kernel, 2, 0, 1), DFFW_ROW(256, bn_apply_kernel, 2, 1, 0), DFFW_ROW(256, bn_apply_kernel, 2, 1, 1),
};
// [precision][relu]
static const BnRow BWD_REDUCE_ROWS[] = {
    DFFW_ROW(256, bn_bwd_reduce_kernel, 0, 0), DFFW_ROW(256, bn_bwd_reduce_kernel, 0, 1), DFFW_ROW(256, bn_bwd_reduce_kernel, 1, 0),
    DFFW_ROW(256, bn_bwd_reduce_kernel, 1, 1), DFFW_ROW(256, bn_bwd_reduce_kernel, 2, 0), DFFW_ROW(256, bn_bwd_reduce_kernel, 2, 1),
};
// [precision][relu][res]
static const BnRow BWD_APPLY_ROWS[] = {
    DFFW_ROW(256, bn_bwd_apply_kernel, 0, 0, 0), DFFW_ROW(256, bn_bwd_apply_kernel, 0, 0, 1), DFFW_ROW(256, bn_bwd_apply_kernel, 0, 1, 0),
    DFFW_ROW(256, bn_bwd_apply_kernel, 0, 1, 1), DFFW_ROW(256, bn_bwd_apply_kernel, 1, 0, 0), DFFW_ROW(256, bn_bwd_apply_kernel, 1, 0, 1),
    DFFW_ROW(256, bn_bwd_apply_kernel, 1, 1, 0), DFFW_ROW(256, bn_bwd_apply_kernel, 1, 1, 1), DFFW_ROW(256, bn_bwd_apply_kernel, 2, 0, 0),
    DFFW_ROW(256, bn_bwd_apply_kernel, 2, 0, 1), DFFW_ROW(256, bn_bwd_apply_kernel, 2, 1, 0), DFFW_ROW(256, bn_bwd_apply_kernel, 2, 1, 1),
};
static const BnRow *stats_row(int prec) { return prec_row(STATS_ROWS, prec, 1, 0); }
static const BnRow *apply_row(int prec, int relu, int res) { return prec_row(APPLY_ROWS, prec, 4, 2 * !!relu + !!res); }
static const BnRow *bwd_reduce_row(int prec, int relu) { return prec_row(BWD_REDUCE_ROWS, prec, 2, !!relu); }
static const BnRow *bwd_apply_row(int prec, int relu, int res) { return prec_row(BWD_APPLY_ROWS, prec, 4, 2 * !!relu + !!res); }
static const char *name_of(const BnRow *row) { return row ? row->name : nullptr; }

const char *bn_stats_kernel_name(int prec) { return name_of(stats_row(prec)); }
const char *bn_apply_kernel_name(int prec, int relu, int res) { return name_of(apply_row(prec, relu, res)); }
const char *bn_bwd_reduce_kernel_name(int prec, int relu) { return name_of(bwd_reduce_row(prec, relu)); }
const char *bn_bwd_apply_kernel_name(int prec, int relu, int res) { return name_of(bwd_apply_row(prec, relu, res)); }

static int units_of(int M) { return (int)(((int64_t)M + UNIT_PIX - 1) / UNIT_PIX); }
static int want_of(int wgs) { return wgs > 0 ? wgs : DEFAULT_WGS; }

unsigned bn_grid(int M, int wgs) { return persistent_grid(units_of(M), want_of(wgs)); }

hipError_t launch_bn_stats(int prec, const BnArgs &a, int wgs, double eps, double momentum, float *running_mean, float *running_var, float *save_mean,
                           float *save_invstd, hipStream_t s) {
    hipError_t e = launch_row(stats_row(prec), a.total_units, want_of(wgs), 1, s, a);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(a.C / 4), dim3(256), 0, s, (const double *)a.partial, (int)bn_grid(a.M, wgs), a.C, a.M, eps, momentum,
                       running_mean, running_var, save_mean, save_invstd);
    return hipGetLastError();
}

hipError_t launch_bn_apply(int prec, int relu, int res, const BnArgs &a, int wgs, hipStream_t s) {
    return launch_row(apply_row(prec, relu, res), a.total_units, want_of(wgs), 1, s, a);
}

hipError_t launch_bn_bwd_reduce(int prec, int relu, const BnArgs &a, int wgs, float *grad_gamma, float *grad_beta, hipStream_t s) {
    hipError_t e = launch_row(bwd_reduce_row(prec, relu), a.total_units, want_of(wgs), 1, s, a);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(a.C / 4), dim3(256), 0, s, (const double *)a.partial, (int)bn_grid(a.M, wgs), a.C, a.invstd, grad_gamma,
                       grad_beta);
    return hipGetLastError();
}

hipError_t launch_bn_bwd_apply(int prec, int relu, int res, const BnArgs &a, int wgs, hipStream_t s) {
    return launch_row(bwd_apply_row(prec, relu, res), a.total_units, want_of(wgs), 1, s, a);
}

using CombineRow = KernelRow<CombineArgs>;
// [precision][mask only, add only, mask and add]
static const CombineRow COMBINE_ROWS[] = {
    DFFW_ROW(256, grad_combine_kernel, 0, 1, 0), DFFW_ROW(256, grad_combine_kernel, 0, 0, 1), DFFW_ROW(256, grad_combine_kernel, 0, 1, 1),
    DFFW_ROW(256, grad_combine_kernel, 1, 1, 0), DFFW_ROW(256, grad_combine_kernel, 1, 0, 1), DFFW_ROW(256, grad_combine_kernel, 1, 1, 1),
    DFFW_ROW(256, grad_combine_kernel, 2, 1, 0), DFFW_ROW(256, grad_combine_kernel, 2, 0, 1), DFFW_ROW(256, grad_combine_kernel, 2, 1, 1),
};
static const CombineRow *combine_row(int prec, int mask, int add) { return mask || add ? prec_row(COMBINE_ROWS, prec, 3, 2 * !!add + !!mask - 1) : nullptr; }

const char *grad_combine_kernel_name(int prec, int mask, int add) {
    const CombineRow *row = combine_row(prec, mask, add);
    return row ? row->name : nullptr;
}

hipError_t launch_grad_combine(int prec, const CombineArgs &a, int wgs, hipStream_t s) {
    return launch_row(combine_row(prec, a.y != nullptr, a.b != nullptr), a.total_units, want_of(wgs), 1, s, a);
}

}  // namespace dffw
