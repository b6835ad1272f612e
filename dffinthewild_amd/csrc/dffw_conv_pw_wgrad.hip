// Weight gradient of the convs without in-plane taps, kernel (3,1,1) pad (1,0,0) and kernel (1,1,1):
//
//   dW[co][ci][kz] = sum over (b, n, p) of g[b, n, p, co] * f[b, n + kz - pz, p, ci]        p: flat pixel of the H*W plane
//
// No in-plane halo, so the plane is flat.  A unit is a COLUMN: P = 128 consecutive flat pixels of one sample (the plane's last chunk zero-filled
// beyond H*W: padded, never masked), walked over all N slices by one workgroup of 4 waves.  Per step n the chunk of g[b, n] and the chunk of
// f[b, n + pz] are staged (register fills: 16-byte global loads issued before the step's products, 16-byte LDS stores after them) into LDS, f into
// a ring of KD slots, so every value of g and f is read from memory once per grid.y row and serves all KD slice taps; the taps of slices -1 and N
// are skipped, uniformly over the workgroup.  The contraction is split over the waves: wave w owns pixels 32 w .. 32 w + 31 of the chunk, one
// 32-deep MFMA step per (tap, 16-channel tile of f), both operands through ds_read_b64_tr_b16 with the lane map of conv_wgrad_kernel.  A wave keeps
// KD x <= 2 tiles in fp32 accumulators; every FLUSH_STEPS steps at the latest (16 384 pixels per accumulator) they are added, in float64, into the
// wave's own block of the workspace (first flush: a plain store, so the workspace need not be cleared); conv_pw_wgrad_finish_kernel sums the
// blocks in float64 in (workgroup, wave) order.  No atomics anywhere: two runs give identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_conv_pw_wgrad.h"
#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"
#include "dffw_tr_read.h"

namespace dffw {

using namespace pwgrad;

template <int PREC>
struct PwgradLds {
    static constexpr int PARTS = Fmt<PREC>::PARTS;
    // row (= pixel) strides in bytes.  A 32-lane half of a transposed read covers 8 consecutive pixels x 32 bytes: conflict-free where the 8 rows fall
    // on the 8 32-byte slots of a 256-byte bank row, i.e. stride / 32 odd (the rule of conv_wgrad_kernel; the flat image has no row wrap at all)
    static constexpr int G_PART = CO_T * 2, F_PART = CI_G * 2;
    static constexpr int G_ROW = PARTS == 1 ? 32 : 96, F_ROW = PARTS == 1 ? 96 : 160;
    static_assert(G_ROW >= PARTS * G_PART && F_ROW >= PARTS * F_PART && G_ROW % 16 == 0 && F_ROW % 16 == 0, "rows hold their parts, 16-byte stores stay aligned");
    static_assert((G_ROW / 32) % 2 == 1 && G_ROW % 32 == 0 && (F_ROW / 32) % 2 == 1 && F_ROW % 32 == 0, "8 consecutive pixels on 8 distinct 32-byte slots");
    static constexpr int G_BYTES = P * G_ROW, F_SLOT = P * F_ROW;
};

template <int PREC, int KD>
__global__ __launch_bounds__(256) void conv_pw_wgrad_kernel(const PwgradArgs a) {
    using L = PwgradLds<PREC>;
    static_assert(KD == 1 || KD == 3, "slice taps");
    static_assert(P == 4 * WAVE_PIX, "one 32-pixel chunk per wave and step");
    constexpr int PARTS = L::PARTS, PZ = KD / 2;
    constexpr int NG = P * PARTS * 2 / 256, NF = P * PARTS * 4 / 256;   // 16-byte pieces of a step per thread
    constexpr int BLK = block(KD);
    __shared__ __attribute__((aligned(16))) char lds_g[L::G_BYTES];
    __shared__ __attribute__((aligned(16))) char lds_f[KD * L::F_SLOT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // grid.y: 16-channel tile of g, 32-channel group of f
    const int cig = blockIdx.y % a.ncig, cot = blockIdx.y / a.ncig;
    const int cf_here = min(CI_G, a.Cf - cig * CI_G), nt = (cf_here + 15) / 16;

    // this lane's piece of a transposed read (conv_wgrad_kernel's map on a flat chunk): pixel 32 wave + 16 (lane >> 5) + 4 (group & 1) + q of the
    // first read, 8 pixels on for the second; channels 4p .. 4p + 3
    const auto [q, p, half, gl] = tr_lane(lane);
    const int pix0 = wave * WAVE_PIX + half * 16 + 4 * gl + q;
    const char *const ga = lds_g + pix0 * L::G_ROW + p * 8;
    const char *const fa = lds_f + pix0 * L::F_ROW + p * 8;

    // this thread's staging pieces: pixel of the chunk, part, octet -> LDS offset and offset inside a pixel's record
    int g_px[NG], g_rec[NG], g_lds[NG], f_px[NF], f_rec[NF], f_lds[NF];
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int i = tid + 256 * k, oct = i & 1, part = (i >> 1) % PARTS, ch = cot * CO_T + oct * 8;
        g_px[k] = i / (2 * PARTS);
        g_rec[k] = ch < a.Cg ? part * a.Cg + ch : -1;
        g_lds[k] = g_px[k] * L::G_ROW + part * L::G_PART + oct * 16;
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const int i = tid + 256 * k, oct = i & 3, part = (i >> 2) % PARTS, ch = cig * CI_G + oct * 8;
        f_px[k] = i / (4 * PARTS);
        f_rec[k] = ch < a.Cf ? part * a.Cf + ch : -1;
        f_lds[k] = f_px[k] * L::F_ROW + part * L::F_PART + oct * 16;
    }

    f32x4 acc[KD][2];
#pragma unroll
    for (int kz = 0; kz < KD; ++kz)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[kz][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    double *const blk = a.partial + ((((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * BLK);
    bool first = true;
    int since = 0;
    auto flush = [&]() {
#pragma unroll
        for (int kz = 0; kz < KD; ++kz)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) flush_f64(blk + (((lane >> 4) * 4 + r) * CI_G + t * 16 + (lane & 15)) * KD + kz, acc[kz][t][r], first);
                }
                acc[kz][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        first = false;
        since = 0;
    };

    const int64_t gslice = (int64_t)a.HW * (PARTS * a.Cg), fslice = (int64_t)a.HW * (PARTS * a.Cf);
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int b = u / a.chunks, p0 = (u - b * a.chunks) * P;   // the chunk never leaves its plane: the pixels beyond H*W are zeros
        // slice 0 of the sample; null where the piece is padding (beyond the plane, beyond the channels)
        const uint16_t *gsrc[NG], *fsrc[NF];
#pragma unroll
        for (int k = 0; k < NG; ++k)
            gsrc[k] = g_rec[k] >= 0 && p0 + g_px[k] < a.HW ? a.g + (int64_t)b * a.N * gslice + (int64_t)(p0 + g_px[k]) * (PARTS * a.Cg) + g_rec[k] : nullptr;
#pragma unroll
        for (int k = 0; k < NF; ++k)
            fsrc[k] = f_rec[k] >= 0 && p0 + f_px[k] < a.HW ? a.f + (int64_t)b * a.N * fslice + (int64_t)(p0 + f_px[k]) * (PARTS * a.Cf) + f_rec[k] : nullptr;
        uint4 rgv[NG], rfv[NF];
        // step n stages g[b, n] (n >= 0) and f[b, n + PZ] (below N): global -> registers ...
        auto load = [&](int n) {
            const int nf = n + PZ;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                rgv[k] = make_uint4(0, 0, 0, 0);
                if (n >= 0 && gsrc[k]) rgv[k] = *reinterpret_cast<const uint4 *>(gsrc[k] + n * gslice);
            }
#pragma unroll
            for (int k = 0; k < NF; ++k) {
                rfv[k] = make_uint4(0, 0, 0, 0);
                if (nf < a.N && fsrc[k]) rfv[k] = *reinterpret_cast<const uint4 *>(fsrc[k] + nf * fslice);
            }
        };
        // ... registers -> LDS, f into slot (n + PZ) % KD of the ring
        auto store = [&](int n) {
            const int nf = n + PZ;
            if (n >= 0) {
#pragma unroll
                for (int k = 0; k < NG; ++k) *reinterpret_cast<uint4 *>(lds_g + g_lds[k]) = rgv[k];
            }
            if (nf < a.N) {
                char *slot = lds_f + (nf % KD) * L::F_SLOT;
#pragma unroll
                for (int k = 0; k < NF; ++k) *reinterpret_cast<uint4 *>(slot + f_lds[k]) = rfv[k];
            }
        };
        // (the previous unit ended behind the barrier that follows its last products)
        load(-PZ);
        store(-PZ);
        for (int n = -PZ; n < a.N; ++n) {
            const bool more = n + 1 < a.N;
            if (more) load(n + 1);
            __syncthreads();   // step n's image is complete
            if (n >= 0) {
                short8 ag[PARTS];
#pragma unroll
                for (int part = 0; part < PARTS; ++part) {
                    const char *g0 = ga + part * L::G_PART;
                    ag[part] = tr_pair(g0, g0 + 8 * L::G_ROW);
                }
#pragma unroll
                for (int kz = 0; kz < KD; ++kz) {
                    const int nf = n + kz - PZ;
                    if (nf < 0 || nf >= a.N) continue;   // the slice padding: this tap sees zeros (uniform over the workgroup)
                    const char *fs = fa + (nf % KD) * L::F_SLOT;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        if (t < nt) {   // uniform over the workgroup: every lane of a transposed read is active
                            short8 bf[PARTS];
#pragma unroll
                            for (int part = 0; part < PARTS; ++part) {
                                const char *f0 = fs + part * L::F_PART + t * 32;
                                bf[part] = tr_pair(f0, f0 + 8 * L::F_ROW);
                            }
                            acc[kz][t] = mma3<PREC>(ag, bf, acc[kz][t]);
                        }
                    }
                }
                ++since;
            }
            __syncthreads();   // step n's reads are done: g's image and the ring slot of f[n - PZ] may be overwritten
            if (more) store(n + 1);
            if (since >= a.flush_steps) flush();
        }
    }
    flush();   // also with nothing summed: every block of the workspace is written
}

// dW (Cg, Cf, kd, 1, 1) fp32 = the waves' blocks summed in float64 in (workgroup, wave) order.  One wave per filter element: it loads the element's value
// out of 64 blocks at a time (the default grid has 2 048 of them at 8 -> 8 channels: one thread walking them alone took longer than the contraction),
// lane 0 adds them one by one
__global__ __launch_bounds__(256) void conv_pw_wgrad_finish_kernel(const double *__restrict__ partial, int nblk, int Cg, int Cf, int kd, int ncig,
                                                                    float *__restrict__ dw) {
    __shared__ double sh[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave;
    const bool live = e < Cg * Cf * kd;   // (uniform over the wave; no early return: the barriers below are the whole block's)
    const int ee = live ? e : 0;
    const int kz = ee % kd;
    const int r = ee / kd;
    const int ci = r % Cf, co = r / Cf;
    const int y = (co / CO_T) * ncig + ci / CI_G, blk = block(kd);
    const double *p = partial + (int64_t)y * nblk * blk + ((co % CO_T) * CI_G + ci % CI_G) * kd + kz;
    double s = 0.0;
    for (int base = 0; base < nblk; base += 64) {
        const int w = base + lane;
        const double v = live && w < nblk ? p[(int64_t)w * blk] : 0.0;
        __syncthreads();   // the previous round's reads are done
        sh[wave][lane] = v;
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < 64; ++i) s += sh[wave][i];
    }
    if (live && lane == 0) dw[e] = (float)s;
}

using PwgradRow = KernelRow<PwgradArgs>;
// [precision][kd == 3]
static const PwgradRow PWGRAD_ROWS[] = {
    DFFW_ROW(256, conv_pw_wgrad_kernel, 0, 1), DFFW_ROW(256, conv_pw_wgrad_kernel, 0, 3),
    DFFW_ROW(256, conv_pw_wgrad_kernel, 1, 1), DFFW_ROW(256, conv_pw_wgrad_kernel, 1, 3),
    DFFW_ROW(256, conv_pw_wgrad_kernel, 2, 1), DFFW_ROW(256, conv_pw_wgrad_kernel, 2, 3),
};
static const PwgradRow *select(int prec, int kd) { return kd == 1 || kd == 3 ? prec_row(PWGRAD_ROWS, prec, 2, kd == 3) : nullptr; }

const char *conv_pw_wgrad_kernel_name(int prec, int kd) {
    const PwgradRow *row = select(prec, kd);
    return row ? row->name : nullptr;
}

unsigned conv_pw_wgrad_grid_x(const PwgradArgs &a, int wgs) {
    return persistent_grid(a.total_units, std::max(8, (wgs > 0 ? wgs : DEFAULT_WGS) / (a.ncot * a.ncig)));
}

hipError_t launch_conv_pw_wgrad(int prec, int kd, const PwgradArgs &a, unsigned grid_x, float *dw, hipStream_t s) {
    const int total = a.Cg * a.Cf * kd;
    return launch_row_then(select(prec, kd), dim3(grid_x, a.ncot * a.ncig), a, s, conv_pw_wgrad_finish_kernel, (total + 3) / 4, a.partial, (int)grid_x * 4, a.Cg,
                           a.Cf, kd, a.ncig, dw);
}

}  // namespace dffw
