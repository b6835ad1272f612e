// Weight gradient of the 3x3x3 / 1x3x3 convs of the aggregation network, stride 1 or (1,2,2), and of the transposed 3x3x3:
//
//   dW[co][ci][kz][ky][kx] = sum over (b, n, y, x) of g[b, n, y, x, co] * f[b, n + kz - pz, S*y + ky - 1, S*x + kx - 1, ci]
//
// The contraction runs over PIXELS while both tensors are channels-last records [pixel][part][channel], so both MFMA operands are read transposed
// out of LDS with ds_read_b64_tr_b16: a 16-lane group reads 4 pixels x 16 channels, two reads make a lane's 8 contraction values of a 32-deep
// v_mfma_f32_16x16x32 step.  A workgroup (4 waves) owns one slice tap, one 16-channel tile of g and one 32-channel group of f (grid.y), walks units
// of 4 x 16 grid points by the persistent-grid rule of dffw_persist.h, stages the unit's g tile and f footprint in LDS (register fills, zero
// outside the volume and beyond the channels: padded, never masked) and keeps its 16 x 32 x 9 block of the filter in fp32 accumulators, the
// (column tile, in-plane tap) items dealt round-robin to the waves.  Every FLUSH_UNITS units at the latest the accumulators are added, in float64,
// into the workgroup's own block of the workspace (first flush: a plain store, so the workspace need not be cleared); conv_wgrad_finish sums the
// workgroups' blocks in float64 in workgroup order.  No atomics anywhere: two runs give identical bits.
//
// The step and the flush are dffw_tr_read.h's (mma3, flush_f64).  The lane map is tr_lane()'s too, but spelled out here: through the helper the
// stride-2 instantiations compile to other machine code than the measured one (profiles/grad_refactor_isa.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_conv_wgrad.h"
#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"
#include "dffw_tr_read.h"

namespace dffw {

using namespace wgrad;

template <int PREC, int S>
struct WgradLds {
    static constexpr int PARTS = Fmt<PREC>::PARTS;
    static constexpr int FY = S * (TY - 1) + 3, FX = S * (TX - 1) + 3;   // the footprint of a unit: 6 x 18, or 9 x 33 at stride 2
    // row (= pixel) strides in bytes.  A 32-lane half reads 8 consecutive grid points x 32 bytes: conflict-free where the 8 rows fall on the 8
    // 32-byte slots of a 256-byte bank row, i.e. (S * stride) / 32 odd
    static constexpr int G_PART = CO_T * 2, F_PART = CI_G * 2;
    static constexpr int G_ROW = PARTS == 1 ? 32 : 96;
    static constexpr int F_ROW = S == 1 ? (PARTS == 1 ? 96 : 160) : (PARTS == 1 ? 80 : 144);
    static_assert(G_ROW >= PARTS * G_PART && F_ROW >= PARTS * F_PART && G_ROW % 16 == 0 && F_ROW % 16 == 0, "rows hold their parts, 16-byte stores stay aligned");
    static_assert((G_ROW / 32) % 2 == 1 && G_ROW % 32 == 0 && (S * F_ROW) % 32 == 0 && (S * F_ROW / 32) % 2 == 1, "8 consecutive grid points on 8 distinct 32-byte slots");
    static constexpr int G_BYTES = TY * TX * G_ROW, F_BYTES = FY * FX * F_ROW;
};

template <int PREC, int S>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
    using L = WgradLds<PREC, S>;
    constexpr int PARTS = L::PARTS, FX = L::FX, FY = L::FY;
    constexpr int NJ = (2 * 9 + 3) / 4;   // items (column tile, tap) of a wave
    __shared__ __attribute__((aligned(16))) char lds_g[L::G_BYTES];
    __shared__ __attribute__((aligned(16))) char lds_f[L::F_BYTES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // grid.y: slice tap, 16-channel tile of g, 32-channel group of f
    int yy = blockIdx.y;
    const int cig = yy % a.ncig;
    yy /= a.ncig;
    const int cot = yy % a.ncot, kz = yy / a.ncot;
    const int cf_here = min(CI_G, a.Cf - cig * CI_G), nitems = (cf_here + 15) / 16 * 9;
    const int Hf = S * a.Hg, Wf = S * a.Wg;

    // this lane's piece of a transposed read: row q of the group's 4, channels 4p .. 4p + 3; the group's 4 grid points are columns
    // 8r + 4(group & 1) + 0..3 of tile row 2c + (lane >> 5) for read r of chunk c
    const int q = (lane >> 2) & 3, p = lane & 3, half = lane >> 5, gl = (lane >> 4) & 1;   // (tr_lane(): see the head of the file)
    const int col0 = 4 * gl + q;
    const char *const ga = lds_g + (half * TX + col0) * L::G_ROW + p * 8;
    const char *const fa = lds_f + (S * half * FX + S * col0) * L::F_ROW + p * 8;

    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    double *const blk = a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * BLOCK;
    bool first = true;
    int since = 0;
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int item = wave + 4 * j;
            if (item < nitems) {
                const int t = item / 9, tap = item - t * 9;
#pragma unroll
                for (int r = 0; r < 4; ++r) flush_f64(blk + (((lane >> 4) * 4 + r) * CI_G + t * 16 + (lane & 15)) * 9 + tap, acc[j][r], first);
            }
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        first = false;
        since = 0;
    };

    const UnitRange rg = persistent_range(a.total_tiles);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int txi = u % a.tiles_x;
        int tt = u / a.tiles_x;
        const int tyi = tt % a.tiles_y;
        tt /= a.tiles_y;
        const int n = tt % a.N, b = tt / a.N;
        const int nf = n + kz - a.pz;
        if (nf < 0 || nf >= a.N) continue;   // the slice padding: this tap sees zeros (uniform over the workgroup)
        const int gy0 = tyi * TY, gx0 = txi * TX;
        __syncthreads();   // the previous unit's reads are done
        {   // g tile: TY * TX pixels x PARTS x 2 octets
            const uint16_t *gp = a.g + ((int64_t)b * a.N + n) * a.Hg * a.Wg * (PARTS * a.Cg);
            for (int i = tid; i < TY * TX * PARTS * 2; i += 256) {
                const int oct = i & 1, part = (i >> 1) % PARTS, px = i / (2 * PARTS);
                const int gy = gy0 + px / TX, gx = gx0 + px % TX, ch = cot * CO_T + oct * 8;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (gy < a.Hg && gx < a.Wg && ch < a.Cg) v = *reinterpret_cast<const uint4 *>(gp + ((int64_t)gy * a.Wg + gx) * (PARTS * a.Cg) + part * a.Cg + ch);
                *reinterpret_cast<uint4 *>(lds_g + px * L::G_ROW + part * L::G_PART + oct * 16) = v;
            }
        }
        {   // f footprint: FY * FX pixels x PARTS x 4 octets
            const uint16_t *fp = a.f + ((int64_t)b * a.N + nf) * Hf * Wf * (PARTS * a.Cf);
            for (int i = tid; i < FY * FX * PARTS * 4; i += 256) {
                const int oct = i & 3, part = (i >> 2) % PARTS, px = i / (4 * PARTS);
                const int fy = S * gy0 - 1 + px / FX, fx = S * gx0 - 1 + px % FX, ch = cig * CI_G + oct * 8;
                uint4 v = make_uint4(0, 0, 0, 0);
                if ((unsigned)fy < (unsigned)Hf && (unsigned)fx < (unsigned)Wf && ch < a.Cf)
                    v = *reinterpret_cast<const uint4 *>(fp + ((int64_t)fy * Wf + fx) * (PARTS * a.Cf) + part * a.Cf + ch);
                *reinterpret_cast<uint4 *>(lds_f + px * L::F_ROW + part * L::F_PART + oct * 16) = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < TY / 2; ++c) {
            short8 ag[PARTS];
#pragma unroll
            for (int part = 0; part < PARTS; ++part) {
                const char *g0 = ga + (2 * c * TX) * L::G_ROW + part * L::G_PART;
                ag[part] = tr_pair(g0, g0 + 8 * L::G_ROW);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int item = wave + 4 * j;
                if (item < nitems) {   // uniform over the wave: every lane of a transposed read is active
                    const int t = item / 9, tap = item - t * 9, ky = tap / 3, kx = tap - ky * 3;
                    short8 bf[PARTS];
#pragma unroll
                    for (int part = 0; part < PARTS; ++part) {
                        const char *f0 = fa + ((S * 2 * c + ky) * FX + kx) * L::F_ROW + part * L::F_PART + t * 32;
                        bf[part] = tr_pair(f0, f0 + 8 * S * L::F_ROW);
                    }
                    acc[j] = mma3<PREC>(ag, bf, acc[j]);
                }
            }
        }
        if (++since >= a.flush_units) flush();
    }
    flush();   // also with nothing summed: every block of the workspace is written
}

// The same sum for the 3x3x3 stride-1 conv whose input is the channel concatenation of two record tensors a (Ca channels) and b (Cb channels) of
// one volume, never materialised: conv_wgrad_kernel<PREC, 1> with kd = 3, pz = 1 and Cf = Ca + Cb, its footprint fill choosing the
// source per octet.  Channel ch of the concatenation is a's channel ch at a's row pitch PARTS * Ca below Ca, b's channel ch - Ca at b's row pitch
// PARTS * Cb below Ca + Cb, and zero beyond; Ca is a multiple of 8, so no octet straddles the switch.  Everything after the fill is the same text.
// It is a copy and not a __device__ template shared with conv_wgrad_kernel: merely called through a function, that kernel's six instantiations
// compile to other machine code than the measured one (profiles/conv_wgrad_cat_isa.txt).
template <int PREC>
__global__ __launch_bounds__(256) void conv_wgrad_cat_kernel(const WgradCatArgs a) {
    constexpr int S = 1;
    using L = WgradLds<PREC, S>;
    constexpr int PARTS = L::PARTS, FX = L::FX, FY = L::FY;
    constexpr int NJ = (2 * 9 + 3) / 4;   // items (column tile, tap) of a wave
    __shared__ __attribute__((aligned(16))) char lds_g[L::G_BYTES];
    __shared__ __attribute__((aligned(16))) char lds_f[L::F_BYTES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // grid.y: slice tap, 16-channel tile of g, 32-channel group of f
    int yy = blockIdx.y;
    const int cig = yy % a.ncig;
    yy /= a.ncig;
    const int cot = yy % a.ncot, kz = yy / a.ncot;
    const int Cf = a.Ca + a.Cb, cf_here = min(CI_G, Cf - cig * CI_G), nitems = (cf_here + 15) / 16 * 9;
    const int Hf = S * a.Hg, Wf = S * a.Wg;

    // this lane's piece of a transposed read: row q of the group's 4, channels 4p .. 4p + 3; the group's 4 grid points are columns
    // 8r + 4(group & 1) + 0..3 of tile row 2c + (lane >> 5) for read r of chunk c
    const int q = (lane >> 2) & 3, p = lane & 3, half = lane >> 5, gl = (lane >> 4) & 1;   // (tr_lane(): see the head of the file)
    const int col0 = 4 * gl + q;
    const char *const ga = lds_g + (half * TX + col0) * L::G_ROW + p * 8;
    const char *const fa = lds_f + (S * half * FX + S * col0) * L::F_ROW + p * 8;

    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    double *const blk = a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * BLOCK;
    bool first = true;
    int since = 0;
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int item = wave + 4 * j;
            if (item < nitems) {
                const int t = item / 9, tap = item - t * 9;
#pragma unroll
                for (int r = 0; r < 4; ++r) flush_f64(blk + (((lane >> 4) * 4 + r) * CI_G + t * 16 + (lane & 15)) * 9 + tap, acc[j][r], first);
            }
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        first = false;
        since = 0;
    };

    const UnitRange rg = persistent_range(a.total_tiles);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int txi = u % a.tiles_x;
        int tt = u / a.tiles_x;
        const int tyi = tt % a.tiles_y;
        tt /= a.tiles_y;
        const int n = tt % a.N, b = tt / a.N;
        const int nf = n + kz - 1;
        if (nf < 0 || nf >= a.N) continue;   // the slice padding: this tap sees zeros (uniform over the workgroup)
        const int gy0 = tyi * TY, gx0 = txi * TX;
        __syncthreads();   // the previous unit's reads are done
        {   // g tile: TY * TX pixels x PARTS x 2 octets
            const uint16_t *gp = a.g + ((int64_t)b * a.N + n) * a.Hg * a.Wg * (PARTS * a.Cg);
            for (int i = tid; i < TY * TX * PARTS * 2; i += 256) {
                const int oct = i & 1, part = (i >> 1) % PARTS, px = i / (2 * PARTS);
                const int gy = gy0 + px / TX, gx = gx0 + px % TX, ch = cot * CO_T + oct * 8;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (gy < a.Hg && gx < a.Wg && ch < a.Cg) v = *reinterpret_cast<const uint4 *>(gp + ((int64_t)gy * a.Wg + gx) * (PARTS * a.Cg) + part * a.Cg + ch);
                *reinterpret_cast<uint4 *>(lds_g + px * L::G_ROW + part * L::G_PART + oct * 16) = v;
            }
        }
        {   // f footprint: FY * FX pixels x PARTS x 4 octets, each from the source its channel lies in
            const int64_t plane = ((int64_t)b * a.N + nf) * Hf * Wf;
            const uint16_t *const pa = a.f_a + plane * (PARTS * a.Ca), *const pb = a.f_b + plane * (PARTS * a.Cb);
            for (int i = tid; i < FY * FX * PARTS * 4; i += 256) {
                const int oct = i & 3, part = (i >> 2) % PARTS, px = i / (4 * PARTS);
                const int fy = S * gy0 - 1 + px / FX, fx = S * gx0 - 1 + px % FX, ch = cig * CI_G + oct * 8;
                const bool in_a = ch < a.Ca;
                const uint16_t *const src = in_a ? pa : pb;
                const int C = in_a ? a.Ca : a.Cb, c = in_a ? ch : ch - a.Ca;   // the source's channels and the octet's first channel in it
                uint4 v = make_uint4(0, 0, 0, 0);
                if ((unsigned)fy < (unsigned)Hf && (unsigned)fx < (unsigned)Wf && c < C)
                    v = *reinterpret_cast<const uint4 *>(src + ((int64_t)fy * Wf + fx) * (PARTS * C) + part * C + c);
                *reinterpret_cast<uint4 *>(lds_f + px * L::F_ROW + part * L::F_PART + oct * 16) = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < TY / 2; ++c) {
            short8 ag[PARTS];
#pragma unroll
            for (int part = 0; part < PARTS; ++part) {
                const char *g0 = ga + (2 * c * TX) * L::G_ROW + part * L::G_PART;
                ag[part] = tr_pair(g0, g0 + 8 * L::G_ROW);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int item = wave + 4 * j;
                if (item < nitems) {   // uniform over the wave: every lane of a transposed read is active
                    const int t = item / 9, tap = item - t * 9, ky = tap / 3, kx = tap - ky * 3;
                    short8 bf[PARTS];
#pragma unroll
                    for (int part = 0; part < PARTS; ++part) {
                        const char *f0 = fa + ((S * 2 * c + ky) * FX + kx) * L::F_ROW + part * L::F_PART + t * 32;
                        bf[part] = tr_pair(f0, f0 + 8 * S * L::F_ROW);
                    }
                    acc[j] = mma3<PREC>(ag, bf, acc[j]);
                }
            }
        }
        if (++since >= a.flush_units) flush();
    }
    flush();   // also with nothing summed: every block of the workspace is written
}

// dW (Cg, Cf, kd, 3, 3) fp32 = the workgroups' blocks summed in float64 in workgroup order, one thread per element
__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(const double *__restrict__ partial, int nwg, int Cg, int Cf, int kd, int ncot, int ncig,
                                                                 float *__restrict__ dw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cg * Cf * kd * 9) return;
    const int tap = e % 9;
    int r = e / 9;
    const int kz = r % kd;
    r /= kd;
    const int ci = r % Cf, co = r / Cf;
    const int y = (kz * ncot + co / CO_T) * ncig + ci / CI_G;
    const double *p = partial + (int64_t)y * nwg * BLOCK + ((co % CO_T) * CI_G + ci % CI_G) * 9 + tap;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += p[(int64_t)w * BLOCK];
    dw[e] = (float)s;
}

using WgradRow = KernelRow<WgradArgs>;
// [precision][stride - 1]
static const WgradRow WGRAD_ROWS[] = {
    DFFW_ROW(256, conv_wgrad_kernel, 0, 1), DFFW_ROW(256, conv_wgrad_kernel, 0, 2),
    DFFW_ROW(256, conv_wgrad_kernel, 1, 1), DFFW_ROW(256, conv_wgrad_kernel, 1, 2),
    DFFW_ROW(256, conv_wgrad_kernel, 2, 1), DFFW_ROW(256, conv_wgrad_kernel, 2, 2),
};
static const WgradRow *select(int prec, int stride) { return stride == 1 || stride == 2 ? prec_row(WGRAD_ROWS, prec, 2, stride - 1) : nullptr; }

const char *conv_wgrad_kernel_name(int prec, int stride) {
    const WgradRow *row = select(prec, stride);
    return row ? row->name : nullptr;
}

unsigned conv_wgrad_grid_x(const WgradArgs &a, int wgs) {
    const int ny = a.kd * a.ncot * a.ncig;
    return persistent_grid(a.total_tiles, std::max(8, (wgs > 0 ? wgs : DEFAULT_WGS) / ny));
}

hipError_t launch_conv_wgrad(int prec, int stride, const WgradArgs &a, unsigned grid_x, float *dw, hipStream_t s) {
    const int ny = a.kd * a.ncot * a.ncig, total = a.Cg * a.Cf * a.kd * 9;
    return launch_row_then(select(prec, stride), dim3(grid_x, ny), a, s, conv_wgrad_finish_kernel, (total + 255) / 256, a.partial, (int)grid_x, a.Cg, a.Cf, a.kd,
                           a.ncot, a.ncig, dw);
}

using WgradCatRow = KernelRow<WgradCatArgs>;
// [precision]
static const WgradCatRow WGRAD_CAT_ROWS[] = {DFFW_ROW(256, conv_wgrad_cat_kernel, 0), DFFW_ROW(256, conv_wgrad_cat_kernel, 1), DFFW_ROW(256, conv_wgrad_cat_kernel, 2)};

const char *conv_wgrad_cat_kernel_name(int prec) {
    const WgradCatRow *row = prec_row(WGRAD_CAT_ROWS, prec, 1, 0);
    return row ? row->name : nullptr;
}

unsigned conv_wgrad_cat_grid_x(const WgradCatArgs &a, int wgs) {
    const int ny = 3 * a.ncot * a.ncig;
    return persistent_grid(a.total_tiles, std::max(8, (wgs > 0 ? wgs : DEFAULT_WGS) / ny));
}

hipError_t launch_conv_wgrad_cat(int prec, const WgradCatArgs &a, unsigned grid_x, float *dw, hipStream_t s) {
    const int Cf = a.Ca + a.Cb, ny = 3 * a.ncot * a.ncig, total = a.Cg * Cf * 3 * 9;
    return launch_row_then(prec_row(WGRAD_CAT_ROWS, prec, 1, 0), dim3(grid_x, ny), a, s, conv_wgrad_finish_kernel, (total + 255) / 256, a.partial, (int)grid_x, a.Cg, Cf,
                           3, a.ncot, a.ncig, dw);
}

}  // namespace dffw
