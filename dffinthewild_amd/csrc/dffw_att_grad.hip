// Backward of the attention tail y = x + relu(conv111(relu(conv311(x)))) in one kernel.  With a = relu(conv311(x)) and
// t = relu(conv111(a)) stored by the forward, p a flat pixel and n a slice:
//
//   gt[co]          = [t[co] > 0] gy[co]
//   ga[ci]          = [a[ci] > 0] sum_co w1[co][ci] gt[co]
//   gx[n][ci]       = gy[n][ci] + sum_kz sum_co w3[co][ci][kz] ga[n - kz + 1][co]
//   dW1[co][ci]     = sum_(b,n,p) gt[co] a[ci]
//   dW3[co][ci][kz] = sum_(b,n,p) ga[n][co] x[n + kz - 1][ci]
//
// §15's column walk.  A unit is P = 128 consecutive flat pixels of one sample (the plane's last chunk zero-filled: padded, never masked), walked
// over all N slices by one workgroup of 4 waves; wave w owns pixels 32 w .. 32 w + 31 in every phase.  Step n stages slice n of gy, t (its hi
// part: the mask), a and x (register fills: 16-byte global loads issued before step n - 1's products, LDS stores after them) as [pixel][part][channel]
// images: gy, gt = masked gy, a, and x into a ring of two.  Phase 1 forms ga[n] (channel contraction: the filter as the MFMA's row operand, split
// once per workgroup into LDS, 16 pixels as its columns), masks it with a, rounds it to the record format and writes it into a ring of two; phase 2 reads it back for
// the three slice taps of gx -- out[n - 1] = P + W3[0]^T ga[n];  P = Q + gy[n] + W3[1]^T ga[n];  Q = W3[2]^T ga[n] -- so gx[n - 1] leaves at step n
// and every input is read once.  The weight gradients contract over the wave's 32 pixels through ds_read_b64_tr_b16 (§15's lane map):
// dW1 += gt^T a, dW3[1] += ga[n]^T x[n], dW3[0] += ga[n]^T x[n - 1], dW3[2] += ga[n - 1]^T x[n]; the taps of slices -1 and N never come up.
// Every FLUSH_STEPS steps at the latest the waves add their fp32 accumulators, one wave after the other, in float64 into the workgroup's block
// of the workspace (first flush: a plain store); att_tail_bwd_finish_kernel sums the blocks.  No atomics: two runs give identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_att_grad.h"
#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"
#include "dffw_tr_read.h"

namespace dffw {

using namespace attgrad;

template <int PREC, int C>
struct AttLds {
    static constexpr int PARTS = Fmt<PREC>::PARTS;
    static constexpr int CP = C < 16 ? 16 : C;   // channels of a part's row: whole 16-channel MFMA tiles, the pad stays zero
    static constexpr int PART = CP * 2, RAW = PARTS * PART;
    // 8 consecutive pixels of a transposed read on 8 distinct 32-byte slots of a bank row: stride / 32 odd (§15's rule)
    static constexpr int ROW = (RAW / 32) % 2 ? RAW : RAW + 32;
    static constexpr int IMG = P * ROW;
    static_assert(ROW % 32 == 0 && (ROW / 32) % 2 == 1 && ROW >= RAW, "rows hold their parts on odd multiples of 32 bytes");
};

// 0xFFFF in each half whose 16-bit value (bf16 or fp16: sign-magnitude) is > 0
__device__ __forceinline__ uint32_t positive_mask2(uint32_t w) {
    return ((int)(w << 16) > 0 ? 0xFFFFu : 0u) | ((int)(w & 0xFFFF0000u) > 0 ? 0xFFFF0000u : 0u);
}
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;   // a 16-byte piece in registers
__device__ __forceinline__ short8 as_short8(u32x4 v) { return __builtin_bit_cast(short8, v); }

template <int PREC, int C>
__global__ __launch_bounds__(256) void att_tail_bwd_kernel(const AttGradArgs a) {
    using L = AttLds<PREC, C>;
    static_assert(C == 8 || C == 16 || C == 32, "channels of the attention tails");
    static_assert(P == 4 * WAVE_PIX, "32 pixels per wave");
    constexpr int PARTS = L::PARTS, CP = L::CP, NT = CP / 16, OCT = C / 8, RS = PARTS * C;
    constexpr int NU = (WAVE_PIX * OCT + 63) / 64;   // (pixel, octet) staging pieces per lane
    constexpr int KG = CP / 8;                       // 8-channel groups of a contraction that hold data or pad; the lanes beyond supply zeros
    constexpr int ROW = L::ROW, PART = L::PART, IMG = L::IMG;
    __shared__ __attribute__((aligned(16))) char lds[7 * IMG];
    __shared__ __attribute__((aligned(16))) char lds_w[4 * NT * PARTS * 64 * 16];
    char *const im_gy = lds, *const im_gt = lds + IMG, *const im_a = lds + 2 * IMG, *const im_x = lds + 3 * IMG, *const im_ga = lds + 5 * IMG;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 15, kg = lane >> 4;
    const bool want_x = a.gx != nullptr, want_w = a.partial != nullptr;

    // the pads (channels C .. CP - 1, the bytes between RAW and ROW) are zero from here on: nothing below stores to them
    for (int i = tid * 16; i < 7 * IMG; i += 256 * 16) *reinterpret_cast<uint4 *>(lds + i) = make_uint4(0, 0, 0, 0);
    __syncthreads();

    // the filters as row operands, split here once per workgroup and kept in LDS: row = ci (tile mt), contraction = co; lane l's 16 bytes hold
    // co = 8 kg .. 8 kg + 7 of row ci = 16 mt + m.  [W3 kz = 0, 1, 2 | W1][mt][part][lane]
    auto w_at = [&](int k, int mt, int part) __attribute__((always_inline)) { return lds_w + (((k * NT + mt) * PARTS + part) * 64 + lane) * 16; };
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float *w = k == 3 ? a.w1 : want_x ? a.w3 : nullptr;
            const int taps = k == 3 ? 1 : 3, kz = k == 3 ? 0 : k;
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) {
                const int ci = mt * 16 + m;
                short8 v[PARTS];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int co = kg * 8 + j;
                    const float f = w && ci < C && co < C ? w[((int64_t)co * C + ci) * taps + kz] : 0.f;
                    uint16_t hi, lo;
                    Fmt<PREC>::split(f, hi, lo);
                    v[0][j] = (short)hi;
                    if constexpr (PARTS == 2) v[1][j] = (short)lo;
                }
#pragma unroll
                for (int part = 0; part < PARTS; ++part) *reinterpret_cast<short8 *>(w_at(k, mt, part)) = v[part];
            }
        }
    }
    auto read_w = [&](int k, int mt, short8(&o)[PARTS]) __attribute__((always_inline)) {
#pragma unroll
        for (int part = 0; part < PARTS; ++part) o[part] = *reinterpret_cast<const short8 *>(w_at(k, mt, part));
    };

    // this lane's staging pieces: pixel of the chunk and octet -> LDS offset (part 0) and offset inside a pixel's record
    int s_px[NU], s_rec[NU], s_lds[NU];
    bool s_on[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const int iu = lane + 64 * j, oct = iu % OCT;
        s_on[j] = iu < WAVE_PIX * OCT;
        s_px[j] = wave * WAVE_PIX + (s_on[j] ? iu / OCT : 0);
        s_rec[j] = oct * 8;
        s_lds[j] = s_px[j] * ROW + oct * 16;
    }
    // this lane's places in the channel contractions: column = pixel 16 pt + m of the wave's 32, data operand bytes 16 kg .. of a part's row;
    // result rows = channels 16 mt + 4 kg .. + 3 of that pixel
    const int colpix = wave * WAVE_PIX + m;
    const bool k_on = kg < KG;
    const uint32_t k_mask = k_on ? 0xFFFFFFFFu : 0u;
    const int b_off = colpix * ROW + (k_on ? kg : 0) * 16;
    const int d_off = colpix * ROW + kg * 8;
    // ... and of a transposed read (§15): pixel 32 wave + 16 half + 4 gl + q of the first read, 8 pixels on for the second; channels 4 p .. 4 p + 3
    const auto [q, p, half, gl] = tr_lane(lane);
    const int tr_off = (wave * WAVE_PIX + half * 16 + 4 * gl + q) * ROW + p * 8;

    auto read_b = [&](const char *img, int pt, short8(&b)[PARTS]) __attribute__((always_inline)) {
#pragma unroll
        for (int part = 0; part < PARTS; ++part) {
            u32x4 v = *reinterpret_cast<const u32x4 *>(img + b_off + pt * 16 * ROW + part * PART);
            if constexpr (KG < 4) v &= k_mask;   // the contraction's lanes beyond the row supply zeros
            b[part] = as_short8(v);
        }
    };
    auto read_tr = [&](const char *img, short8(&o)[NT][PARTS]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int part = 0; part < PARTS; ++part) {
                const char *s = img + tr_off + part * PART + t * 32;
                o[t][part] = tr_pair(s, s + 8 * ROW);
            }
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    f32x4 acc[4][NT][NT];   // [dW3 kz = 0, 1, 2 | dW1][co tile][ci tile]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[k][i][j] = zero4;
    double *const blk = want_w ? a.partial + (int64_t)blockIdx.x * block(C) : nullptr;
    bool first = true;
    int since = 0;
    auto flush = [&]() __attribute__((always_inline)) {
        if (!want_w) return;
#pragma unroll
        for (int w = 0; w < 4; ++w) {   // one wave after the other: a fixed order of the float64 additions
            if (wave == w) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int co = i * 16 + kg * 4 + r, ci = j * 16 + m;
                                if (co < C && ci < C) flush_f64(blk + (k * C + co) * C + ci, acc[k][i][j][r], first && w == 0);
                            }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[k][i][j] = zero4;
        first = false;
        since = 0;
    };

    const int64_t slice = (int64_t)a.HW * RS;
    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int b = u / a.chunks, p0 = (u - b * a.chunks) * P;   // the chunk never leaves its plane: the pixels beyond H*W are zeros
        const int64_t base = ((int64_t)b * a.N * a.HW + p0) * RS;  // slice 0 of the sample, the chunk's first pixel
        int64_t s_off[NU];   // < 0: padding (beyond the plane) or no piece of this lane
#pragma unroll
        for (int j = 0; j < NU; ++j) s_off[j] = s_on[j] && p0 + s_px[j] < a.HW ? base + (int64_t)s_px[j] * RS + s_rec[j] : -1;
        u32x4 r_gy[NU][PARTS], r_t[NU], r_a[NU][PARTS], r_x[NU][PARTS];
        // slice n: global -> registers ...
        auto load = [&](int n) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const int64_t o = s_off[j] + n * slice;
                const bool on = s_off[j] >= 0;
                const u32x4 z = {0, 0, 0, 0};
                r_t[j] = on ? *reinterpret_cast<const u32x4 *>(a.t + o) : z;
#pragma unroll
                for (int part = 0; part < PARTS; ++part) {
                    r_gy[j][part] = on ? *reinterpret_cast<const u32x4 *>(a.gy + o + part * C) : z;
                    r_a[j][part] = on ? *reinterpret_cast<const u32x4 *>(a.a + o + part * C) : z;
                    r_x[j][part] = on ? *reinterpret_cast<const u32x4 *>(a.x + o + part * C) : z;
                }
            }
        };
        // ... registers -> LDS: gy, gt = [t > 0] gy (the mask of the stored t: its hi part is positive exactly where the record is), a, x into slot n % 2
        auto store = [&](int n) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                if (!s_on[j]) continue;
                const u32x4 mk = {positive_mask2(r_t[j][0]), positive_mask2(r_t[j][1]), positive_mask2(r_t[j][2]), positive_mask2(r_t[j][3])};
#pragma unroll
                for (int part = 0; part < PARTS; ++part) {
                    const int o = s_lds[j] + part * PART;
                    const u32x4 g = r_gy[j][part];
                    *reinterpret_cast<u32x4 *>(im_gy + o) = g;
                    *reinterpret_cast<u32x4 *>(im_gt + o) = g & mk;
                    *reinterpret_cast<u32x4 *>(im_a + o) = r_a[j][part];
                    *reinterpret_cast<u32x4 *>(im_x + (n & 1) * IMG + o) = r_x[j][part];
                }
            }
        };
        // gx[b, n] of this lane's 4 channels of pixel 16 pt + m: split into a record, two 8-byte stores
        auto store_gx = [&](int n, int pt, int mt, const f32x4 &v) __attribute__((always_inline)) {
            const int px = colpix + pt * 16, c0 = mt * 16 + kg * 4;
            uint32_t h01, l01, h23, l23;
            Fmt<PREC>::split2(v[0], v[1], h01, l01);
            Fmt<PREC>::split2(v[2], v[3], h23, l23);
            if (c0 < C && p0 + px < a.HW) {
                uint16_t *dst = a.gx + base + n * slice + (int64_t)px * RS + c0;
                *reinterpret_cast<uint2 *>(dst) = make_uint2(h01, h23);
                if constexpr (PARTS == 2) *reinterpret_cast<uint2 *>(dst + C) = make_uint2(l01, l23);
            }
        };

        f32x4 Pn[2][NT], Qn[2][NT];   // gx[n] without its tap of ga[n + 1]; the tap of ga[n] in gx[n + 1]
        // (the previous unit ended behind the barrier that follows its last reads)
        load(0);
        store(0);
        for (int n = 0; n < a.N; ++n) {
            const bool more = n + 1 < a.N;
            if (more) load(n + 1);
            char *const ga_cur = im_ga + (n & 1) * IMG, *const ga_prev = im_ga + ((n + 1) & 1) * IMG;
            const char *const x_cur = im_x + (n & 1) * IMG, *const x_prev = im_x + ((n + 1) & 1) * IMG;
            __syncthreads();   // slice n's images are complete
            // phase 1: ga[n] = [a > 0] W1^T gt, rounded to the record format, into its ring slot
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                short8 bg[PARTS];
                read_b(im_gt, pt, bg);
#pragma unroll
                for (int mt = 0; mt < NT; ++mt) {
                    short8 wa[PARTS];
                    read_w(3, mt, wa);
                    const f32x4 d = mma3<PREC>(wa, bg, zero4);
                    const int o = d_off + pt * 16 * ROW + mt * 32;
                    const uint2 av = *reinterpret_cast<const uint2 *>(im_a + o);   // a's hi part: positive exactly where the record is
                    const uint32_t m01 = positive_mask2(av.x), m23 = positive_mask2(av.y);
                    uint32_t h01, l01, h23, l23;
                    Fmt<PREC>::split2(d[0], d[1], h01, l01);
                    Fmt<PREC>::split2(d[2], d[3], h23, l23);
                    if (mt * 16 + kg * 4 < C) {
                        *reinterpret_cast<uint2 *>(ga_cur + o) = make_uint2(h01 & m01, h23 & m23);
                        if constexpr (PARTS == 2) *reinterpret_cast<uint2 *>(ga_cur + o + PART) = make_uint2(l01 & m01, l23 & m23);
                    }
                }
            }
            if (want_w) {   // dW1 += gt^T a over the wave's 32 pixels
                short8 ag[NT][PARTS], bf[NT][PARTS];
                read_tr(im_gt, ag);
                read_tr(im_a, bf);
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[3][i][j] = mma3<PREC>(ag[i], bf[j], acc[3][i][j]);
            }
            __syncthreads();   // ga[n] is written
            // phase 2: the three slice taps of ga[n]
            if (want_x) {
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    short8 bg[PARTS];
                    read_b(ga_cur, pt, bg);
#pragma unroll
                    for (int mt = 0; mt < NT; ++mt) {
                        short8 wa[PARTS];
                        read_w(0, mt, wa);
                        if (n > 0) store_gx(n - 1, pt, mt, mma3<PREC>(wa, bg, Pn[pt][mt]));
                        const int o = d_off + pt * 16 * ROW + mt * 32;
                        const uint2 gh = *reinterpret_cast<const uint2 *>(im_gy + o);
                        uint2 gl2 = make_uint2(0, 0);
                        if constexpr (PARTS == 2) gl2 = *reinterpret_cast<const uint2 *>(im_gy + o + PART);
                        f32x4 init;
                        float g0, g1, g2, g3;
                        Fmt<PREC>::join2(gh.x, gl2.x, g0, g1);
                        Fmt<PREC>::join2(gh.y, gl2.y, g2, g3);
                        init[0] = g0;
                        init[1] = g1;
                        init[2] = g2;
                        init[3] = g3;
                        if (n > 0) init += Qn[pt][mt];
                        read_w(1, mt, wa);
                        Pn[pt][mt] = mma3<PREC>(wa, bg, init);
                        read_w(2, mt, wa);
                        Qn[pt][mt] = mma3<PREC>(wa, bg, zero4);
                    }
                }
            }
            if (want_w) {   // dW3[1] += ga[n]^T x[n];  dW3[0] += ga[n]^T x[n - 1];  dW3[2] += ga[n - 1]^T x[n]  (n = 0: no slice -1, uniformly)
                short8 ag[NT][PARTS], bx[NT][PARTS];
                read_tr(ga_cur, ag);
                read_tr(x_cur, bx);
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[1][i][j] = mma3<PREC>(ag[i], bx[j], acc[1][i][j]);
                if (n > 0) {
                    short8 agp[NT][PARTS], bxp[NT][PARTS];
                    read_tr(ga_prev, agp);
                    read_tr(x_prev, bxp);
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            acc[0][i][j] = mma3<PREC>(ag[i], bxp[j], acc[0][i][j]);
                            acc[2][i][j] = mma3<PREC>(agp[i], bx[j], acc[2][i][j]);
                        }
                }
            }
            __syncthreads();   // step n's reads are done: the images and the ring slots of n - 1 may be overwritten
            if (more) store(n + 1);
            if (++since >= a.flush_steps) flush();
        }
        if (want_x) {   // the last slice has no tap of ga[N]
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int mt = 0; mt < NT; ++mt) store_gx(a.N - 1, pt, mt, Pn[pt][mt]);
        }
    }
    flush();   // also with nothing summed: every block of the workspace is written
}

// dW3 (C, C, 3, 1, 1) and dW1 (C, C, 1, 1, 1) fp32 = the workgroups' blocks summed in float64 in a fixed order.  One wave per element: lane l adds the
// blocks l, l + 64, ... one by one, then the 64 lane sums meet in a butterfly (strides 32, 16, ... 1)
__global__ __launch_bounds__(256) void att_tail_bwd_finish_kernel(const double *__restrict__ partial, int nblk, int C, float *__restrict__ dw3,
                                                                  float *__restrict__ dw1) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave, cc = C * C;
    if (e >= 4 * cc) return;   // (uniform over the wave)
    double s = 0.0;
    for (int w = lane; w < nblk; w += 64) s += partial[(int64_t)w * (4 * cc) + e];
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        const int k = e / cc, r = e - k * cc;
        if (k < 3) dw3[r * 3 + k] = (float)s;
        else dw1[r] = (float)s;
    }
}

using AttGradRow = KernelRow<AttGradArgs>;
// [precision][C == 8, 16, 32]
static const AttGradRow ATTGRAD_ROWS[] = {
    DFFW_ROW(256, att_tail_bwd_kernel, 0, 8), DFFW_ROW(256, att_tail_bwd_kernel, 0, 16), DFFW_ROW(256, att_tail_bwd_kernel, 0, 32),
    DFFW_ROW(256, att_tail_bwd_kernel, 1, 8), DFFW_ROW(256, att_tail_bwd_kernel, 1, 16), DFFW_ROW(256, att_tail_bwd_kernel, 1, 32),
    DFFW_ROW(256, att_tail_bwd_kernel, 2, 8), DFFW_ROW(256, att_tail_bwd_kernel, 2, 16), DFFW_ROW(256, att_tail_bwd_kernel, 2, 32),
};
static const AttGradRow *select(int prec, int C) {
    return C == 8 || C == 16 || C == 32 ? prec_row(ATTGRAD_ROWS, prec, 3, C == 8 ? 0 : C == 16 ? 1 : 2) : nullptr;
}

const char *att_tail_bwd_kernel_name(int prec, int C) {
    const AttGradRow *row = select(prec, C);
    return row ? row->name : nullptr;
}

unsigned att_tail_bwd_grid_x(const AttGradArgs &a, int wgs) { return persistent_grid(a.total_units, std::max(8, wgs > 0 ? wgs : DEFAULT_WGS)); }

hipError_t launch_att_tail_bwd(int prec, int C, const AttGradArgs &a, unsigned grid_x, float *dw3, float *dw1, hipStream_t s) {
    const AttGradRow *row = select(prec, C);
    if (!row) return hipErrorInvalidValue;
    if (a.partial) return launch_row_then(row, dim3(grid_x), a, s, att_tail_bwd_finish_kernel, (unsigned)block(C) / 4, a.partial, (int)grid_x, C, dw3, dw1);
    hipLaunchKernelGGL(row->fn, dim3(grid_x), dim3(row->block), 0, s, a);
    return hipGetLastError();
}

}  // namespace dffw
