// Weight gradient of the stem, Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2)) on the image stack:
//
//   dW[co][ci][0][ky][kx] = sum over (b, n, y, x) of g[b, n, y, x, co] * x[b, ci, n, y + 2 ky - 8, x + 2 kx - 8]      (zero outside the image)
//
// The contraction runs over PIXELS.  g is an 8-channel activation record [pixel][part][channel] and becomes the MFMA's row operand through
// ds_read_b64_tr_b16, exactly as in dffw_conv_wgrad.hip (its second octet is zero: padded, never masked).  x is the planar fp32 stack: a unit's
// footprint is rounded to the parts of the precision on its way into LDS and kept PLANAR there, so the column operand of filter element
// (ci, ky, kx) is a plain 8-byte read of 4 consecutive pixels, shifted by 2 ky rows and 2 kx pixels.  A shift of 2 kx pixels is 4 kx bytes: the
// image is kept twice, the second copy two pixels to the right, and odd kx read that one, so every ds_read_b64 is 8-byte aligned.
// The 243 filter elements of a channel are the MFMA columns, 16 tiles of 16 dealt round-robin to the 4 waves (4 accumulator tiles each); a
// workgroup walks units of 16 x 32 pixels by the persistent-grid rule of dffw_persist.h.  Accumulation, flush and finish follow §13: fp32 for at
// most 16 384 pixels, then float64 into the workgroup's own block, the blocks summed in workgroup order.  No atomics: two runs give identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dffw_device.h"
#include "dffw_internal.h"
#include "dffw_persist.h"
#include "dffw_stem_wgrad.h"
#include "dffw_tr_read.h"

namespace dffw {

using namespace stemw;

template <int PREC>
struct StemWgradLds {
    static constexpr int PARTS = Fmt<PREC>::PARTS;
    // g: one image per part, one 32-byte row of 16 channels (8 real) per pixel: 8 consecutive pixels lie on the 8 32-byte slots of a 256-byte
    // bank row, as in dffw_conv_wgrad.hip's one-part image (its two-part rows of 96 bytes would cost 16 KB more and the second workgroup of a CU)
    static constexpr int G_ROW = 32, G_PART = TY * TX * G_ROW;
    static constexpr int G_BYTES = PARTS * G_PART;
    // x: [part][copy][plane][FY rows][X_ROW elements] of 16 bits; copy 1 holds every row two elements to the right.  Strides in elements,
    // multiples of 4 (8-byte reads stay aligned); the pads spread the 16 columns of a tile over the banks
    static constexpr int X_ROW = 52, X_PLANE = FY * X_ROW + 4, X_COPY = CI * X_PLANE + 32, X_PART = 2 * X_COPY;
    static_assert(X_ROW >= FX + 2 + 2 && X_ROW % 4 == 0 && X_PLANE % 4 == 0 && X_COPY % 4 == 0, "copy 1 fits its shifted row; 8-byte alignment");
    static constexpr int X_BYTES = PARTS * X_PART * 2;
};

template <int PREC>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const StemWgradArgs a) {
    using L = StemWgradLds<PREC>;
    constexpr int PARTS = L::PARTS;
    constexpr int NJ = TILES / 4;   // column tiles of a wave
    __shared__ __attribute__((aligned(16))) char lds_g[L::G_BYTES];
    __shared__ __attribute__((aligned(16))) uint16_t lds_x[L::X_BYTES / 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    // the row operand, as conv_wgrad_kernel reads it: this lane addresses pixel q of the group's 4, channels 4p .. 4p + 3; the group's 4 pixels
    // are columns 16 ch + 8r + 4 gl + 0..3 of tile row 2 cr + half for read r of chunk (cr, ch)
    const auto [q, p, half, gl] = tr_lane(lane);
    const char *const ga = lds_g + (half * TX + 4 * gl + q) * L::G_ROW + p * 8;
    // the column operand: this lane's column of each of its tiles and the element offset of its 4 pixels of read 0 of chunk (0, 0).  A dead
    // column (the last 13 of tile 15) reads filter element 0's pixels and is never flushed
    int xo[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int col = (wave + 4 * j) * 16 + (lane & 15);
        if (col >= COLS) col = 0;
        const int ci = col / (K * K), ky = col / K % K, kx = col % K, cp = kx & 1;
        xo[j] = cp * L::X_COPY + ci * L::X_PLANE + (DIL * ky + half) * L::X_ROW + DIL * kx + 2 * cp + 4 * gl;
    }

    // the zero octet of every g row: written once, the units fill the real one
    for (int i = tid; i < TY * TX * PARTS; i += 256) *reinterpret_cast<uint4 *>(lds_g + i * L::G_ROW + 16) = make_uint4(0, 0, 0, 0);

    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    double *const blk = a.partial + (int64_t)blockIdx.x * BLOCK;
    bool first = true;
    int since = 0;
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = (wave + 4 * j) * 16 + (lane & 15);
            if (col < COLS && lane < 32) {   // rows 0 .. 7 of the 16 are g's channels
#pragma unroll
                for (int r = 0; r < 4; ++r) flush_f64(blk + ((lane >> 4) * 4 + r) * COLS + col, acc[j][r], first);
            }
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        first = false;
        since = 0;
    };

    const UnitRange rg = persistent_range(a.total_units);
    for (int u = rg.first; u < rg.end; u += rg.step) {
        const int txi = u % a.tiles_x;
        int tt = u / a.tiles_x;
        const int tyi = tt % a.tiles_y;
        tt /= a.tiles_y;
        const int n = tt % a.N, b = tt / a.N;
        const int gy0 = tyi * TY, gx0 = txi * TX;
        __syncthreads();   // the previous unit's reads are done (and, at the first unit, the zero octets are written)
        {   // g tile: TY * TX pixels x PARTS octets, zero beyond the image
            const uint16_t *gp = a.g + ((int64_t)b * a.N + n) * a.H * a.W * (PARTS * CO);
#pragma unroll
            for (int i = tid; i < TY * TX * PARTS; i += 256) {   // (the loops of the staging are unrolled: every load of a unit is in flight at once)
                const int part = i % PARTS, px = i / PARTS;
                const int gy = gy0 + px / TX, gx = gx0 + px % TX;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (gy < a.H && gx < a.W) v = *reinterpret_cast<const uint4 *>(gp + ((int64_t)gy * a.W + gx) * (PARTS * CO) + part * CO);
                *reinterpret_cast<uint4 *>(lds_g + px * L::G_ROW + part * L::G_PART) = v;
            }
        }
        {   // x footprint: CI planes x FY rows x FX / 4 quads of pixels, zero outside the image, rounded to the parts like every record
#pragma unroll
            for (int i = tid; i < CI * FY * (FX / 4); i += 256) {
                const int quad = i % (FX / 4), fy = i / (FX / 4) % FY, ci = i / (FX / 4) / FY;
                const int iy = gy0 - PAD + fy, ix = gx0 - PAD + 4 * quad;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if ((unsigned)iy < (unsigned)a.H) {
                    const float *xp = a.x + (((int64_t)b * CI + ci) * a.N + n) * a.H * a.W + (int64_t)iy * a.W;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((unsigned)(ix + e) < (unsigned)a.W) v[e] = xp[ix + e];
                }
                uint32_t h01, l01, h23, l23;
                Fmt<PREC>::split2(v[0], v[1], h01, l01);
                Fmt<PREC>::split2(v[2], v[3], h23, l23);
                uint16_t *row = lds_x + ci * L::X_PLANE + fy * L::X_ROW + 4 * quad;
                *reinterpret_cast<uint2 *>(row) = make_uint2(h01, h23);
                *reinterpret_cast<uint32_t *>(row + L::X_COPY + 2) = h01;
                *reinterpret_cast<uint32_t *>(row + L::X_COPY + 4) = h23;
                if constexpr (PARTS == 2) {
                    *reinterpret_cast<uint2 *>(row + L::X_PART) = make_uint2(l01, l23);
                    *reinterpret_cast<uint32_t *>(row + L::X_PART + L::X_COPY + 2) = l01;
                    *reinterpret_cast<uint32_t *>(row + L::X_PART + L::X_COPY + 4) = l23;
                }
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int cr = 0; cr < TY / 2; ++cr) {
#pragma unroll
            for (int ch = 0; ch < TX / 16; ++ch) {
                short8 ag[PARTS];
#pragma unroll
                for (int part = 0; part < PARTS; ++part) {
                    const char *g0 = ga + (2 * cr * TX + 16 * ch) * L::G_ROW + part * L::G_PART;
                    ag[part] = tr_pair(g0, g0 + 8 * L::G_ROW);
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    short8 bx[PARTS];
#pragma unroll
                    for (int part = 0; part < PARTS; ++part) {
                        const uint16_t *x0 = lds_x + part * L::X_PART + xo[j] + 2 * cr * L::X_ROW + 16 * ch;
                        const short4v lo4 = *reinterpret_cast<const short4v *>(x0), hi4 = *reinterpret_cast<const short4v *>(x0 + 8);
                        bx[part] = short8{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
                    }
                    acc[j] = mma3<PREC>(ag, bx, acc[j]);
                }
            }
        }
        if (++since >= a.flush_units) flush();
    }
    flush();   // also with nothing summed: every block of the workspace is written
}

// dW (8, 3, 1, 9, 9) fp32 = the workgroups' blocks summed in float64 in workgroup order, one thread per element
__global__ __launch_bounds__(256) void stem_wgrad_finish_kernel(const double *__restrict__ partial, int nwg, float *__restrict__ dw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= BLOCK) return;
    double s = 0.0;
#pragma unroll 32   // the additions keep their order; the loads of 32 blocks are in flight at once
    for (int w = 0; w < nwg; ++w) s += partial[(int64_t)w * BLOCK + e];
    dw[e] = (float)s;
}

using StemWgradRow = KernelRow<StemWgradArgs>;
static const StemWgradRow STEM_WGRAD_ROWS[] = {DFFW_ROW(256, stem_wgrad_kernel, 0), DFFW_ROW(256, stem_wgrad_kernel, 1), DFFW_ROW(256, stem_wgrad_kernel, 2)};

const char *stem_wgrad_kernel_name(int prec) {
    const StemWgradRow *row = prec_row(STEM_WGRAD_ROWS, prec, 1, 0);
    return row ? row->name : nullptr;
}

unsigned stem_wgrad_grid_x(const StemWgradArgs &a, int wgs) { return persistent_grid(a.total_units, std::max(8, wgs > 0 ? wgs : DEFAULT_WGS)); }

hipError_t launch_stem_wgrad(int prec, const StemWgradArgs &a, unsigned grid_x, float *dw, hipStream_t s) {
    return launch_row_then(prec_row(STEM_WGRAD_ROWS, prec, 1, 0), dim3(grid_x), a, s, stem_wgrad_finish_kernel, (BLOCK + 255) / 256, a.partial, (int)grid_x, dw);
}

}  // namespace dffw
