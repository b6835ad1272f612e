// The streaming kernels of the End_to_End alignment network (FlowNetwork, End_to_End.py:37-105), one persistent kernel per block:
//   of_roll8 / of_first   the 8-channel stride-1 feature blocks at full resolution (of_first reads the fp32 focal stack itself)
//   of_roll               the stride-1 feature blocks with 16 output channels, and (SUMS) the 16 -> 16 conv pair of the level-1 head
//   of_s2                 the 8 -> 16 channel down-sampling feature block
//   head_warp             the first conv of the level-1 / level-2 alignment head on the FOV-warped features
// They share the skeleton of the depth network's SRD kernels (dffw_srd_roll.hip: a workgroup owns a column of 8 x 16 pixels of one sample
// and walks its slices, intermediates stay in LDS, counted waits) and its argument block (SrdArgs); no device code is shared between
// the two files.  Host side: dffw_align.cpp.
#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "dffw_align.h"
#include "dffw_device.h"
#include "dffw_persist.h"

namespace dffw {

using SrdRow = KernelRow<SrdArgs>;   // dffw_persist.h

// ---- of_roll8: the 8-channel stride-1 residual blocks of the alignment network (`OF_feature.0`, `OF_feature.1`, full resolution) --
// As of_roll_kernel, in srd_roll_kernel's pixel-pair form (8 output channels): stage A = conv.0 -> t in LDS, stage B = conv.2 over
// t (3 chunks) + one chunk for the 1x1x1 shortcut (K octet 0 = the even pixel's 8 input channels, octet 1 = the odd pixel's), ReLU,
// stores.  a.w2 = conv.2 as 3 pair-form chunks + the shortcut chunk (pack_conv).
template <int PREC>
__global__ __launch_bounds__(256) void of_roll8_kernel(const SrdArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int C = 8, TY = 8, TX = 16, NWAVES = 4;
    constexpr int XY = TY + 4, XX = TX + 4, XPIX = XY * XX;        // x footprint
    constexpr int TYT = TY + 2, TXT = TX + 2, TPIX = TYT * TXT;    // region of t that conv.2 needs
    constexpr int PIXB = C * 2;                                    // bytes per pixel per plane
    constexpr int NPIECE = (XPIX + 63) / 64;                       // 1 KiB wave instructions per plane (one 16-byte chunk per pixel)
    constexpr int PLANEB = NPIECE * 1024;
    constexpr int SLOTB = PARTS * PLANEB;
    constexpr int RX = 4;                                          // x FIFO depth
    constexpr int NP = PARTS * NPIECE, PPW = (NP + NWAVES - 1) / NWAVES;
    static_assert(NP % PPW == 0, "every wave issues PPW pieces or none (counted vmcnt waits)");
    constexpr int TPLANEB = (TPIX * PIXB + 15) / 16 * 16;
    constexpr int X_OFF = 0, T_OFF = RX * SLOTB;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[T_OFF + PARTS * TPLANEB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    auto lds_store8 = [&](unsigned byte_off, uint32_t v0, uint32_t v1) {
        const u32x2 d = {v0, v1};
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds0 + byte_off), "v"(d) : "memory");
    };

    // ---- columns of this workgroup: as conv_roll (XCD-contiguous ranges, round-robin inside the XCD) ----------------
    const UnitRange ur = persistent_range(a.total_tiles);   // dffw_persist.h
    const int ufirst = ur.first, uend = ur.end, wgs_per_xcd = ur.step;
    if (ufirst >= uend) return;
    struct Unit {
        int b, gy0, gx0;
    };
    auto decode = [&](int u) {
        Unit c;
        const int txi = u % a.tiles_x;
        const int tt = u / a.tiles_x;
        c.b = tt / a.tiles_y;
        c.gy0 = (tt % a.tiles_y) * TY;
        c.gx0 = txi * TX;
        return c;
    };

    // ---- x FIFO: the slices of the workgroup's columns as one stream (N per column) ---------------------------------
    const int rec = PARTS * C;                                     // 16-bit elements per pixel record
    const int slice_elems = a.H * a.W * rec;
    const uint16_t *fsrc[PPW];
    bool fok[PPW];
    int fu = ufirst, fq = 0;
    auto setup_fill = [&]() {
        const Unit c = decode(fu);
#pragma unroll
        for (int k = 0; k < PPW; ++k) {
            const int p = wave * PPW + k;
            const int part = p / NPIECE, i = p % NPIECE;
            const int pix = i * 64 + lane;
            const int fy = pix / XX, sx = pix - fy * XX;
            const int fx = sx < XX / 2 ? 2 * sx : 2 * (sx - XX / 2) + 1;   // LDS rows hold the even columns first, then the odd ones
            const int iy = c.gy0 - 2 + fy, ix = c.gx0 - 2 + fx;
            fok[k] = p < NP && pix < XPIX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            fsrc[k] = a.x + (int64_t)c.b * a.N * slice_elems + (int64_t)(iy * a.W + ix) * rec + part * C;
        }
    };
    setup_fill();
    int fslot = 0;
    auto issue_next = [&]() {
        const bool zin = fu < uend;
        unsigned char *slot = smem + X_OFF + fslot * SLOTB;
        const int64_t zo = (int64_t)fq * slice_elems;
#pragma unroll
        for (int k = 0; k < PPW; ++k) {
            const int p = wave * PPW + k;
            if (p >= NP) break;
            const int part = p / NPIECE, i = p % NPIECE;
            const uint16_t *src = (zin && fok[k]) ? fsrc[k] + zo : a.zero;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(slot + part * PLANEB + i * 1024), 16, 0, 0);
        }
        fslot = (fslot + 1 == RX) ? 0 : fslot + 1;
        if (++fq == a.N && fu < uend) {
            fq = 0;
            fu += wgs_per_xcd;
            if (fu < uend) setup_fill();
        }
    };

    // ---- per-lane constants ------------------------------------------------------------------------------------------
    // Both convs have 8 output channels: a GEMM column is a PAIR of horizontally adjacent pixels (result rows 0-7 = even
    // pixel, 8-15 = odd pixel) contracting per filter row over the 4 input columns the pair touches (4 x 8 channels = one
    // 32-deep chunk; K octet g = input column 2*pair + g), as in conv_roll's pair form: no dead rows, half the tiles.
    // LDS rows (x and t) keep the even columns first, then the odd ones, so the pairs of a tile read consecutive 16-byte slots.
    // stage A: the 10 x 18 t pixels are 90 pairs = 6 operand tiles (the last one partly idle): waves 2, 3 take two tiles
    // each, waves 0, 1 one each (those two waves also run stage C of an earlier slice in the same phase)
    constexpr int TA = 2;
    const int nA = wave < 2 ? 2 : 1;
    constexpr int APAIRS = TYT * (TXT / 2);
    int pa[TA], ta_y[TA], ta_x[TA], ta_st[TA];
    bool ta_ok[TA];
#pragma unroll
    for (int j = 0; j < TA; ++j) {
        const int tile = j == 0 ? wave : 4 + wave;
        int pi = tile * 16 + r;
        ta_ok[j] = pi < APAIRS;
        if (pi >= APAIRS) pi = APAIRS - 1;   // idle columns recompute the last pair, nothing is stored for them
        const int row = pi / (TXT / 2), pc = pi - row * (TXT / 2);
        ta_y[j] = row;
        ta_x[j] = 2 * pc + (g >> 1);        // the t pixel this lane ends up with (channels (g & 1)*4 ..)
        pa[j] = (row * XX + ((g & 1) ? XX / 2 : 0) + pc + (g >> 1)) * PIXB;   // input column 2*pc + g of row `row`
        ta_st[j] = T_OFF + (row * TXT + ((g >> 1) ? TXT / 2 : 0) + pc) * PIXB + (g & 1) * 8;
    }
    // stage B: the 8 x 16 feat pixels are 64 pairs = 4 tiles, one per wave
    const int pb_pi = wave * 16 + r, pb_y = pb_pi / (TX / 2), pb_pc = pb_pi % (TX / 2), pb_x = 2 * pb_pc + (g >> 1);
    const int pbo = (pb_y * TXT + ((g & 1) ? TXT / 2 : 0) + pb_pc + (g >> 1)) * PIXB;
    // shortcut operand: K octet g < 2 = the 8 input channels of pixel 2*pair + g at the centre tap (octets 2, 3: zero weights)
    const int pb_sc = ((pb_y + 2) * XX + ((g & 1) ? XX / 2 : 0) + pb_pc + 1) * PIXB;
    // the two filters as MFMA A-fragments (3 chunks each) and their BatchNorm shifts
    short8 w0[3][PARTS], w2[3][PARTS], wsc[PARTS];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) {
            w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
            w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
        }
#pragma unroll
    for (int pt = 0; pt < PARTS; ++pt) wsc[pt] = reinterpret_cast<const short8 *>(a.w2)[(3 * PARTS + pt) * 64 + lane];
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(a.b0 + (g & 1) * 4);
    const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + (g & 1) * 4);
    // one operand tile: 3 chunks (filter rows) x hi/lo, read by inline asm (hipcc degrades every lgkmcnt wait to 0 and adds
    // vmcnt(0) in front of reads of DMA-filled slots while an LDS-DMA is outstanding) and contracted as they arrive
    auto tile_mma = [&](unsigned base, auto rowB_c, auto loB_c, const short8 (&wf)[3][PARTS], f32x4 acc) {
        constexpr int rowB = decltype(rowB_c)::value, loB = decltype(loB_c)::value;   // immediates of the reads: no address arithmetic per chunk
        short8 xh[3], xl[3];
#define DFFW_SRD_READ(k)                                                                                                                  \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xh[k]) : "v"(base), "n"(k * rowB));                                               \
    if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k]) : "v"(base), "n"(k * rowB + loB));               \
    else xl[k] = short8{0, 0, 0, 0, 0, 0, 0, 0};   /* (single-part storage: never contracted; NOT a copy of the in-flight hi fragment, tools/isa_wait_lint.py) */
        DFFW_SRD_READ(0)
        DFFW_SRD_READ(1)
        DFFW_SRD_READ(2)
#undef DFFW_SRD_READ
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k == 0) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(xh[0]), "+v"(xl[0]) : "n"(2 * PARTS));
            else if (k == 1) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(xh[1]), "+v"(xl[1]) : "n"(PARTS));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh[2]), "+v"(xl[2]));
            if constexpr (PARTS == 2) {
                acc = mma<F16>(wf[k][1], xh[k], acc);
                acc = mma<F16>(wf[k][0], xl[k], acc);
            }
            acc = mma<F16>(wf[k][0], xh[k], acc);
        }
        return acc;
    };

    constexpr int INFLIGHT = (RX - 2) * PPW;   // slices that may stay in flight when the next one is needed
#pragma unroll
    for (int q = 0; q < RX - 1; ++q) issue_next();
    __builtin_amdgcn_s_waitcnt(0x0F70);   // compiler-visible vmcnt(0): filters, shifts and the first slices
    asm volatile("s_barrier" ::: "memory");

    int xslot = 0;
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        const Unit U = decode(cu);
        for (int s = 0; s < a.N; ++s) {
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(INFLIGHT) : "memory");
            // ---- stage A: t = relu(conv.0(x) + shift) on the 10 x 18 region, zero outside the image --------------------------------
#pragma unroll
            for (int j = 0; j < TA; ++j) {
                if (j >= nA) break;
                const f32x4 acc = tile_mma(lds0 + X_OFF + xslot * SLOTB + pa[j], std::integral_constant<int, XX * PIXB>{}, std::integral_constant<int, PLANEB>{}, w0, b0);
                const int iy = U.gy0 - 1 + ta_y[j], ix = U.gx0 - 1 + ta_x[j];
                const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                if (ta_ok[j]) {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_lim_bits(acc[0], inside ? 0x7f800000 : 0), relu_lim_bits(acc[1], inside ? 0x7f800000 : 0), h01, l01);
                    Fmt<PREC>::split2(relu_lim_bits(acc[2], inside ? 0x7f800000 : 0), relu_lim_bits(acc[3], inside ? 0x7f800000 : 0), h23, l23);
                    lds_store8(ta_st[j], h01, h23);
                    if constexpr (PARTS == 2) lds_store8(ta_st[j] + TPLANEB, l01, l23);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // ---- stage B: out = relu(conv.2(t) + shift + shortcut(x)) -------------------------------------------------------------
            {
                f32x4 acc = tile_mma(lds0 + T_OFF + pbo, std::integral_constant<int, TXT * PIXB>{}, std::integral_constant<int, TPLANEB>{}, w2, b2);
                const unsigned xp = lds0 + X_OFF + xslot * SLOTB + pb_sc;
                short8 sh, sl;
                asm volatile("ds_read_b128 %0, %1" : "=v"(sh) : "v"(xp));
                if constexpr (PARTS == 2) {
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(sl) : "v"(xp), "n"(PLANEB));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sh), "+v"(sl));
                    acc = mma<F16>(wsc[1], sh, acc);
                    acc = mma<F16>(wsc[0], sl, acc);
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sh));
                }
                acc = mma<F16>(wsc[0], sh, acc);
                uint32_t h01, h23, l01, l23;
                Fmt<PREC>::split2(relu_bits(acc[0]), relu_bits(acc[1]), h01, l01);
                Fmt<PREC>::split2(relu_bits(acc[2]), relu_bits(acc[3]), h23, l23);
                const int64_t pix = (((int64_t)U.b * a.N + s) * a.H + U.gy0 + pb_y) * a.W + U.gx0 + pb_x;
                if constexpr (PARTS == 2) {
                    swap16(h01, l01);
                    swap16(h23, l23);
                    *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C) = make_uint4(h01, h23, l01, l23);
                } else {
                    *reinterpret_cast<uint2 *>(a.out + pix * rec + (g & 1) * 4) = make_uint2(h01, h23);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            issue_next();
            xslot = (xslot + 1 == RX) ? 0 : xslot + 1;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no LDS-DMA may outlive the wave
}

// ---- of_first: the first residual block of the alignment network (`OF_feature.0`, 3 -> 8 channels) straight from the fp32 stack ---
// of_roll8's arithmetic (pixel-pair form, same filter packing, same operation order: bit-identical results) with the block input
// taken from the planar fp32 focal stack (B,3,N,H,W) instead of the 8-channel record volume: thread p < 240 owns pixel p of the
// 12 x 20 footprint, requests its three colour values for slice s+1 before the contraction of slice s, splits them afterwards into the
// record [c0 c1 c2 0 0 0 0 0] (what from_ncdhw_pad wrote) and stores it into one of two LDS slots, even columns of a row first.  Saves
// the record volume's write and read (32 B per pixel each; the stack is 12 B per pixel).  Plain loads only: hipcc counts every wait.
template <int PREC>
__global__ __launch_bounds__(256) void of_first_kernel(const SrdArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int C = 8, TY = 8, TX = 16;
    constexpr int XY = TY + 4, XX = TX + 4, XPIX = XY * XX;        // x footprint
    constexpr int TYT = TY + 2, TXT = TX + 2, TPIX = TYT * TXT;    // region of t that conv.2 needs
    constexpr int PIXB = C * 2;
    constexpr int PLANEB = XPIX * PIXB, SLOTB = PARTS * PLANEB;
    constexpr int TPLANEB = (TPIX * PIXB + 15) / 16 * 16;
    constexpr int T_OFF = 2 * SLOTB;
    static_assert(XPIX <= 256, "one footprint pixel per thread");
    __shared__ __attribute__((aligned(16))) unsigned char smem[T_OFF + PARTS * TPLANEB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const UnitRange ur = persistent_range(a.total_tiles);   // dffw_persist.h
    const int ufirst = ur.first, uend = ur.end, wgs_per_xcd = ur.step;
    if (ufirst >= uend) return;
    struct Unit {
        int b, gy0, gx0;
    };
    auto decode = [&](int u) {
        Unit c;
        const int txi = u % a.tiles_x;
        const int tt = u / a.tiles_x;
        c.b = tt / a.tiles_y;
        c.gy0 = (tt % a.tiles_y) * TY;
        c.gx0 = txi * TX;
        return c;
    };
    const int rec = PARTS * C;
    const float *FS = a.w3;                                         // the fp32 focal stack (B,3,N,H,W)
    const int64_t plane = (int64_t)a.H * a.W, cplane = (int64_t)a.N * plane;

    // ---- fill side ---------------------------------------------------------------------------------------------------
    const bool gth = tid < XPIX;
    const int fy = tid / XX, fx = tid - fy * XX;
    const int lpos = (fy * XX + ((fx & 1) ? XX / 2 + (fx >> 1) : (fx >> 1))) * PIXB;   // even columns of a row first
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    auto issue = [&](const Unit &U, int n) {
        const int iy = U.gy0 - 2 + fy, ix = U.gx0 - 2 + fx;
        c0 = c1 = c2 = 0.f;
        if (gth && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
            const float *sp = FS + (int64_t)U.b * 3 * cplane + (int64_t)n * plane + (int64_t)iy * a.W + ix;
            c0 = sp[0];
            c1 = sp[cplane];
            c2 = sp[2 * cplane];
        }
    };
    auto land = [&](int slot) {
        if (!gth) return;
        uint4 h = make_uint4(0, 0, 0, 0), l = h;
        Fmt<PREC>::split2(c0, c1, h.x, l.x);
        Fmt<PREC>::split2(c2, 0.f, h.y, l.y);
        *reinterpret_cast<uint4 *>(smem + slot * SLOTB + lpos) = h;
        if constexpr (PARTS == 2) *reinterpret_cast<uint4 *>(smem + slot * SLOTB + PLANEB + lpos) = l;
    };

    // ---- per-lane constants (of_roll8's) --------------------------------------------------------------------------------
    constexpr int TA = 2;
    const int nA = wave < 2 ? 2 : 1;
    constexpr int APAIRS = TYT * (TXT / 2);
    int pa[TA], ta_y[TA], ta_x[TA], ta_st[TA];
    bool ta_ok[TA];
#pragma unroll
    for (int j = 0; j < TA; ++j) {
        const int tile = j == 0 ? wave : 4 + wave;
        int pi = tile * 16 + r;
        ta_ok[j] = pi < APAIRS;
        if (pi >= APAIRS) pi = APAIRS - 1;
        const int row = pi / (TXT / 2), pc = pi - row * (TXT / 2);
        ta_y[j] = row;
        ta_x[j] = 2 * pc + (g >> 1);
        pa[j] = (row * XX + ((g & 1) ? XX / 2 : 0) + pc + (g >> 1)) * PIXB;
        ta_st[j] = T_OFF + (row * TXT + ((g >> 1) ? TXT / 2 : 0) + pc) * PIXB + (g & 1) * 8;
    }
    const int pb_pi = wave * 16 + r, pb_y = pb_pi / (TX / 2), pb_pc = pb_pi % (TX / 2), pb_x = 2 * pb_pc + (g >> 1);
    const int pbo = (pb_y * TXT + ((g & 1) ? TXT / 2 : 0) + pb_pc + (g >> 1)) * PIXB;
    const int pb_sc = ((pb_y + 2) * XX + ((g & 1) ? XX / 2 : 0) + pb_pc + 1) * PIXB;
    short8 w0[3][PARTS], w2[3][PARTS], wsc[PARTS];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) {
            w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
            w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
        }
#pragma unroll
    for (int pt = 0; pt < PARTS; ++pt) wsc[pt] = reinterpret_cast<const short8 *>(a.w2)[(3 * PARTS + pt) * 64 + lane];
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(a.b0 + (g & 1) * 4);
    const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + (g & 1) * 4);
    auto tile_mma = [&](const unsigned char *base, int rowB, int loB, const short8 (&wf)[3][PARTS], f32x4 acc) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const short8 xh = *reinterpret_cast<const short8 *>(base + k * rowB);
            if constexpr (PARTS == 2) {
                const short8 xl = *reinterpret_cast<const short8 *>(base + k * rowB + loB);
                acc = mma<F16>(wf[k][1], xh, acc);
                acc = mma<F16>(wf[k][0], xl, acc);
            }
            acc = mma<F16>(wf[k][0], xh, acc);
        }
        return acc;
    };

    Unit U = decode(ufirst);
    issue(U, 0);
    int slot = 0;
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        const Unit Ucur = U;
        for (int s = 0; s < a.N; ++s) {
            land(slot);
            const bool more = s + 1 < a.N || cu + wgs_per_xcd < uend;
            if (s + 1 == a.N && more) U = decode(cu + wgs_per_xcd);
            if (more) issue(U, s + 1 < a.N ? s + 1 : 0);
            __syncthreads();
            const unsigned char *xs = smem + slot * SLOTB;
            // ---- stage A: t = relu(conv.0(x) + shift) on the 10 x 18 region, zero outside the image ----------------------------
#pragma unroll
            for (int j = 0; j < TA; ++j) {
                if (j >= nA) break;
                const f32x4 acc = tile_mma(xs + pa[j], XX * PIXB, PLANEB, w0, b0);
                const int iy = Ucur.gy0 - 1 + ta_y[j], ix = Ucur.gx0 - 1 + ta_x[j];
                const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                if (ta_ok[j]) {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_lim_bits(acc[0], inside ? 0x7f800000 : 0), relu_lim_bits(acc[1], inside ? 0x7f800000 : 0), h01, l01);
                    Fmt<PREC>::split2(relu_lim_bits(acc[2], inside ? 0x7f800000 : 0), relu_lim_bits(acc[3], inside ? 0x7f800000 : 0), h23, l23);
                    *reinterpret_cast<uint2 *>(smem + ta_st[j]) = make_uint2(h01, h23);
                    if constexpr (PARTS == 2) *reinterpret_cast<uint2 *>(smem + ta_st[j] + TPLANEB) = make_uint2(l01, l23);
                }
            }
            __syncthreads();
            // ---- stage B: out = relu(conv.2(t) + shift + shortcut(x)) -------------------------------------------------------------
            {
                f32x4 acc = tile_mma(smem + T_OFF + pbo, TXT * PIXB, TPLANEB, w2, b2);
                const short8 sh = *reinterpret_cast<const short8 *>(xs + pb_sc);
                if constexpr (PARTS == 2) {
                    const short8 sl = *reinterpret_cast<const short8 *>(xs + PLANEB + pb_sc);
                    acc = mma<F16>(wsc[1], sh, acc);
                    acc = mma<F16>(wsc[0], sl, acc);
                }
                acc = mma<F16>(wsc[0], sh, acc);
                uint32_t h01, h23, l01, l23;
                Fmt<PREC>::split2(relu_bits(acc[0]), relu_bits(acc[1]), h01, l01);
                Fmt<PREC>::split2(relu_bits(acc[2]), relu_bits(acc[3]), h23, l23);
                const int64_t pix = (((int64_t)Ucur.b * a.N + s) * a.H + Ucur.gy0 + pb_y) * a.W + Ucur.gx0 + pb_x;
                if constexpr (PARTS == 2) {
                    swap16(h01, l01);
                    swap16(h23, l23);
                    *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C) = make_uint4(h01, h23, l01, l23);
                } else {
                    *reinterpret_cast<uint2 *>(a.out + pix * rec + (g & 1) * 4) = make_uint2(h01, h23);
                }
            }
            slot ^= 1;
        }
    }
}

static const SrdRow kOfFirst[] = {DFFW_ROW(256, of_first_kernel, 0), DFFW_ROW(256, of_first_kernel, 1), DFFW_ROW(256, of_first_kernel, 2)};   // [prec]
void of_first_kernel_name(int prec, char *buf, int n) { copy_row_name(prec_row(kOfFirst, prec, 1, 0), buf, n); }
hipError_t launch_of_first(int prec, const SrdArgs &a, hipStream_t s) {
    return launch_row(prec_row(kOfFirst, prec, 1, 0), a.total_tiles, a.wgs > 0 ? a.wgs : 1024, 1, s, a);
}

// one operand fragment (hi [+ lo] plane) of an of_roll tile, and the counted wait that releases it (DS operations retire in order: `left` =
// operations requested after it that may still be in flight; the "+v" ties keep the MFMAs behind the wait)
template <int PARTS, int LOB>
__device__ __forceinline__ void of_read(unsigned ad, short8 &h, short8 &l) {
    asm volatile("ds_read_b128 %0, %1" : "=v"(h) : "v"(ad));
    if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(l) : "v"(ad), "n"(LOB));
}
template <int PARTS>
__device__ __forceinline__ void of_wait(int left, short8 &h, short8 &l) {
    if constexpr (PARTS == 1) {
        (void)l;
        if (left >= 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(h));
        else if (left >= 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(h));
        else if (left >= 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(h));
        else if (left >= 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(h));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h));
        return;
    }
    if (left >= 10) asm volatile("s_waitcnt lgkmcnt(10)" : "+v"(h), "+v"(l));
    else if (left >= 8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(h), "+v"(l));
    else if (left >= 6) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(h), "+v"(l));
    else if (left >= 5) asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(h), "+v"(l));
    else if (left >= 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(h), "+v"(l));
    else if (left >= 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(h), "+v"(l));
    else if (left >= 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(h), "+v"(l));
    else if (left >= 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(h), "+v"(l));
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h), "+v"(l));
}

// ---- of_roll: a stride-1 residual block of the alignment network (End_to_End.py:135-145, `OF_feature.0`, `OF_feature.1`) -------
//     out = relu( conv1x1x1(x) + BN(conv1x3x3(relu(BN(conv1x3x3(x))))) ),   8 (3 real) or 16 -> 16 channels, full resolution
// As two launches t = relu(BN(conv(x))) went through HBM and the second conv re-read x for the folded shortcut (two 16-channel
// stages + a mostly empty third one).  Here, as in srd_roll16: x slices stream through an LDS FIFO, stage A leaves t in LDS,
// stage B contracts t (5 chunks) plus ONE extra chunk for the 1x1x1 shortcut (the centre pixel of x, already in LDS) and stores
// the block's output.  Slices are independent (no attention), so a step is A -> barrier -> B -> barrier.
// SUMS (the pair of 16 -> 16 convs in the middle of the level-1 alignment head, whose result only feeds the head's last conv + plane
// mean = plane sums, dffw_kernels.hip "alpha head tail"): the block's output is not stored; instead every (column, slice) leaves 18
// 16-channel fp32 vectors in a.out (as float[(plane * tiles + tile) * 288 + k * 16 + c], plane = b * N + slice): k = 3w, 3w+1, 3w+2 the
// sum over wave w's two rows of the 8 x 16 tile, over their first and over their last pixel; 12 / 13 the tile's first / last row;
// 14..17 its corner pixels (top-left, top-right, bottom-left, bottom-right); head_tail_finish_tiles_kernel adds them up in a fixed order.
template <int PREC, bool CIN8, bool SUMS = false>
__global__ __launch_bounds__(256) void of_roll_kernel(const SrdArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int C = 16, CI = CIN8 ? 8 : 16, TY = 8, TX = 16, NWAVES = 4;
    constexpr int XY = TY + 4, XX = TX + 4, XPIX = XY * XX;
    constexpr int TYT = TY + 2, TXT = TX + 2, TPIX = TYT * TXT;
    constexpr int PIXB = C * 2, XPIXB = CI * 2, XOCT = CI / 8;
    constexpr int NPIECE = (XPIX * XOCT + 63) / 64;                // 1 KiB wave instructions per plane
    constexpr int PLANEB = NPIECE * 1024;
    constexpr int SLOTB = PARTS * PLANEB;
    constexpr int RX = CIN8 ? 4 : 3;
    constexpr int NP = PARTS * NPIECE, PPW = (NP + NWAVES - 1) / NWAVES;
    static_assert(NP % PPW == 0, "every wave issues PPW pieces or none (counted vmcnt waits)");
    constexpr int TPLANEB = TPIX * PIXB;
    constexpr int X_OFF = 0, T_OFF = RX * SLOTB;
    constexpr int NCHA = CIN8 ? 3 : 5, NCHB = 5;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[T_OFF + PARTS * TPLANEB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    auto lds_store8 = [&](unsigned byte_off, uint32_t v0, uint32_t v1) {
        const u32x2 d = {v0, v1};
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds0 + byte_off), "v"(d) : "memory");
    };

    const UnitRange ur = persistent_range(a.total_tiles);   // dffw_persist.h
    const int ufirst = ur.first, uend = ur.end, wgs_per_xcd = ur.step;
    if (ufirst >= uend) return;
    struct Unit {
        int b, gy0, gx0;
    };
    auto decode = [&](int u) {
        Unit c;
        const int txi = u % a.tiles_x;
        const int tt = u / a.tiles_x;
        c.b = tt / a.tiles_y;
        c.gy0 = (tt % a.tiles_y) * TY;
        c.gx0 = txi * TX;
        return c;
    };

    const int rec = PARTS * C, xrec = PARTS * CI;
    const int slice_elems = a.H * a.W * xrec;
    const uint16_t *fsrc[PPW];
    bool fok[PPW];
    int fu = ufirst, fq = 0;
    auto setup_fill = [&]() {
        const Unit c = decode(fu);
#pragma unroll
        for (int k = 0; k < PPW; ++k) {
            const int p = wave * PPW + k;
            const int part = p / NPIECE, i = p % NPIECE;
            const int ci = i * 64 + lane, pix = ci / XOCT, oct = ci % XOCT;
            const int fy = pix / XX, fx = pix - fy * XX;
            const int iy = c.gy0 - 2 + fy, ix = c.gx0 - 2 + fx;
            fok[k] = p < NP && pix < XPIX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            fsrc[k] = a.x + (int64_t)c.b * a.N * slice_elems + (int64_t)(iy * a.W + ix) * xrec + part * CI + oct * 8;
        }
    };
    setup_fill();
    int fslot = 0;
    auto issue_next = [&]() {
        const bool zin = fu < uend;
        unsigned char *slot = smem + X_OFF + fslot * SLOTB;
        const int64_t zo = (int64_t)fq * slice_elems;
#pragma unroll
        for (int k = 0; k < PPW; ++k) {
            const int p = wave * PPW + k;
            if (p >= NP) break;
            const int part = p / NPIECE, i = p % NPIECE;
            const uint16_t *src = (zin && fok[k]) ? fsrc[k] + zo : a.zero;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(slot + part * PLANEB + i * 1024), 16, 0, 0);
        }
        fslot = (fslot + 1 == RX) ? 0 : fslot + 1;
        if (++fq == a.N && fu < uend) {
            fq = 0;
            fu += wgs_per_xcd;
            if (fu < uend) setup_fill();
        }
    };

    // stage A: the 10 x 18 t pixels are 12 operand tiles, three per wave: tiles 0-9 = the first 16 pixels of row 0-9 (16 consecutive pixels of ONE
    // row: conflict-free operand reads; tiles of 16 consecutive indices of the region wrapped rows and collided two ways, as in srd_roll16 before
    // round 4), tiles 10-11 = the two remaining pixels of each row (the last one a quarter busy)
    constexpr int TA = 3;
    int pa[TA], ta_y[TA], ta_x[TA], ta_st[TA];
    bool ta_ok[TA];
#pragma unroll
    for (int j = 0; j < TA; ++j) {
        const int tile = wave * TA + j;
        const int q = (tile - TYT) * 16 + r;                       // index among the 2 * TYT left-over pixels
        ta_ok[j] = tile < TYT || q < 2 * TYT;
        ta_y[j] = tile < TYT ? tile : (q < 2 * TYT ? q >> 1 : TYT - 1);
        ta_x[j] = tile < TYT ? r : TX + (q & 1);
        pa[j] = (ta_y[j] * XX + ta_x[j]) * XPIXB + (CIN8 ? 0 : (g & 1) * 16);
        ta_st[j] = T_OFF + (ta_y[j] * TXT + ta_x[j]) * PIXB + g * 8;
    }
    // K octets: 8 input channels: chunk k, octet g = filter tap 4k + g; 16 channels: (tap 2k + (g >> 1), channel octet g & 1);
    // taps >= 9 carry zero weights
    int tapA[NCHA], tapB[NCHB];
#pragma unroll
    for (int k = 0; k < NCHA; ++k) {
        const int tap = CIN8 ? 4 * k + g : 2 * k + (g >> 1);
        const int dy = tap < 9 ? tap / 3 : 0, dx = tap < 9 ? tap % 3 : 0;
        tapA[k] = (dy * XX + dx) * XPIXB;
    }
#pragma unroll
    for (int k = 0; k < NCHB; ++k) {
        const int tap = 2 * k + (g >> 1);
        const int dy = tap < 9 ? tap / 3 : 0, dx = tap < 9 ? tap % 3 : 0;
        tapB[k] = (dy * TXT + dx) * PIXB;
    }
    // stage B: wave w = output rows 2w, 2w+1
    constexpr int TB = 2;
    int pbo[TB], pbx[TB];
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        const int fy = wave * TB + j;
        pbo[j] = (fy * TXT + r) * PIXB + (g & 1) * 16;
        pbx[j] = ((fy + 2) * XX + r + 2) * XPIXB + (g < XOCT ? g : 0) * 16;   // shortcut chunk: channel octet g of the centre pixel of x
    }
    short8 w0[NCHA][PARTS], w2[NCHB + 1][PARTS];   // conv.2: 5 chunks over t + the shortcut chunk over x
#pragma unroll
    for (int k = 0; k < NCHA; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int k = 0; k < NCHB + 1; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(a.b0 + g * 4);
    const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + g * 4);
    constexpr int INFLIGHT = (RX - 2) * PPW;
#pragma unroll
    for (int q = 0; q < RX - 1; ++q) issue_next();
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("s_barrier" ::: "memory");

    int xslot = 0;
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        const Unit U = decode(cu);
        for (int s = 0; s < a.N; ++s) {
            // (1) this step's x slice has landed (for every wave after the barrier); stage B of the previous step has read t
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(INFLIGHT) : "memory");
            const unsigned xs = lds0 + X_OFF + xslot * SLOTB;
            // ---- stage A: t = relu(conv.0(x) + shift) on the 10 x 18 region, zero outside the image (conv.2's padding) ------------
            // operand reads run one tile ahead: chunk k of tile j+1 is requested as soon as chunk k of tile j has been contracted (into the same
            // registers), so only the stage's first tile waits for the LDS.  DS operations retire in order: behind the reads of (j, k) there are
            // the 2 (NC-1-k) reads of the tile's later chunks, the 2k already requested for tile j+1 and at most the 2 stores of tile j-1's
            // epilogue -- lgkmcnt(2 (NC-1)) covers (j, k) whether or not the stores were issued.
            short8 fxh[NCHB + 1], fxl[NCHB + 1];
#pragma unroll
            for (int k = 0; k < NCHA; ++k) of_read<PARTS, PLANEB>(xs + pa[0] + tapA[k], fxh[k], fxl[k]);
#pragma unroll
            for (int j = 0; j < TA; ++j) {
                f32x4 acc = b0;
#pragma unroll
                for (int k = 0; k < NCHA; ++k) {
                    of_wait<PARTS>(j + 1 < TA ? (NCHA - 1) * PARTS : (NCHA - 1 - k) * PARTS, fxh[k], fxl[k]);
                    if constexpr (PARTS == 2) {
                        acc = mma<F16>(w0[k][1], fxh[k], acc);
                        acc = mma<F16>(w0[k][0], fxl[k], acc);
                    }
                    acc = mma<F16>(w0[k][0], fxh[k], acc);
                    if (j + 1 < TA) of_read<PARTS, PLANEB>(xs + pa[j + 1] + tapA[k], fxh[k], fxl[k]);
                }
                const int iy = U.gy0 - 1 + ta_y[j], ix = U.gx0 - 1 + ta_x[j];
                const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                if (ta_ok[j]) {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_lim_bits(acc[0], inside ? 0x7f800000 : 0), relu_lim_bits(acc[1], inside ? 0x7f800000 : 0), h01, l01);
                    Fmt<PREC>::split2(relu_lim_bits(acc[2], inside ? 0x7f800000 : 0), relu_lim_bits(acc[3], inside ? 0x7f800000 : 0), h23, l23);
                    lds_store8(ta_st[j], h01, h23);
                    if constexpr (PARTS == 2) lds_store8(ta_st[j] + TPLANEB, l01, l23);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // ---- stage B: out = relu(conv.2(t) + shift + shortcut(x)) -----------------------------------------------------------
            f32x4 sum_t = {0.f, 0.f, 0.f, 0.f}, sum_c = sum_t;   // SUMS only
            // (chunk NCHB = the shortcut chunk: centre pixel of x, its channel octets as K octets -- weights of absent octets are zeros; reads one
            // tile ahead as in stage A: 2 NCHB operations behind the reads of (j, k), no DS stores in this stage)
#pragma unroll
            for (int k = 0; k < NCHB; ++k) of_read<PARTS, TPLANEB>(lds0 + T_OFF + pbo[0] + tapB[k], fxh[k], fxl[k]);
            of_read<PARTS, PLANEB>(xs + pbx[0], fxh[NCHB], fxl[NCHB]);
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                f32x4 acc = b2;
#pragma unroll
                for (int k = 0; k <= NCHB; ++k) {
                    of_wait<PARTS>(j + 1 < TB ? NCHB * PARTS : (NCHB - k) * PARTS, fxh[k], fxl[k]);
                    if constexpr (PARTS == 2) {
                        acc = mma<F16>(w2[k][1], fxh[k], acc);
                        acc = mma<F16>(w2[k][0], fxl[k], acc);
                    }
                    acc = mma<F16>(w2[k][0], fxh[k], acc);
                    if (j + 1 < TB) {
                        if (k < NCHB) of_read<PARTS, TPLANEB>(lds0 + T_OFF + pbo[j + 1] + tapB[k], fxh[k], fxl[k]);
                        else of_read<PARTS, PLANEB>(xs + pbx[j + 1], fxh[k], fxl[k]);
                    }
                }
                if constexpr (SUMS) {
                    // this lane: channels 4g..4g+3 of pixel (row 2*wave + j, column r).  Row sums over the 16 lanes of the row group by
                    // DPP (quad xor 1, xor 2, half-row mirror, row mirror: every lane ends up with the sum); lanes r = 0 / r = 15 are
                    // the tile's first / last column.  Everything leaves straight from registers (16-byte stores of lanes r = 0 / 15).
                    f32x4 v, rs;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v[i] = relu_bits(acc[i]);
                        float t = v[i];
                        t += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
                        t += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
                        t += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0x141, 0xF, 0xF, true));   // row_half_mirror
                        t += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0x140, 0xF, 0xF, true));   // row_mirror
                        rs[i] = t;
                    }
                    float *trec = reinterpret_cast<float *>(a.out) +
                                  (((int64_t)U.b * a.N + s) * (a.tiles_y * a.tiles_x) + (U.gy0 / TY) * a.tiles_x + U.gx0 / TX) * (18 * C) + g * 4;
                    if (j == 0) {
                        sum_t = rs;
                        sum_c = v;
                        if (wave == 0 && r == 0) *reinterpret_cast<f32x4 *>(trec + 12 * C) = rs;          // first row of the tile
                        if (wave == 0 && (r == 0 || r == 15)) *reinterpret_cast<f32x4 *>(trec + (r == 0 ? 14 : 15) * C) = v;   // TL, TR
                    } else {
                        sum_t += rs;
                        sum_c += v;
                        if (wave == NWAVES - 1 && r == 0) *reinterpret_cast<f32x4 *>(trec + 13 * C) = rs;  // last row
                        if (wave == NWAVES - 1 && (r == 0 || r == 15)) *reinterpret_cast<f32x4 *>(trec + (r == 0 ? 16 : 17) * C) = v;   // BL, BR
                        if (r == 0) *reinterpret_cast<f32x4 *>(trec + (wave * 3 + 0) * C) = sum_t;         // this wave's two rows
                        if (r == 0 || r == 15) *reinterpret_cast<f32x4 *>(trec + (wave * 3 + (r == 0 ? 1 : 2)) * C) = sum_c;   // ... their first / last column
                    }
                } else {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_bits(acc[0]), relu_bits(acc[1]), h01, l01);
                    Fmt<PREC>::split2(relu_bits(acc[2]), relu_bits(acc[3]), h23, l23);
                    const int64_t pix = (((int64_t)U.b * a.N + s) * a.H + U.gy0 + wave * TB + j) * a.W + U.gx0 + r;
                    if constexpr (PARTS == 2) {
                        swap16(h01, l01);
                        swap16(h23, l23);
                        *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C + (g >> 1) * 8) = make_uint4(h01, h23, l01, l23);
                    } else {
                        *reinterpret_cast<uint2 *>(a.out + pix * rec + g * 4) = make_uint2(h01, h23);
                    }
                }
            }
            // (3) the x slot is free: queue the slice RX-1 ahead into it
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            issue_next();
            xslot = (xslot + 1 == RX) ? 0 : xslot + 1;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- head_warp: the first conv of an alignment head on the FOV-warped features, without the warped volume -------------------------
// (End_to_End.py:88-101: FE = FOV_warp(FE, alpha); conv over [ref | cur | flow]; the ref part enters as `ref`, see head_first_conv() in dffw_align.cpp)
//     y0[b,n] = relu( BN(conv1x3x3([warp(fe)[b,n] (CF) | flow_x, flow_y])) + ref[b] )       CF + 2 -> 2 CF channels
// CF = 8: level 1 (full resolution), CF = 16: level 2 (half resolution).  As two launches flow_volume wrote the volume
// [cur | flow | pad] (1.6 GB at 8 x 10 x 480 x 640 for level 1) and the conv read it back.  Here a workgroup walks the slices of a
// column of 8 x 16 output pixels: every channel octet of every pixel of the 10 x 18 footprint has its thread, which gathers the four
// bilinear corners (hi and lo piece each) ONE STEP AHEAD into registers -- the loads of slice s+1 travel under the contraction and
// the stores of slice s -- blends them with the operation order of flow_volume_kernel (warp_octet), splits to the storage format and
// writes its octet of the record [CF channels | flow_x flow_y 0..] into one of two LDS slots; the contraction (CF = 8: 4 waves, wave
// w = output rows 2w, 2w+1; CF = 16: 8 waves, wave w = row w, two 16-channel output tiles; K octet g of chunk k = o = 4k + g ->
// (tap o / OCT, channel octet o % OCT), OCT = CF / 8 + 1; filter resident in LDS) and the epilogue (+ ref, held in registers for all
// slices of the column, ReLU, split, 16-byte stores) follow after one barrier.  Plain loads only (no LDS-DMA): hipcc counts every wait.
#ifndef DFFW_HW_ABL
#define DFFW_HW_ABL 0   // dev-only ablations (tools/build_variant_lib.sh): 1 no corner loads, 2 no output stores, 4 no MFMAs, 8 no blend
#endif
template <int PREC, int CF>
__global__ __launch_bounds__(CF == 8 ? 256 : 512) __attribute__((amdgpu_waves_per_eu(4))) void head_warp_kernel(const HeadWarpArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int GO = CF / 8, OCT = GO + 1, NT = CF / 8, C = 16 * NT;
    constexpr int NWAVES = CF == 8 ? 4 : 8, NTHR = NWAVES * 64;
    constexpr int TY = 8, TX = 16, XY = TY + 2, XX = TX + 2, XPIX = XY * XX;
    constexpr int PIXB = OCT * 16, PLANEB = XPIX * PIXB, SLOTB = PARTS * PLANEB;
    constexpr int NCH = (9 * OCT + 3) / 4, TB = TY / NWAVES;
    constexpr int W_OFF = 2 * SLOTB, WB = NCH * NT * PARTS * 1024;   // the filter: [chunk][output tile][part][64 lanes][16 bytes]
    // the warp parameters of every (sample, slice): (alpha0 + fov, alpha1, alpha2), read from LDS in issue().  As global loads (wave-uniform addresses, but
    // hipcc issues vector loads for them) every step waited vmcnt(0) for them -- with the previous step's result stores in the same queue: a store
    // acknowledgement per step on the critical path (with every load, store, MFMA and blend taken out the kernel still ran 0.51 of its 0.73 ms:
    // profiles/r06_head_warp.txt).  B N <= head_warp_max_planes(); the engine keeps the two-launch form beyond.
    constexpr int PRM_OFF = W_OFF + WB, PRM_MAX = head_warp_max_planes();
    static_assert(XPIX * GO <= NTHR, "one gather item per thread");
    __shared__ __attribute__((aligned(16))) unsigned char smem[PRM_OFF + PRM_MAX * 12];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const UnitRange ur = persistent_range(a.total_tiles);   // dffw_persist.h
    const int ufirst = ur.first, uend = ur.end, wgs_per_xcd = ur.step;
    if (ufirst >= uend) return;
    struct Unit {
        int b, gy0, gx0;
    };
    auto decode = [&](int u) {
        Unit c;
        const int txi = u % a.tiles_x;
        const int tt = u / a.tiles_x;
        c.b = tt / a.tiles_y;
        c.gy0 = (tt % a.tiles_y) * TY;
        c.gx0 = txi * TX;
        return c;
    };
    const int rec = PARTS * C, frec = PARTS * CF;
    for (int i = tid; i < WB / 16; i += NTHR) reinterpret_cast<uint4 *>(smem + W_OFF)[i] = reinterpret_cast<const uint4 *>(a.w)[i];
    float *prm = reinterpret_cast<float *>(smem + PRM_OFF);
    for (int i = tid; i < a.B * a.N; i += NTHR) {
        const int b = i / a.N, n = i - b * a.N;
        prm[i * 3 + 0] = a.alpha[b * 3 * a.N + n] + a.fov[i];
        prm[i * 3 + 1] = a.alpha[b * 3 * a.N + a.N + n];
        prm[i * 3 + 2] = a.alpha[b * 3 * a.N + 2 * a.N + n];
    }
    __syncthreads();

    // ---- gather side: thread t < 180 * GO owns channel octet t / 180 of footprint pixel t % 180 ---------------------
    const bool gth = tid < XPIX * GO;
    const int goct = GO == 1 ? 0 : tid / XPIX, gp = tid - goct * XPIX;
    const int fy = gp / XX, fx = gp - fy * XX;
    uint4 q[4][PARTS];          // corner k: [hi, lo]
    float wgt[4], flx = 0.f, fly = 0.f;
    bool pin = false;
    auto issue = [&](const Unit &U, int n) {
        const int iy = U.gy0 - 1 + fy, ix = U.gx0 - 1 + fx;
        pin = gth && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        if (!pin) return;
        const int pi = (U.b * a.N + n) * 3;
        const WarpPoint wp = warp_point(ix, iy, a.H, a.W, prm[pi], prm[pi + 1], prm[pi + 2]);
        flx = wp.fx;
        fly = wp.fy;
        const float x0f = floorf(wp.sx), y0f = floorf(wp.sy);
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float wx1 = wp.sx - x0f, wy1 = wp.sy - y0f;
        const float wx[2] = {1.0f - wx1, wx1}, wy[2] = {1.0f - wy1, wy1};
        const uint16_t *slice = a.fe + ((int64_t)(U.b * a.N + n) * a.H * a.W) * frec + goct * 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yc = y0 + (k >> 1), xc = x0 + (k & 1);
            const bool ok = (unsigned)yc < (unsigned)a.H && (unsigned)xc < (unsigned)a.W;
            wgt[k] = ok ? wx[k & 1] * wy[k >> 1] : 0.f;
            const uint16_t *rp = slice + (ok ? (yc * a.W + xc) * frec : 0);
#pragma unroll
            for (int i = 0; i < PARTS; ++i) {
                if constexpr (DFFW_HW_ABL & 1) q[k][i] = make_uint4(ix, iy, n, k);
                else q[k][i] = *reinterpret_cast<const uint4 *>(rp + i * CF);
            }
        }
    };
    auto land = [&](int slot) {     // blend the corners requested by the last issue(), write the octet (octet-0 threads: also the flow record)
        if (!gth) return;
        unsigned char *dst = smem + slot * SLOTB + gp * PIXB;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (pin && !(DFFW_HW_ABL & 8)) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (wgt[k] == 0.f) continue;      // corner outside the image (or weight exactly 0): skipped, as warp_octet skips it
                const uint4 h = q[k][0];
                uint4 l = make_uint4(0, 0, 0, 0);
                if constexpr (PARTS == 2) l = q[k][1];
                float x, y;
                Fmt<PREC>::join2(h.x, l.x, x, y); v[0] += x * wgt[k]; v[1] += y * wgt[k];
                Fmt<PREC>::join2(h.y, l.y, x, y); v[2] += x * wgt[k]; v[3] += y * wgt[k];
                Fmt<PREC>::join2(h.z, l.z, x, y); v[4] += x * wgt[k]; v[5] += y * wgt[k];
                Fmt<PREC>::join2(h.w, l.w, x, y); v[6] += x * wgt[k]; v[7] += y * wgt[k];
            }
        }
        uint4 h, l;
        Fmt<PREC>::split2(v[0], v[1], h.x, l.x);
        Fmt<PREC>::split2(v[2], v[3], h.y, l.y);
        Fmt<PREC>::split2(v[4], v[5], h.z, l.z);
        Fmt<PREC>::split2(v[6], v[7], h.w, l.w);
        *reinterpret_cast<uint4 *>(dst + goct * 16) = h;
        if constexpr (PARTS == 2) *reinterpret_cast<uint4 *>(dst + PLANEB + goct * 16) = l;
        if (goct == 0) {
            uint4 fh = make_uint4(0, 0, 0, 0), fl = fh;
            if (pin) Fmt<PREC>::split2(flx, fly, fh.x, fl.x);
            *reinterpret_cast<uint4 *>(dst + GO * 16) = fh;
            if constexpr (PARTS == 2) *reinterpret_cast<uint4 *>(dst + PLANEB + GO * 16) = fl;
        }
    };

    // ---- contraction side ----------------------------------------------------------------------------------------
    int pofs[TB], tapo[NCH];
#pragma unroll
    for (int j = 0; j < TB; ++j) pofs[j] = ((wave * TB + j) * XX + r) * PIXB;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int o = 4 * k + g, tap = o < 9 * OCT ? o / OCT : 0, oct = o < 9 * OCT ? o % OCT : 0;   // (octets >= 9 OCT carry zero weights)
        tapo[k] = ((tap / 3) * XX + tap % 3) * PIXB + oct * 16;
    }
    const unsigned char *wl = smem + W_OFF + lane * 16;
    f32x4 b0[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b0[nt] = *reinterpret_cast<const f32x4 *>(a.bias + nt * 16 + g * 4);

    Unit U = decode(ufirst);
    issue(U, 0);
    int slot = 0;
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        // the reference part of this column: 4 channels per output tile of the lane's output pixels, added in front of the ReLU of every slice
        f32x4 rv[TB][NT];
#pragma unroll
        for (int j = 0; j < TB; ++j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const uint16_t *rp = a.ref + (((int64_t)U.b * a.H + U.gy0 + wave * TB + j) * a.W + U.gx0 + r) * rec + nt * 16 + g * 4;
                const uint2 h = *reinterpret_cast<const uint2 *>(rp);
                uint2 l = make_uint2(0, 0);
                if constexpr (PARTS == 2) l = *reinterpret_cast<const uint2 *>(rp + C);
                float r0, r1, r2, r3;
                Fmt<PREC>::join2(h.x, l.x, r0, r1);
                Fmt<PREC>::join2(h.y, l.y, r2, r3);
                rv[j][nt] = f32x4{r0, r1, r2, r3} + b0[nt];
            }
        const Unit Ucur = U;
        for (int s = 0; s < a.N; ++s) {
            land(slot);
            __builtin_amdgcn_sched_barrier(0);
            // next step's corners: the following slice of this column, or the first slice of the workgroup's next column
            const bool more = s + 1 < a.N || cu + wgs_per_xcd < uend;
            if (s + 1 == a.N && more) U = decode(cu + wgs_per_xcd);
            if (more) issue(U, s + 1 < a.N ? s + 1 : 0);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            const unsigned char *xs = smem + slot * SLOTB;
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                f32x4 acc[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt] = rv[j][nt];
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const short8 xh = *reinterpret_cast<const short8 *>(xs + pofs[j] + tapo[k]);
                    short8 xl = xh;
                    if constexpr (PARTS == 2) xl = *reinterpret_cast<const short8 *>(xs + PLANEB + pofs[j] + tapo[k]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const short8 wh = *reinterpret_cast<const short8 *>(wl + ((k * NT + nt) * PARTS) * 1024);
                        if constexpr (DFFW_HW_ABL & 4) {
                            acc[nt][0] += __builtin_bit_cast(float, (int)xh[0] + (int)xl[1] + (int)wh[0]);
                            continue;
                        }
                        if constexpr (PARTS == 2) {
                            const short8 wlo = *reinterpret_cast<const short8 *>(wl + ((k * NT + nt) * PARTS + 1) * 1024);
                            acc[nt] = mma<F16>(wlo, xh, acc[nt]);
                            acc[nt] = mma<F16>(wh, xl, acc[nt]);
                        }
                        acc[nt] = mma<F16>(wh, xh, acc[nt]);
                    }
                    if (CF == 8 ? k == 2 : ((k & 1) == 0 && k > 0)) __builtin_amdgcn_sched_barrier(0);   // (every fragment of the row in flight at once: +40 registers)
                }
                const int64_t pix = (((int64_t)Ucur.b * a.N + s) * a.H + Ucur.gy0 + wave * TB + j) * a.W + Ucur.gx0 + r;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_bits(acc[nt][0]), relu_bits(acc[nt][1]), h01, l01);
                    Fmt<PREC>::split2(relu_bits(acc[nt][2]), relu_bits(acc[nt][3]), h23, l23);
                    if ((DFFW_HW_ABL & 2) && h01 != 0x12345u) continue;
                    if constexpr (PARTS == 2) {
                        swap16(h01, l01);
                        swap16(h23, l23);
                        *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C + nt * 16 + (g >> 1) * 8) = make_uint4(h01, h23, l01, l23);
                    } else {
                        *reinterpret_cast<uint2 *>(a.out + pix * rec + nt * 16 + g * 4) = make_uint2(h01, h23);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            slot ^= 1;
        }
    }
}

static const KernelRow<HeadWarpArgs> kHeadWarp[] = {   // [prec][cf 8 | 16]
    DFFW_ROW(256, head_warp_kernel, 0, 8), DFFW_ROW(512, head_warp_kernel, 0, 16), DFFW_ROW(256, head_warp_kernel, 1, 8),
    DFFW_ROW(512, head_warp_kernel, 1, 16), DFFW_ROW(256, head_warp_kernel, 2, 8), DFFW_ROW(512, head_warp_kernel, 2, 16),
};
static const KernelRow<HeadWarpArgs> *select_head_warp(int prec, int cf) { return cf == 8 || cf == 16 ? prec_row(kHeadWarp, prec, 2, cf == 16) : nullptr; }
void head_warp_kernel_name(int prec, int cf, char *buf, int n) { copy_row_name(select_head_warp(prec, cf), buf, n); }
hipError_t launch_head_warp(int prec, int cf, const HeadWarpArgs &a, hipStream_t s) {
    if ((int64_t)a.B * a.N > head_warp_max_planes()) return hipErrorInvalidValue;
    return launch_row(select_head_warp(prec, cf), a.total_tiles, a.wgs > 0 ? a.wgs : (cf == 8 ? 1024 : 512), 1, s, a);
}

// ---- of_s2: the down-sampling residual block of the alignment network at 8 -> 16 channels (End_to_End.py:135-145 with stride 2,
// `OF_feature1.0`) as ONE streaming kernel ---------------------------------------------------------------------------------------
//     out = relu( conv1x1x1_s2(x) + BN(conv1x3x3(relu(BN(conv1x3x3_s2(x))))) )
// As three launches (strided conv on conv_tile, the 1x1x1 shortcut on the gather kernel, the second conv with the shortcut as a
// residual) the full-resolution input was read twice and the two half-resolution intermediates went through HBM.  Here a workgroup
// walks the slices of a column of 8 x 16 OUTPUT pixels: the 21 x 37 input footprint of a slice (two 3x3 halos, the inner one at stride
// 2) is fetched one step ahead into registers (plain 16-byte loads, one (pixel, part) piece per thread and pass) and written into one
// of two LDS slots with the even columns of a row first, so that the stride-2 operand reads of 16 neighbouring pixels stay
// contiguous; stage A computes t = relu(BN(conv.0)) on the 10 x 18 region conv.2 needs (3 chunks, K octet g of chunk k = tap 4k + g)
// into LDS records, zero outside the image; stage B contracts t (5 chunks, srd_roll16's order) plus one chunk for the shortcut (the
// input pixel under the output pixel, already in LDS) and stores the block's output.  No LDS-DMA: hipcc counts every wait itself.
template <int PREC>
__global__ __launch_bounds__(256) void of_s2_kernel(const SrdArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int CI = 8, C = 16, TY = 8, TX = 16;
    constexpr int TYT = TY + 2, TXT = TX + 2, TPIX = TYT * TXT;               // t region
    constexpr int XY = 2 * TYT + 1, XX = 2 * TXT + 1, XPIX = XY * XX, XEV = TXT + 1;   // input footprint; XEV even columns per row
    constexpr int XPIXB = CI * 2, PIXB = C * 2;
    constexpr int XPLANEB = XPIX * XPIXB, XSLOTB = PARTS * XPLANEB, TPLANEB = TPIX * PIXB;
    constexpr int T_OFF = 2 * XSLOTB;
    constexpr int NITEM = XPIX * PARTS, NPASS = (NITEM + 255) / 256;
    constexpr int NCHA = 3, NCHB = 5, TA = 3, TB = 2;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T_OFF + PARTS * TPLANEB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const UnitRange ur = persistent_range(a.total_tiles);   // dffw_persist.h
    const int ufirst = ur.first, uend = ur.end, wgs_per_xcd = ur.step;
    if (ufirst >= uend) return;
    struct Unit {
        int b, gy0, gx0;
    };
    auto decode = [&](int u) {      // columns of the OUTPUT grid (a.H x a.W = output size; the input is 2 a.H x 2 a.W)
        Unit c;
        const int txi = u % a.tiles_x;
        const int tt = u / a.tiles_x;
        c.b = tt / a.tiles_y;
        c.gy0 = (tt % a.tiles_y) * TY;
        c.gx0 = txi * TX;
        return c;
    };
    const int Hi = 2 * a.H, Wi = 2 * a.W;
    const int rec = PARTS * C, xrec = PARTS * CI;

    // ---- fill side: item = (footprint pixel, part); thread t takes items t, t + 256, ... -------------------------------
    uint4 q[NPASS];
    int ldst[NPASS];      // LDS byte offset inside a slot of the item's piece (even columns of a row first)
#pragma unroll
    for (int k = 0; k < NPASS; ++k) {
        const int item = tid + k * 256, part = item / XPIX, pix = item - part * XPIX;
        const int fy = pix / XX, fx = pix - fy * XX;
        ldst[k] = part * XPLANEB + (fy * XX + ((fx & 1) ? XEV + (fx >> 1) : (fx >> 1))) * XPIXB;
    }
    auto issue = [&](const Unit &U, int n) {
        const uint16_t *slice = a.x + ((int64_t)(U.b * a.N + n) * Hi * Wi) * xrec;
#pragma unroll
        for (int k = 0; k < NPASS; ++k) {
            const int item = tid + k * 256, part = item / XPIX, pix = item - part * XPIX;
            const int fy = pix / XX, fx = pix - fy * XX;
            const int iy = 2 * U.gy0 - 3 + fy, ix = 2 * U.gx0 - 3 + fx;
            const bool ok = item < NITEM && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
            q[k] = make_uint4(0, 0, 0, 0);
            if (ok) q[k] = *reinterpret_cast<const uint4 *>(slice + (iy * Wi + ix) * xrec + part * CI);
        }
    };
    auto land = [&](int slot) {
#pragma unroll
        for (int k = 0; k < NPASS; ++k)
            if (tid + k * 256 < NITEM) *reinterpret_cast<uint4 *>(smem + slot * XSLOTB + ldst[k]) = q[k];
    };

    // ---- stage A: the 10 x 18 t pixels are 12 operand tiles (the last one partly idle), three per wave ----------------
    int pa[TA], ta_y[TA], ta_x[TA], ta_st[TA];
    bool ta_ok[TA];
#pragma unroll
    for (int j = 0; j < TA; ++j) {
        int p = (wave * TA + j) * 16 + r;
        ta_ok[j] = p < TPIX;
        if (p >= TPIX) p = TPIX - 1;
        ta_y[j] = p / TXT;
        ta_x[j] = p - ta_y[j] * TXT;
        pa[j] = (2 * ta_y[j] * XX + ta_x[j]) * XPIXB;             // footprint pixel (2 ty, 2 tx): even column tx of row 2 ty
        ta_st[j] = T_OFF + p * PIXB + g * 8;
    }
    int tapA[NCHA], tapB[NCHB];
#pragma unroll
    for (int k = 0; k < NCHA; ++k) {
        const int tap = 4 * k + g;                                 // taps >= 9 carry zero weights
        const int dy = tap < 9 ? tap / 3 : 0, dx = tap < 9 ? tap % 3 : 0;
        tapA[k] = (dy * XX + (dx == 1 ? XEV : (dx == 2 ? 1 : 0))) * XPIXB;
    }
#pragma unroll
    for (int k = 0; k < NCHB; ++k) {
        const int tap = 2 * k + (g >> 1);
        const int dy = tap < 9 ? tap / 3 : 0, dx = tap < 9 ? tap % 3 : 0;
        tapB[k] = (dy * TXT + dx) * PIXB + (g & 1) * 16;
    }
    // ---- stage B: wave w = output rows 2w, 2w+1 ---------------------------------------------------------------------
    int pbo[TB], pbx[TB];
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        const int oy = wave * TB + j;
        pbo[j] = (oy * TXT + r) * PIXB;
        pbx[j] = ((2 * oy + 3) * XX + XEV + r + 1) * XPIXB;       // input pixel (2 oy + 3, 2 r + 3): odd column r + 1
    }
    short8 w0[NCHA][PARTS], w2[NCHB][PARTS], wsc[PARTS];
#pragma unroll
    for (int k = 0; k < NCHA; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int k = 0; k < NCHB; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int pt = 0; pt < PARTS; ++pt) wsc[pt] = reinterpret_cast<const short8 *>(a.w3f)[pt * 64 + lane];
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(a.b0 + g * 4);
    const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + g * 4);

    Unit U = decode(ufirst);
    issue(U, 0);
    int slot = 0;
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        const Unit Ucur = U;
        for (int s = 0; s < a.N; ++s) {
            land(slot);
            __builtin_amdgcn_sched_barrier(0);
            const bool more = s + 1 < a.N || cu + wgs_per_xcd < uend;
            if (s + 1 == a.N && more) U = decode(cu + wgs_per_xcd);
            if (more) issue(U, s + 1 < a.N ? s + 1 : 0);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();          // the slice is in LDS; stage B of the previous step has read t
            const unsigned char *xs = smem + slot * XSLOTB;
            // ---- stage A: t = relu(conv.0(x) + shift) on the 10 x 18 region, zero outside the image (conv.2's padding) ----------
#pragma unroll
            for (int j = 0; j < TA; ++j) {
                f32x4 acc = b0;
#pragma unroll
                for (int k = 0; k < NCHA; ++k) {
                    const short8 xh = *reinterpret_cast<const short8 *>(xs + pa[j] + tapA[k]);
                    if constexpr (PARTS == 2) {
                        const short8 xl = *reinterpret_cast<const short8 *>(xs + XPLANEB + pa[j] + tapA[k]);
                        acc = mma<F16>(w0[k][1], xh, acc);
                        acc = mma<F16>(w0[k][0], xl, acc);
                    }
                    acc = mma<F16>(w0[k][0], xh, acc);
                }
                const int iy = Ucur.gy0 - 1 + ta_y[j], ix = Ucur.gx0 - 1 + ta_x[j];
                const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                if (ta_ok[j]) {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_lim_bits(acc[0], inside ? 0x7f800000 : 0), relu_lim_bits(acc[1], inside ? 0x7f800000 : 0), h01, l01);
                    Fmt<PREC>::split2(relu_lim_bits(acc[2], inside ? 0x7f800000 : 0), relu_lim_bits(acc[3], inside ? 0x7f800000 : 0), h23, l23);
                    *reinterpret_cast<uint2 *>(smem + ta_st[j]) = make_uint2(h01, h23);
                    if constexpr (PARTS == 2) *reinterpret_cast<uint2 *>(smem + ta_st[j] + TPLANEB) = make_uint2(l01, l23);
                }
            }
            __syncthreads();
            // ---- stage B: out = relu(conv.2(t) + shift + shortcut(x)) ------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                f32x4 acc = b2;
#pragma unroll
                for (int k = 0; k < NCHB; ++k) {
                    const short8 th = *reinterpret_cast<const short8 *>(smem + T_OFF + pbo[j] + tapB[k]);
                    if constexpr (PARTS == 2) {
                        const short8 tl = *reinterpret_cast<const short8 *>(smem + T_OFF + TPLANEB + pbo[j] + tapB[k]);
                        acc = mma<F16>(w2[k][1], th, acc);
                        acc = mma<F16>(w2[k][0], tl, acc);
                    }
                    acc = mma<F16>(w2[k][0], th, acc);
                }
                {   // the shortcut chunk: K octet 0 = the 8 channels of the input pixel under the output pixel (octets 1..3: zero weights)
                    const short8 sh = *reinterpret_cast<const short8 *>(xs + pbx[j]);
                    if constexpr (PARTS == 2) {
                        const short8 sl = *reinterpret_cast<const short8 *>(xs + XPLANEB + pbx[j]);
                        acc = mma<F16>(wsc[1], sh, acc);
                        acc = mma<F16>(wsc[0], sl, acc);
                    }
                    acc = mma<F16>(wsc[0], sh, acc);
                }
                uint32_t h01, h23, l01, l23;
                Fmt<PREC>::split2(relu_bits(acc[0]), relu_bits(acc[1]), h01, l01);
                Fmt<PREC>::split2(relu_bits(acc[2]), relu_bits(acc[3]), h23, l23);
                const int64_t pix = (((int64_t)Ucur.b * a.N + s) * a.H + Ucur.gy0 + wave * TB + j) * a.W + Ucur.gx0 + r;
                if constexpr (PARTS == 2) {
                    swap16(h01, l01);
                    swap16(h23, l23);
                    *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C + (g >> 1) * 8) = make_uint4(h01, h23, l01, l23);
                } else {
                    *reinterpret_cast<uint2 *>(a.out + pix * rec + g * 4) = make_uint2(h01, h23);
                }
            }
            slot ^= 1;
        }
    }
}

static const SrdRow kOfS2[] = {DFFW_ROW(256, of_s2_kernel, 0), DFFW_ROW(256, of_s2_kernel, 1), DFFW_ROW(256, of_s2_kernel, 2)};   // [prec]
void of_s2_kernel_name(int prec, char *buf, int n) { copy_row_name(prec_row(kOfS2, prec, 1, 0), buf, n); }
hipError_t launch_of_s2(int prec, const SrdArgs &a, hipStream_t s) { return launch_row(prec_row(kOfS2, prec, 1, 0), a.total_tiles, a.wgs > 0 ? a.wgs : 512, 1, s, a); }

static const SrdRow kOfRoll8[] = {DFFW_ROW(256, of_roll8_kernel, 0), DFFW_ROW(256, of_roll8_kernel, 1), DFFW_ROW(256, of_roll8_kernel, 2)};   // [prec]
void of_roll8_kernel_name(int prec, char *buf, int n) { copy_row_name(prec_row(kOfRoll8, prec, 1, 0), buf, n); }
hipError_t launch_of_roll8(int prec, const SrdArgs &a, hipStream_t s) { return launch_row(prec_row(kOfRoll8, prec, 1, 0), a.total_tiles, a.wgs > 0 ? a.wgs : 768, 1, s, a); }

static const SrdRow kOfRoll[] = {   // [prec][16 input channels | 8 | 16 with sums]
    // the first two of a precision: labels, not the symbols (which end in the defaulted ", false"): the spelling the tests and the profile tools were recorded with
    {"dffw::of_roll_kernel<0, false>", of_roll_kernel<0, false>, 256}, {"dffw::of_roll_kernel<0, true>", of_roll_kernel<0, true>, 256}, DFFW_ROW(256, of_roll_kernel, 0, false, true),
    {"dffw::of_roll_kernel<1, false>", of_roll_kernel<1, false>, 256}, {"dffw::of_roll_kernel<1, true>", of_roll_kernel<1, true>, 256}, DFFW_ROW(256, of_roll_kernel, 1, false, true),
    {"dffw::of_roll_kernel<2, false>", of_roll_kernel<2, false>, 256}, {"dffw::of_roll_kernel<2, true>", of_roll_kernel<2, true>, 256}, DFFW_ROW(256, of_roll_kernel, 2, false, true),
};
static const SrdRow *select_of_roll(int prec, bool cin8, bool sums) { return sums && cin8 ? nullptr : prec_row(kOfRoll, prec, 3, sums ? 2 : cin8); }
void of_roll_kernel_name(int prec, bool cin8, char *buf, int n, bool sums) { copy_row_name(select_of_roll(prec, cin8, sums), buf, n); }
hipError_t launch_of_roll(int prec, bool cin8, const SrdArgs &a, hipStream_t s, bool sums) {
    return launch_row(select_of_roll(prec, cin8, sums), a.total_tiles, a.wgs > 0 ? a.wgs : (cin8 ? 768 : 512), 1, s, a);
}

}  // namespace dffw
