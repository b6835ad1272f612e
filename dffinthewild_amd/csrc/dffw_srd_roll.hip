// The fused SRD blocks of the depth network: srd_roll (8 channels, described here), srd_roll16 and its pipelined form srd_pipe16 (16 channels) and
// srd_attention_mfma (the attention tail of the 32-channel block).  The alignment network's kernels on the same skeleton are dffw_align.hip.
//
// srd_roll: the whole SRD block of the 8-channel full-resolution stage (DEN.py:317-330 with resnet_block_2d :295-304,
// `FM_measure.Focus_extraction.2`) in ONE persistent kernel.
//
//     t    = relu(BN(conv1x3x3(x)))                       per slice          (Focus_Measure.conv.0)
//     feat = relu(x + BN(conv1x3x3(t)))                   per slice          (Focus_Measure.conv.2)
//     out  = feat + relu(conv1x1x1(relu(conv3x1x1(feat))))  across slices    (N_ch_attention.0 / .2, no BN, no bias)
//     pooled = maxpool(1,2,2)(out)                        (what the following EFD block reads, DEN.py:310)
//
// As three launches every stage is a full pass over the 8-channel volume bound by HBM: x is read twice, t and feat are
// written and read back (7 volume passes, 4.7 GB at batch 32).  Here a workgroup owns a column of 8 x 16 pixels of one
// sample and walks its slices; t and feat never leave LDS:
//   * x slices (12 x 20 footprint: two 3x3 halos) stream through a FIFO of LDS slots by LDS-DMA, several slices ahead
//     (counted vmcnt, raw s_barrier, as in conv_roll);
//   * stage A: conv.0 on the 10 x 18 region conv.2 needs -> t as hi/lo records in LDS (zero outside the image: it is
//     conv.2's padding);  stage B: conv.2 + x + ReLU on the 8 x 16 pixels -> feat in fp32 in a ring of 3 LDS slices;
//     both on the matrix cores with the two filters (2 x 3 chunks) resident in registers;
//   * stage C (two slices behind): the attention over feat[z-1], feat[z], feat[z+1] on the matrix cores as well (as 256
//     fp32 FMAs per pixel on the VALU it was the longest phase of a step): conv3x1x1 = 2 chunks over (pixel of the pair,
//     slice); its ReLU'd result, split to hi/lo in registers, IS the operand block of conv1x1x1 (K octet = the lane's own
//     4 channels hi | lo, filter rows [w_hi w_hi] and [w_lo 0]: two MFMAs, no data movement); + feat[z] (kept in fp32
//     registers by the lane that produced it), split to the storage format, stored; 2x2 max via DPP / permlane for the
//     pooled copy.
// HBM traffic: x once (halo from L2), out once, pooled once.  t and feat are rounded to hi+lo (the storage format) as
// operands, exactly as in the three-launch form.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "dffw_device.h"
#include "dffw_persist.h"
#include "dffw_srd_roll.h"

namespace dffw {

using SrdRow = KernelRow<SrdArgs>;   // dffw_persist.h

// ABL (development only, DFFW_SRD_ABL): timing ablations -- 1 no stage C, 2 no stage A, 4 no stage B, 8 no fill, 16 no barriers, 32 no global stores
template <int PREC, bool POOL, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void srd_roll_kernel(const SrdArgs a, const float *__restrict__ w3g, const float *__restrict__ w1g) {
    // (w3g / w1g = a.w3 / a.w1 as separate read-only parameters: only then does hipcc fetch the attention weights with
    // scalar loads; through the struct it used vector loads inside the loop, and beside LDS-DMA every use of a vector
    // load drains the whole DMA queue.  For the same reason the LDS stores below are inline asm: hipcc puts a
    // vmcnt(0) in front of every ordinary ds_write while an LDS-DMA is in flight.)
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
    constexpr int FPLANEB = TY * TX * PIXB;                        // one slice of feat as records (even pixels of a row first)
    constexpr int FSLOTB = PARTS * FPLANEB;
    constexpr int X_OFF = 0, T_OFF = RX * SLOTB, F_OFF = T_OFF + PARTS * TPLANEB;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[F_OFF + 3 * FSLOTB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    auto lds_store8 = [&](unsigned byte_off, uint32_t v0, uint32_t v1) {
        const u32x2 d = {v0, v1};
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds0 + byte_off), "v"(d) : "memory");
    };
    auto lds_store16 = [&](unsigned byte_off, f32x4 v) { asm volatile("ds_write_b128 %0, %1" ::"v"(lds0 + byte_off), "v"(v) : "memory"); };

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
    const int pb_res = ((pb_y + 2) * XX + (((pb_x + 2) & 1) ? XX / 2 : 0) + ((pb_x + 2) >> 1)) * PIXB + (g & 1) * 8;
    const int pb_f = (pb_y * TX + (g >> 1) * (TX / 2) + pb_pc) * PIXB;   // the lane's pixel inside a feat plane
    // attention filters as MFMA A-fragments (pack_conv): conv3x1x1 = 2 chunks, conv1x1x1 = [w_hi w_hi] and [w_lo 0]
    short8 w3f[2][PARTS], w1f[PARTS];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w3f[k][pt] = reinterpret_cast<const short8 *>(a.w3f)[(k * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int pt = 0; pt < PARTS; ++pt) w1f[pt] = reinterpret_cast<const short8 *>(a.w1f)[pt * 64 + lane];
    // the two filters as MFMA A-fragments (3 chunks each) and their BatchNorm shifts
    short8 w0[3][PARTS], w2[3][PARTS];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) {
            w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
            w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
        }
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
    f32x4 vq0 = f32x4{0.f, 0.f, 0.f, 0.f}, vq1 = vq0;
    typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
    u32x4v fop = {0u, 0u, 0u, 0u};
#ifdef DFFW_TRACE_BUILD
    StepTrace trc(a.trace, wave, lane, NWAVES);
#else
    StepTrace trc(nullptr, wave, lane, NWAVES);
#endif
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        const Unit U = decode(cu);
        // Step s of a column (s = 0 .. N): phase 1 = stage A of slice s (t = conv.0; waves 0-1 two operand tiles, waves 2-3 one); phase 2 = stage B
        // of slice s (feat[s] = conv.2 + x) and, on the same wave right behind it, stage C of slice s-1 (attention out of feat[s-2..s]).
        // A wave's stage B and stage C work on the same 32 pixels, so the feat ring (3 slices as hi/lo records) is wave-private: stage C follows
        // stage B without a barrier, one slice behind, and the column drains in ONE extra step that holds nothing but stage C of the last slice.
        // (Rounds 1-3 ran stage C two slices behind in phase 1, next to stage A: 2 + 1 operand tiles on the critical path of phase 1, one in
        // phase 2, N + 2 steps per column.)
        for (int s = 0; s <= a.N; ++s) {
            const bool produce = s < a.N;
            const unsigned fslot_off = F_OFF + (s % 3) * FSLOTB;
            trc.stamp(0);
            if (produce) {
                // (1) this step's x slice has landed (for every wave after the barrier)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(INFLIGHT) : "memory");
                if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            trc.stamp(1);
            if (s == 0) {   // feat[-1] = 0 (ring slot 2), the wave's own pixels
                lds_store8(F_OFF + 2 * FSLOTB + pb_f + (g & 1) * 8, 0u, 0u);
                if constexpr (PARTS == 2) lds_store8(F_OFF + 2 * FSLOTB + FPLANEB + pb_f + (g & 1) * 8, 0u, 0u);
            }
            // ---- stage A: t = relu(conv.0(x) + shift) on the 10 x 18 region, zero outside the image ---------------------
            if (produce && !(ABL & 2)) {
                auto store_t = [&](int j, const f32x4 acc) {
                    const int iy = U.gy0 - 1 + ta_y[j], ix = U.gx0 - 1 + ta_x[j];
                    const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                    if (ta_ok[j]) {
                        uint32_t h01, h23, l01, l23;
                        Fmt<PREC>::split2(relu_lim_bits(acc[0], inside ? 0x7f800000 : 0), relu_lim_bits(acc[1], inside ? 0x7f800000 : 0), h01, l01);
                        Fmt<PREC>::split2(relu_lim_bits(acc[2], inside ? 0x7f800000 : 0), relu_lim_bits(acc[3], inside ? 0x7f800000 : 0), h23, l23);
                        lds_store8(ta_st[j], h01, h23);
                        if constexpr (PARTS == 2) lds_store8(ta_st[j] + TPLANEB, l01, l23);
                    }
                };
                if (nA == 2) {
                    // two operand tiles: chunk k of the second one is requested as soon as chunk k of the first has been contracted (same registers), so its
                    // reads travel under the first tile's MFMAs and epilogue (DS operations retire in order: 2 chunks' reads behind the one waited for)
                    const unsigned ab0 = lds0 + X_OFF + xslot * SLOTB + pa[0], ab1 = lds0 + X_OFF + xslot * SLOTB + pa[1];
                    short8 ah[3], al[3];
#define DFFW_SRD_RDA(base, k)                                                                                                             \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ah[k]) : "v"(base), "n"(k * XX * PIXB));                                           \
    if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(al[k]) : "v"(base), "n"(k * XX * PIXB + PLANEB));
#define DFFW_SRD_MMA(k, W)                                 \
    if constexpr (PARTS == 2) {                            \
        acc = mma<F16>(w0[k][1], ah[k], acc);              \
        acc = mma<F16>(w0[k][0], al[k], acc);              \
    }                                                      \
    acc = mma<F16>(w0[k][0], ah[k], acc);
                    DFFW_SRD_RDA(ab0, 0)
                    DFFW_SRD_RDA(ab0, 1)
                    DFFW_SRD_RDA(ab0, 2)
                    f32x4 acc = b0;
                    if constexpr (PARTS == 2) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[0]), "+v"(al[0])); else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah[0]));
                    DFFW_SRD_MMA(0, w0)
                    DFFW_SRD_RDA(ab1, 0)
                    if constexpr (PARTS == 2) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[1]), "+v"(al[1])); else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah[1]));
                    DFFW_SRD_MMA(1, w0)
                    DFFW_SRD_RDA(ab1, 1)
                    if constexpr (PARTS == 2) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[2]), "+v"(al[2])); else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah[2]));
                    DFFW_SRD_MMA(2, w0)
                    DFFW_SRD_RDA(ab1, 2)
                    store_t(0, acc);
                    acc = b0;
                    // (behind the second tile's reads: at most its later chunks -- the first tile's stores come after them and only make the wait longer)
                    if constexpr (PARTS == 2) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[0]), "+v"(al[0])); else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah[0]));
                    DFFW_SRD_MMA(0, w0)
                    if constexpr (PARTS == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah[1]), "+v"(al[1])); else asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(ah[1]));
                    DFFW_SRD_MMA(1, w0)
                    if constexpr (PARTS == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[2]), "+v"(al[2])); else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[2]));
                    DFFW_SRD_MMA(2, w0)
#undef DFFW_SRD_RDA
#undef DFFW_SRD_MMA
                    store_t(1, acc);
                } else {
                    store_t(0, tile_mma(lds0 + X_OFF + xslot * SLOTB + pa[0], std::integral_constant<int, XX * PIXB>{}, std::integral_constant<int, PLANEB>{}, w0, b0));
                }
            }
            trc.stamp(2);
            if (produce) {
                // (2) t complete
                if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                trc.stamp(3);
                // ---- stage B: feat[s] = relu(conv.2(t) + shift + x) ----------------------------------------------------
                if constexpr (!(ABL & 4)) {
                    const f32x4 acc = tile_mma(lds0 + T_OFF + pbo, std::integral_constant<int, TXT * PIXB>{}, std::integral_constant<int, TPLANEB>{}, w2, b2);
                    const unsigned xp = lds0 + X_OFF + xslot * SLOTB + pb_res;
                    u32x2 xh, xl = {0u, 0u};
                    asm volatile("ds_read_b64 %0, %1" : "=v"(xh) : "v"(xp));
                    if constexpr (PARTS == 2) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(xl) : "v"(xp), "n"(PLANEB));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh), "+v"(xl));
                    float r0, r1, r2, r3;
                    Fmt<PREC>::join2(xh[0], xl[0], r0, r1);
                    Fmt<PREC>::join2(xh[1], xl[1], r2, r3);
                    f32x4 v;
                    v[0] = relu_bits(acc[0] + r0);
                    v[1] = relu_bits(acc[1] + r1);
                    v[2] = relu_bits(acc[2] + r2);
                    v[3] = relu_bits(acc[3] + r3);
                    uint32_t fh01, fh23, fl01, fl23;
                    Fmt<PREC>::split2(v[0], v[1], fh01, fl01);
                    Fmt<PREC>::split2(v[2], v[3], fh23, fl23);
                    lds_store8(fslot_off + pb_f + (g & 1) * 8, fh01, fh23);
                    if constexpr (PARTS == 2) lds_store8(fslot_off + FPLANEB + pb_f + (g & 1) * 8, fl01, fl23);
                    fop = u32x4v{fh01, fh23, fl01, fl23};   // feat[s] of the lane's own 4 channels as [hi x4 | lo x4]: stage C's K octet for the slice behind z
                    vq1 = vq0;   // fp32 feat of this lane's pixel / channels, two steps deep: stage C adds it back
                    vq0 = v;
                }
            } else {
                vq1 = vq0;
                fop = u32x4v{0u, 0u, 0u, 0u};   // feat[N] = 0
            }
            trc.stamp(4);
            // ---- stage C: attention for slice z = s-1 out of feat[z-1], feat[z], feat[z+1] = the slice stage B just wrote (or the zeros behind the
            // last one); wave w = pairs of rows 2w, 2w+1 = the pixels ITS stage B produced: feat never crosses waves, no barrier in between ----
            if (s >= 1 && !(ABL & 1)) {
                const int z = s - 1;
                const unsigned sm = F_OFF + ((z + 2) % 3) * FSLOTB, sc = F_OFF + (z % 3) * FSLOTB;
                // chunk 0: K octet g = (pixel g >> 1 of the pair, slice z-1 + (g & 1)) out of the ring; chunk 1: K octet g = the lane's own 4 channels of
                // feat[z+1] as [hi x4 | lo x4], straight from stage B's registers (filter fragments [w_hi w_hi] and [w_lo 0] as for the 1x1x1 conv: two MFMAs)
                const unsigned ad0 = lds0 + ((g & 1) ? sc : sm) + pb_f;
                short8 fh0, fl0;
                asm volatile("ds_read_b128 %0, %1" : "=v"(fh0) : "v"(ad0));
                if constexpr (PARTS == 2) {
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fl0) : "v"(ad0), "n"(FPLANEB));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh0), "+v"(fl0));
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh0));
                }
                const short8 f1op = __builtin_bit_cast(short8, fop);
                f32x4 at = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (PARTS == 2) {
                    at = mma<F16>(w3f[1][1], f1op, at);
                    at = mma<F16>(w3f[0][1], fh0, at);
                    at = mma<F16>(w3f[0][0], fl0, at);
                }
                at = mma<F16>(w3f[1][0], f1op, at);
                at = mma<F16>(w3f[0][0], fh0, at);
                // ReLU, split: {hi of the lane's 4 channels | lo of them} is the lane's K octet of the 1x1x1 conv
                uint32_t ah01, ah23, al01, al23;
                Fmt<PREC>::split2(relu_bits(at[0]), relu_bits(at[1]), ah01, al01);
                Fmt<PREC>::split2(relu_bits(at[2]), relu_bits(at[3]), ah23, al23);
                const u32x4v bq = {ah01, ah23, al01, al23};
                const short8 b2op = __builtin_bit_cast(short8, bq);
                f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (PARTS == 2) o = mma<F16>(w1f[1], b2op, o);
                o = mma<F16>(w1f[0], b2op, o);
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = vq1[i] + relu_bits(o[i]);
                uint32_t h01, h23, l01, l23;
                Fmt<PREC>::split2(v[0], v[1], h01, l01);
                Fmt<PREC>::split2(v[2], v[3], h23, l23);
                const int64_t pix = (((int64_t)U.b * a.N + z) * a.H + U.gy0 + pb_y) * a.W + U.gx0 + pb_x;
                if constexpr (POOL) {   // max over the 2x2 block of the values as stored: other pixel of the pair = lane rows g ^ 2, other row = column r ^ 8
                    float m[4];
                    Fmt<PREC>::join2(h01, l01, m[0], m[1]);
                    Fmt<PREC>::join2(h23, l23, m[2], m[3]);
                    uint32_t ph01, ph23, pl01, pl23;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {   // the values are sums of two ReLU results: non-negative, so the maxima are taken on the bit patterns (no canonicalising v_max_f32)
                        uint32_t mu = __float_as_uint(m[i]);
                        const auto sw = __builtin_amdgcn_permlane32_swap(mu, mu, false, false);
                        mu = max(mu, lane < 32 ? sw[1] : sw[0]);
                        mu = max(mu, (uint32_t)__builtin_amdgcn_mov_dpp((int)mu, 0x128, 0xF, 0xF, true));   // row_ror:8
                        m[i] = __uint_as_float(mu);
                    }
                    Fmt<PREC>::split2(m[0], m[1], ph01, pl01);
                    Fmt<PREC>::split2(m[2], m[3], ph23, pl23);
                    if constexpr (PARTS == 2) {
                        swap16(ph01, pl01);
                        swap16(ph23, pl23);
                    }
                    if (g < 2 && r < 8 && !(ABL & 32)) {
                        const int64_t pp = (((int64_t)U.b * a.N + z) * (a.H / 2) + (U.gy0 / 2 + wave)) * (a.W / 2) + U.gx0 / 2 + pb_pc;
                        if constexpr (PARTS == 2) *reinterpret_cast<uint4 *>(a.pooled + pp * rec + (g & 1) * C) = make_uint4(ph01, ph23, pl01, pl23);
                        else *reinterpret_cast<uint2 *>(a.pooled + pp * rec + (g & 1) * 4) = make_uint2(ph01, ph23);
                    }
                }
                if constexpr (PARTS == 2) {
                    swap16(h01, l01);
                    swap16(h23, l23);
                    if ((ABL & 32) == 0 || h01 == 0x12345u) *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C) = make_uint4(h01, h23, l01, l23);
                } else {
                    *reinterpret_cast<uint2 *>(a.out + pix * rec + (g & 1) * 4) = make_uint2(h01, h23);
                }
            }
            trc.stamp(5);
            if (produce) {
                // (3) everyone's reads of x and t are done: the x slot is free, queue the slice RX-1 ahead into it
                if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                trc.stamp(6);
                if constexpr (!(ABL & 8)) issue_next();
                xslot = (xslot + 1 == RX) ? 0 : xslot + 1;
            }
            trc.next();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no LDS-DMA may outlive the wave
}

// ---- srd_roll16: the same block for the 16-channel half-resolution stage (`FM_conv1.1`) -----------------------------------
// 16 output channels fill the MFMA result rows, so no pixel pairs: a GEMM column is one pixel, the 1x3x3 convs contract over
// 5 chunks of (2 taps x 16 channels) (tap 9 = zeros), records are 32 bytes per plane (natural column order).  Columns are
// 4 x 16 pixels (LDS: 4 x-slices of 8 x 20 pixels + t + the feat ring = 67 KB, two workgroups per CU).  Stage B / C tiles
// are 2 rows x 8 pixels per wave so that the 2x2 max-pool stays inside a wave.  Streaming skeleton, counted waits, inline-asm
// LDS access and the MFMA attention (its split result = the 1x1x1 conv's operand in place) as in srd_roll_kernel.
// ABL (development only, DFFW_SRD_ABL): timing ablations -- 1 no stage C, 2 no stage A, 4 no stage B, 8 no fill, 16 no barriers, 32 no global stores
template <int PREC, bool POOL, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void srd_roll16_kernel(const SrdArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int C = 16, TY = 4, TX = 16, NWAVES = 4;
    constexpr int XY = TY + 4, XX = TX + 4, XPIX = XY * XX;
    constexpr int TYT = TY + 2, TXT = TX + 2, TPIX = TYT * TXT;
    // t rows at a pitch of 24 pixels = 768 bytes: a stage-B tile is 2 rows x 8 pixels, and the 16 lanes of a ds_read_b128 row group only cover 16 distinct
    // 16-byte bank groups when its two rows are a multiple of 256 bytes apart (18-pixel rows, 576 bytes: two-way conflicts on every stage-B read)
    constexpr int TXTP = 24;
    constexpr int PIXB = C * 2;
    constexpr int NPIECE = 6;                                      // 1 KiB wave instructions per plane (5 hold the 160 pixels; 6 keeps 3 per wave)
    static_assert(NPIECE * 32 >= XPIX, "plane holds the footprint");
    constexpr int PLANEB = NPIECE * 1024;
    constexpr int SLOTB = PARTS * PLANEB;
    constexpr int RX = 4;
    constexpr int NP = PARTS * NPIECE, PPW = (NP + NWAVES - 1) / NWAVES;
    static_assert(NP % PPW == 0, "every wave issues PPW pieces or none (counted vmcnt waits)");
    constexpr int TPLANEB = TYT * TXTP * PIXB;
    constexpr int FPLANEB = TY * TX * PIXB;
    constexpr int FSLOTB = PARTS * FPLANEB;
    constexpr int X_OFF = 0, T_OFF = RX * SLOTB, F_OFF = T_OFF + PARTS * TPLANEB;
    constexpr int NCH = 5;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[F_OFF + 3 * FSLOTB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    auto lds_store8 = [&](unsigned byte_off, uint32_t v0, uint32_t v1) {
        const u32x2 d = {v0, v1};
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds0 + byte_off), "v"(d) : "memory");
    };
    auto lds_store16 = [&](unsigned byte_off, f32x4 v) { asm volatile("ds_write_b128 %0, %1" ::"v"(lds0 + byte_off), "v"(v) : "memory"); };

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
            const int ci = i * 64 + lane, pix = ci >> 1, oct = ci & 1;
            const int fy = pix / XX, fx = pix - fy * XX;
            const int iy = c.gy0 - 2 + fy, ix = c.gx0 - 2 + fx;
            fok[k] = p < NP && pix < XPIX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            fsrc[k] = a.x + (int64_t)c.b * a.N * slice_elems + (int64_t)(iy * a.W + ix) * rec + part * C + oct * 8;
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

    // stage A: the 6 x 18 t pixels are 7 operand tiles: tiles 0-5 = the first 16 pixels of row 0-5 (16 consecutive pixels of ONE row: conflict-free
    // operand reads; tiles of 16 consecutive indices of the 6 x 18 region wrapped rows and collided two ways), tile 6 = the two remaining pixels of
    // each row (12 of its 16 lanes busy); waves 0-2 take two tiles, wave 3 one
    constexpr int TA = 2;
    const int nA = wave < 3 ? 2 : 1;
    int pa[TA], ta_y[TA], ta_x[TA], ta_st[TA];
    bool ta_ok[TA];
#pragma unroll
    for (int j = 0; j < TA; ++j) {
        const int tile = j == 0 ? wave : 4 + wave;
        ta_ok[j] = tile < TYT || r < 2 * TYT;
        ta_y[j] = tile < TYT ? tile : (r < 2 * TYT ? r >> 1 : TYT - 1);
        ta_x[j] = tile < TYT ? r : TX + (r & 1);
        pa[j] = (ta_y[j] * XX + ta_x[j]) * PIXB + (g & 1) * 16;
        ta_st[j] = T_OFF + (ta_y[j] * TXTP + ta_x[j]) * PIXB + g * 8;
    }
    // K octet g of chunk k = (filter tap 2k + (g >> 1), channel octet g & 1); tap 9 carries zero weights
    int tapA[NCH], tapB[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int tap = 2 * k + (g >> 1);
        const int dy = tap < 9 ? tap / 3 : 0, dx = tap < 9 ? tap % 3 : 0;
        tapA[k] = (dy * XX + dx) * PIXB;
        tapB[k] = (dy * TXTP + dx) * PIXB;
    }
    // stage B / C: wave w = rows 2*(w >> 1), +1 x columns 8*(w & 1) .. +7 (the 2x2 pooling blocks stay inside the wave)
    const int pb_y = 2 * (wave >> 1) + (r >> 3), pb_x = 8 * (wave & 1) + (r & 7);
    const int pbo = (pb_y * TXTP + pb_x) * PIXB + (g & 1) * 16;
    const int pb_res = ((pb_y + 2) * XX + pb_x + 2) * PIXB + g * 8;
    const int pb_f = (pb_y * TX + pb_x) * PIXB;
    short8 w0[NCH][PARTS], w2[NCH][PARTS], w3f[2][PARTS], w1f[PARTS];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) {
            w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
            w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
        }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w3f[k][pt] = reinterpret_cast<const short8 *>(a.w3f)[(k * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int pt = 0; pt < PARTS; ++pt) w1f[pt] = reinterpret_cast<const short8 *>(a.w1f)[pt * 64 + lane];
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(a.b0 + g * 4);
    const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + g * 4);
    auto tile_mma = [&](unsigned base, const int (&tapo)[NCH], auto loB_c, const short8 (&wf)[NCH][PARTS], f32x4 acc) {
        constexpr int loB = decltype(loB_c)::value;   // the lo plane as an immediate of the read
        short8 xh[NCH], xl[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const unsigned ad = base + tapo[k];
            asm volatile("ds_read_b128 %0, %1" : "=v"(xh[k]) : "v"(ad));
            if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k]) : "v"(ad), "n"(loB));
            else xl[k] = short8{0, 0, 0, 0, 0, 0, 0, 0};   /* (single-part storage: never contracted; NOT a copy of the in-flight hi fragment, tools/isa_wait_lint.py) */
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int left = (NCH - 1 - k) * PARTS;   // reads still allowed in flight (compile-time after unrolling)
            if (left == 8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 6) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(xh[k]), "+v"(xl[k]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh[k]), "+v"(xl[k]));
            if constexpr (PARTS == 2) {
                acc = mma<F16>(wf[k][1], xh[k], acc);
                acc = mma<F16>(wf[k][0], xl[k], acc);
            }
            acc = mma<F16>(wf[k][0], xh[k], acc);
        }
        return acc;
    };

    // two operand tiles side by side (stage A of the waves that own two): the reads of both run three chunks ahead of the MFMAs and the two
    // accumulator chains alternate, so one tile's LDS latency and MFMA dependency gaps are covered by the other's work
    auto tile_mma2 = [&](unsigned base0, unsigned base1, const int (&tapo)[NCH], auto loB_c, const short8 (&wf)[NCH][PARTS], f32x4 &acc0, f32x4 &acc1) {
        static_assert(PARTS == 2 || PARTS == 1, "");
        constexpr int NBUF = 3;
        short8 xh[NBUF][2], xl[NBUF][2];
        auto fetch = [&](int k) {
            const unsigned a0 = base0 + tapo[k], a1 = base1 + tapo[k];
            asm volatile("ds_read_b128 %0, %1" : "=v"(xh[k % NBUF][0]) : "v"(a0));
            if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k % NBUF][0]) : "v"(a0), "n"(decltype(loB_c)::value));
            asm volatile("ds_read_b128 %0, %1" : "=v"(xh[k % NBUF][1]) : "v"(a1));
            if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k % NBUF][1]) : "v"(a1), "n"(decltype(loB_c)::value));
        };
        fetch(0);
        fetch(1);
        fetch(2);
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int left = (NCH - 1 - k < 2 ? NCH - 1 - k : 2) * 2 * PARTS;   // reads of later chunks that may still be in flight
            auto &h0 = xh[k % NBUF][0], &h1 = xh[k % NBUF][1], &l0 = xl[k % NBUF][0], &l1 = xl[k % NBUF][1];
            if (left == 8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            else if (left == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            else if (left == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            if constexpr (PARTS == 1) {
                l0 = h0;
                l1 = h1;
            }
            if constexpr (PARTS == 2) {
                acc0 = mma<F16>(wf[k][1], h0, acc0);
                acc1 = mma<F16>(wf[k][1], h1, acc1);
                acc0 = mma<F16>(wf[k][0], l0, acc0);
                acc1 = mma<F16>(wf[k][0], l1, acc1);
            }
            acc0 = mma<F16>(wf[k][0], h0, acc0);
            acc1 = mma<F16>(wf[k][0], h1, acc1);
            __builtin_amdgcn_sched_barrier(0);
            if (k + 3 < NCH) fetch(k + 3);
        }
    };

    constexpr int INFLIGHT = (RX - 2) * PPW;
#pragma unroll
    for (int q = 0; q < RX - 1; ++q) issue_next();
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("s_barrier" ::: "memory");

    int xslot = 0;
    f32x4 vq0 = f32x4{0.f, 0.f, 0.f, 0.f}, vq1 = vq0;
    typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
    u32x4v fop = {0u, 0u, 0u, 0u};
    for (int cu = ufirst; cu < uend; cu += wgs_per_xcd) {
        const Unit U = decode(cu);
        // a step as in srd_roll_kernel: stage A | barrier | stage B of slice s, then stage C of slice s-1 on the same wave (its own pixels: the feat
        // ring is wave-private); N + 1 steps per column, the last one holds only stage C of the last slice
        for (int s = 0; s <= a.N; ++s) {
            const bool produce = s < a.N;
            const unsigned fslot_off = F_OFF + (s % 3) * FSLOTB;
            if (produce) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(INFLIGHT) : "memory");
                if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            if (s == 0) {   // feat[-1] = 0 (ring slot 2), the wave's own pixels
                lds_store8(F_OFF + 2 * FSLOTB + pb_f + g * 8, 0u, 0u);
                if constexpr (PARTS == 2) lds_store8(F_OFF + 2 * FSLOTB + FPLANEB + pb_f + g * 8, 0u, 0u);
            }
            // ---- stage A ---------------------------------------------------------------------------------------------------------
            if (produce && !(ABL & 2)) {
                f32x4 accA[TA];
                if (nA == 2) {
                    accA[0] = b0;
                    accA[1] = b0;
                    tile_mma2(lds0 + X_OFF + xslot * SLOTB + pa[0], lds0 + X_OFF + xslot * SLOTB + pa[1], tapA, std::integral_constant<int, PLANEB>{}, w0, accA[0], accA[1]);
                } else {
                    accA[0] = tile_mma(lds0 + X_OFF + xslot * SLOTB + pa[0], tapA, std::integral_constant<int, PLANEB>{}, w0, b0);
                    accA[1] = b0;
                }
#pragma unroll
                for (int j = 0; j < TA; ++j) {
                    if (j >= nA) break;
                    const f32x4 acc = accA[j];
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
            }
            if (produce) {
                if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                // ---- stage B ---------------------------------------------------------------------------------------------------------
                if constexpr (!(ABL & 4)) {
                    const f32x4 acc = tile_mma(lds0 + T_OFF + pbo, tapB, std::integral_constant<int, TPLANEB>{}, w2, b2);
                    const unsigned xp = lds0 + X_OFF + xslot * SLOTB + pb_res;
                    u32x2 xh, xl = {0u, 0u};
                    asm volatile("ds_read_b64 %0, %1" : "=v"(xh) : "v"(xp));
                    if constexpr (PARTS == 2) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(xl) : "v"(xp), "n"(PLANEB));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh), "+v"(xl));
                    float r0, r1, r2, r3;
                    Fmt<PREC>::join2(xh[0], xl[0], r0, r1);
                    Fmt<PREC>::join2(xh[1], xl[1], r2, r3);
                    f32x4 v;
                    v[0] = relu_bits(acc[0] + r0);
                    v[1] = relu_bits(acc[1] + r1);
                    v[2] = relu_bits(acc[2] + r2);
                    v[3] = relu_bits(acc[3] + r3);
                    uint32_t fh01, fh23, fl01, fl23;
                    Fmt<PREC>::split2(v[0], v[1], fh01, fl01);
                    Fmt<PREC>::split2(v[2], v[3], fh23, fl23);
                    lds_store8(fslot_off + pb_f + g * 8, fh01, fh23);
                    if constexpr (PARTS == 2) lds_store8(fslot_off + FPLANEB + pb_f + g * 8, fl01, fl23);
                    fop = u32x4v{fh01, fh23, fl01, fl23};   // feat[s], channels 4g..4g+3 as [hi x4 | lo x4]: stage C's K octet for the slice behind z
                    vq1 = vq0;
                    vq0 = v;
                }
            } else {
                vq1 = vq0;
                fop = u32x4v{0u, 0u, 0u, 0u};   // feat[N] = 0
            }
            // ---- stage C: attention for slice z = s-1 (feat[z+1] = what stage B just wrote, or the zeros behind the last slice) ----------------------------------------------------------------------
            if (s >= 1 && !(ABL & 1)) {
                const int z = s - 1;
                const unsigned sm = F_OFF + ((z + 2) % 3) * FSLOTB, sc = F_OFF + (z % 3) * FSLOTB;
                // chunk 0: K octet g = (slice z-1 + (g >> 1), channel octet g & 1) out of the ring; chunk 1: K octet g = channels 4g..4g+3 of feat[z+1] as
                // [hi x4 | lo x4], straight from stage B's registers (fragments [w_hi w_hi] and [w_lo 0]: two MFMAs)
                const unsigned ad0 = lds0 + ((g >> 1) ? sc : sm) + pb_f + (g & 1) * 16;
                short8 fh0, fl0;
                asm volatile("ds_read_b128 %0, %1" : "=v"(fh0) : "v"(ad0));
                if constexpr (PARTS == 2) {
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fl0) : "v"(ad0), "n"(FPLANEB));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh0), "+v"(fl0));
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh0));
                }
                const short8 f1op = __builtin_bit_cast(short8, fop);
                f32x4 at = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (PARTS == 2) {
                    at = mma<F16>(w3f[1][1], f1op, at);
                    at = mma<F16>(w3f[0][1], fh0, at);
                    at = mma<F16>(w3f[0][0], fl0, at);
                }
                at = mma<F16>(w3f[1][0], f1op, at);
                at = mma<F16>(w3f[0][0], fh0, at);
                uint32_t ah01, ah23, al01, al23;
                Fmt<PREC>::split2(relu_bits(at[0]), relu_bits(at[1]), ah01, al01);
                Fmt<PREC>::split2(relu_bits(at[2]), relu_bits(at[3]), ah23, al23);
                const u32x4v bq = {ah01, ah23, al01, al23};
                const short8 b2op = __builtin_bit_cast(short8, bq);
                f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (PARTS == 2) o = mma<F16>(w1f[1], b2op, o);
                o = mma<F16>(w1f[0], b2op, o);
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = vq1[i] + relu_bits(o[i]);
                uint32_t h01, h23, l01, l23;
                Fmt<PREC>::split2(v[0], v[1], h01, l01);
                Fmt<PREC>::split2(v[2], v[3], h23, l23);
                const int64_t pix = (((int64_t)U.b * a.N + z) * a.H + U.gy0 + pb_y) * a.W + U.gx0 + pb_x;
                if constexpr (POOL) {   // 2x2 block: column neighbour = lane r ^ 1, row neighbour = lane r ^ 8
                    float m[4];
                    Fmt<PREC>::join2(h01, l01, m[0], m[1]);
                    Fmt<PREC>::join2(h23, l23, m[2], m[3]);
                    uint32_t ph01, ph23, pl01, pl23;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {   // non-negative values (sums of two ReLU results): maxima on the bit patterns
                        uint32_t mu = __float_as_uint(m[i]);
                        mu = max(mu, (uint32_t)__builtin_amdgcn_mov_dpp((int)mu, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
                        mu = max(mu, (uint32_t)__builtin_amdgcn_mov_dpp((int)mu, 0x128, 0xF, 0xF, true));   // row_ror:8
                        m[i] = __uint_as_float(mu);
                    }
                    Fmt<PREC>::split2(m[0], m[1], ph01, pl01);
                    Fmt<PREC>::split2(m[2], m[3], ph23, pl23);
                    if constexpr (PARTS == 2) {
                        swap16(ph01, pl01);
                        swap16(ph23, pl23);
                    }
                    if ((r & 9) == 0 && !(ABL & 32)) {
                        const int64_t pp = (((int64_t)U.b * a.N + z) * (a.H / 2) + (U.gy0 / 2 + (wave >> 1))) * (a.W / 2) + U.gx0 / 2 + 4 * (wave & 1) + ((r & 7) >> 1);
                        if constexpr (PARTS == 2) *reinterpret_cast<uint4 *>(a.pooled + pp * rec + (g & 1) * C + (g >> 1) * 8) = make_uint4(ph01, ph23, pl01, pl23);
                        else *reinterpret_cast<uint2 *>(a.pooled + pp * rec + g * 4) = make_uint2(ph01, ph23);
                    }
                }
                if constexpr (PARTS == 2) {
                    swap16(h01, l01);
                    swap16(h23, l23);
                    if ((ABL & 32) == 0 || h01 == 0x12345u) *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C + (g >> 1) * 8) = make_uint4(h01, h23, l01, l23);
                } else {
                    *reinterpret_cast<uint2 *>(a.out + pix * rec + g * 4) = make_uint2(h01, h23);
                }
            }
            if (produce) {
                if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if constexpr (!(ABL & 8)) issue_next();
                xslot = (xslot + 1 == RX) ? 0 : xslot + 1;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- srd_pipe16 (round 6): srd_roll16's block as a software pipeline over the workgroup's slice stream -----------------------------------------
// srd_roll16 walks a column slice by slice as  barrier | stage A | barrier | stage B, stage C | barrier | fill : three barriers and three dependent
// stage chains per step that add up (profiles/r04_ablation_srd_roll.txt: no A -36 %, no B -25 %, no C -24 %, no barriers only -8 %), plus one drain step
// per column.  Here the stages of ONE step belong to three consecutive stream positions -- stage A of position p (t into one of TWO t buffers), stage B
// of position p - 1 (its residual pixels of x were read into registers a step earlier, so x[p - 1]'s slot is free), stage C of position p - 2 -- so
// nothing a wave does inside a step depends on what another wave does in the same step: ONE barrier per step (t[p - 1] complete, x[p] landed, the
// slot of x[p - 1] and the buffer t[p] free), the three chains are independent work for the scheduler and the SIMD's other wave, and the stream runs
// on across columns (positions carry their own column / slice; the attention's zero slices at a column's ends are a zeroed ring slot / a zero operand),
// so a column costs N steps, not N + 1.  Same arithmetic in the same order as srd_roll16: bit-identical results (tested).
// 16 output channels fill the MFMA result rows, so no pixel pairs: a GEMM column is one pixel, the 1x3x3 convs contract over
// 5 chunks of (2 taps x 16 channels) (tap 9 = zeros), records are 32 bytes per plane (natural column order).  Columns are
// 4 x 16 pixels (LDS: 4 x-slices of 8 x 20 pixels + t + the feat ring = 67 KB, two workgroups per CU).  Stage B / C tiles
// are 2 rows x 8 pixels per wave so that the 2x2 max-pool stays inside a wave.  Streaming skeleton, counted waits, inline-asm
// LDS access and the MFMA attention (its split result = the 1x1x1 conv's operand in place) as in srd_roll_kernel.
// ABL (development only, DFFW_SRD_ABL): timing ablations -- 1 no stage C, 2 no stage A, 4 no stage B, 8 no fill, 16 no barriers, 32 no global stores
template <int PREC, bool POOL, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void srd_pipe16_kernel(const SrdArgs a) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int C = 16, TY = 4, TX = 16, NWAVES = 4;
    constexpr int XY = TY + 4, XX = TX + 4, XPIX = XY * XX;
    constexpr int TYT = TY + 2, TXT = TX + 2, TPIX = TYT * TXT;
    // t rows at a pitch of 24 pixels = 768 bytes: a stage-B tile is 2 rows x 8 pixels, and the 16 lanes of a ds_read_b128 row group only cover 16 distinct
    // 16-byte bank groups when its two rows are a multiple of 256 bytes apart (18-pixel rows, 576 bytes: two-way conflicts on every stage-B read)
    constexpr int TXTP = 24;
    constexpr int PIXB = C * 2;
    constexpr int NPIECE = 6;                                      // 1 KiB wave instructions per plane (5 hold the 160 pixels; 6 keeps 3 per wave)
    static_assert(NPIECE * 32 >= XPIX, "plane holds the footprint");
    constexpr int PLANEB = NPIECE * 1024;
    constexpr int SLOTB = PARTS * PLANEB;
    constexpr int RX = 4;
    constexpr int NP = PARTS * NPIECE, PPW = (NP + NWAVES - 1) / NWAVES;
    static_assert(NP % PPW == 0, "every wave issues PPW pieces or none (counted vmcnt waits)");
    constexpr int TPLANEB = TYT * TXTP * PIXB;
    constexpr int FPLANEB = TY * TX * PIXB;
    constexpr int FSLOTB = PARTS * FPLANEB;
    constexpr int X_OFF = 0, T_OFF = RX * SLOTB, TBUFB = PARTS * TPLANEB, F_OFF = T_OFF + 2 * TBUFB;   // two t buffers (positions of either parity)
    constexpr int NCH = 5;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[F_OFF + 3 * FSLOTB];
    static_assert(2 * (F_OFF + 3 * FSLOTB) <= 160 * 1024, "two workgroups per CU");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    auto lds_store8 = [&](unsigned byte_off, uint32_t v0, uint32_t v1) {
        const u32x2 d = {v0, v1};
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds0 + byte_off), "v"(d) : "memory");
    };
    auto lds_store16 = [&](unsigned byte_off, f32x4 v) { asm volatile("ds_write_b128 %0, %1" ::"v"(lds0 + byte_off), "v"(v) : "memory"); };

    // (inline copy of persistent_range(), dffw_persist.h: through the helper hipcc allocates this kernel's registers differently)
    const int xcd = blockIdx.x & 7, widx = blockIdx.x >> 3, wgs_per_xcd = gridDim.x >> 3;
    int ufirst, uend;
    {
        const int q = a.total_tiles >> 3, rem = a.total_tiles & 7;
        const int xs = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
        uend = xs + q + (xcd < rem ? 1 : 0);
        ufirst = xs + widx;
    }
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
            const int ci = i * 64 + lane, pix = ci >> 1, oct = ci & 1;
            const int fy = pix / XX, fx = pix - fy * XX;
            const int iy = c.gy0 - 2 + fy, ix = c.gx0 - 2 + fx;
            fok[k] = p < NP && pix < XPIX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            fsrc[k] = a.x + (int64_t)c.b * a.N * slice_elems + (int64_t)(iy * a.W + ix) * rec + part * C + oct * 8;
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

    // stage A: the 6 x 18 t pixels are 7 operand tiles: tiles 0-5 = the first 16 pixels of row 0-5 (16 consecutive pixels of ONE row: conflict-free
    // operand reads; tiles of 16 consecutive indices of the 6 x 18 region wrapped rows and collided two ways), tile 6 = the two remaining pixels of
    // each row (12 of its 16 lanes busy); waves 0-2 take two tiles, wave 3 one
    constexpr int TA = 2;
    const int nA = wave < 3 ? 2 : 1;
    int pa[TA], ta_y[TA], ta_x[TA], ta_st[TA];
    bool ta_ok[TA];
#pragma unroll
    for (int j = 0; j < TA; ++j) {
        const int tile = j == 0 ? wave : 4 + wave;
        ta_ok[j] = tile < TYT || r < 2 * TYT;
        ta_y[j] = tile < TYT ? tile : (r < 2 * TYT ? r >> 1 : TYT - 1);
        ta_x[j] = tile < TYT ? r : TX + (r & 1);
        pa[j] = (ta_y[j] * XX + ta_x[j]) * PIXB + (g & 1) * 16;
        ta_st[j] = T_OFF + (ta_y[j] * TXTP + ta_x[j]) * PIXB + g * 8;
    }
    // K octet g of chunk k = (filter tap 2k + (g >> 1), channel octet g & 1); tap 9 carries zero weights
    int tapA[NCH], tapB[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int tap = 2 * k + (g >> 1);
        const int dy = tap < 9 ? tap / 3 : 0, dx = tap < 9 ? tap % 3 : 0;
        tapA[k] = (dy * XX + dx) * PIXB;
        tapB[k] = (dy * TXTP + dx) * PIXB;
    }
    // stage B / C: wave w = rows 2*(w >> 1), +1 x columns 8*(w & 1) .. +7 (the 2x2 pooling blocks stay inside the wave)
    const int pb_y = 2 * (wave >> 1) + (r >> 3), pb_x = 8 * (wave & 1) + (r & 7);
    const int pbo = (pb_y * TXTP + pb_x) * PIXB + (g & 1) * 16;
    const int pb_res = ((pb_y + 2) * XX + pb_x + 2) * PIXB + g * 8;
    const int pb_f = (pb_y * TX + pb_x) * PIXB;
    short8 w0[NCH][PARTS], w2[NCH][PARTS], w3f[2][PARTS], w1f[PARTS];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) {
            w0[k][pt] = reinterpret_cast<const short8 *>(a.w0)[(k * PARTS + pt) * 64 + lane];
            w2[k][pt] = reinterpret_cast<const short8 *>(a.w2)[(k * PARTS + pt) * 64 + lane];
        }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) w3f[k][pt] = reinterpret_cast<const short8 *>(a.w3f)[(k * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int pt = 0; pt < PARTS; ++pt) w1f[pt] = reinterpret_cast<const short8 *>(a.w1f)[pt * 64 + lane];
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(a.b0 + g * 4);
    const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + g * 4);
    auto tile_mma = [&](unsigned base, const int (&tapo)[NCH], auto loB_c, const short8 (&wf)[NCH][PARTS], f32x4 acc) {
        constexpr int loB = decltype(loB_c)::value;   // the lo plane as an immediate of the read
        short8 xh[NCH], xl[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const unsigned ad = base + tapo[k];
            asm volatile("ds_read_b128 %0, %1" : "=v"(xh[k]) : "v"(ad));
            if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k]) : "v"(ad), "n"(loB));
            else xl[k] = short8{0, 0, 0, 0, 0, 0, 0, 0};   /* (single-part storage: never contracted; NOT a copy of the in-flight hi fragment, tools/isa_wait_lint.py) */
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int left = (NCH - 1 - k) * PARTS;   // reads still allowed in flight (compile-time after unrolling)
            if (left == 8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 6) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(xh[k]), "+v"(xl[k]));
            else if (left == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(xh[k]), "+v"(xl[k]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh[k]), "+v"(xl[k]));
            if constexpr (PARTS == 2) {
                acc = mma<F16>(wf[k][1], xh[k], acc);
                acc = mma<F16>(wf[k][0], xl[k], acc);
            }
            acc = mma<F16>(wf[k][0], xh[k], acc);
        }
        return acc;
    };

    // two operand tiles side by side (stage A of the waves that own two): the reads of both run three chunks ahead of the MFMAs and the two
    // accumulator chains alternate, so one tile's LDS latency and MFMA dependency gaps are covered by the other's work
    auto tile_mma2 = [&](unsigned base0, unsigned base1, const int (&tapo)[NCH], auto loB_c, const short8 (&wf)[NCH][PARTS], f32x4 &acc0, f32x4 &acc1) {
        static_assert(PARTS == 2 || PARTS == 1, "");
        constexpr int NBUF = 3;
        short8 xh[NBUF][2], xl[NBUF][2];
        auto fetch = [&](int k) {
            const unsigned a0 = base0 + tapo[k], a1 = base1 + tapo[k];
            asm volatile("ds_read_b128 %0, %1" : "=v"(xh[k % NBUF][0]) : "v"(a0));
            if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k % NBUF][0]) : "v"(a0), "n"(decltype(loB_c)::value));
            asm volatile("ds_read_b128 %0, %1" : "=v"(xh[k % NBUF][1]) : "v"(a1));
            if constexpr (PARTS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xl[k % NBUF][1]) : "v"(a1), "n"(decltype(loB_c)::value));
        };
        fetch(0);
        fetch(1);
        fetch(2);
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int left = (NCH - 1 - k < 2 ? NCH - 1 - k : 2) * 2 * PARTS;   // reads of later chunks that may still be in flight
            auto &h0 = xh[k % NBUF][0], &h1 = xh[k % NBUF][1], &l0 = xl[k % NBUF][0], &l1 = xl[k % NBUF][1];
            if (left == 8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            else if (left == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            else if (left == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1));
            if constexpr (PARTS == 1) {
                l0 = h0;
                l1 = h1;
            }
            if constexpr (PARTS == 2) {
                acc0 = mma<F16>(wf[k][1], h0, acc0);
                acc1 = mma<F16>(wf[k][1], h1, acc1);
                acc0 = mma<F16>(wf[k][0], l0, acc0);
                acc1 = mma<F16>(wf[k][0], l1, acc1);
            }
            acc0 = mma<F16>(wf[k][0], h0, acc0);
            acc1 = mma<F16>(wf[k][0], h1, acc1);
            __builtin_amdgcn_sched_barrier(0);
            if (k + 3 < NCH) fetch(k + 3);
        }
    };

    constexpr int INFLIGHT = (RX - 2) * PPW;
#pragma unroll
    for (int q = 0; q < RX - 1; ++q) issue_next();
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("s_barrier" ::: "memory");

    int xslot = 0;
    f32x4 vq0 = f32x4{0.f, 0.f, 0.f, 0.f}, vq1 = vq0;
    typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
    u32x4v fop = {0u, 0u, 0u, 0u};
    // the residual pixels of x for stage B: requested while their slice is stage A's (rn*), used one step later (rc*)
    u32x2 rnh = {0u, 0u}, rnl = {0u, 0u}, rch = {0u, 0u}, rcl = {0u, 0u};
    // stream positions: stage A works on (UA, zA), stage C on (UC, zC); P positions in all
    const int ncol = (uend - ufirst + wgs_per_xcd - 1) / wgs_per_xcd;
    const int P = ncol * a.N;
    int cuA = ufirst, zA = 0;
    Unit UA = decode(cuA), UB = UA, UC = UA;
    int zB = 0, zC = 0;
    for (int p = 0; p < P + 2; ++p) {
        const bool hasA = p < P, hasB = p >= 1 && p <= P, hasC = p >= 2;
        // ---- the step's one barrier: x[p] has landed (this wave's pieces; after the barrier everyone's), t[p - 1] is complete, x[p - 1]'s slot and t[p]'s buffer are free
        if (hasA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(INFLIGHT) : "memory");
        if constexpr (ABL & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+v"(rnh), "+v"(rnl));   // (requested in the previous step, landed by the lgkmcnt(0) above)
        rch = rnh;
        rcl = rnl;
        if (hasA && !(ABL & 8)) issue_next();      // slice p + RX - 1 into the slot x[p - 1] left
        const unsigned tA = T_OFF + (p & 1) * TBUFB, tB = T_OFF + ((p & 1) ^ 1) * TBUFB;
        // ---- stage A of position p -------------------------------------------------------------------------------------------------
        if (hasA && !(ABL & 2)) {
            f32x4 accA[TA];
            if (nA == 2) {
                accA[0] = b0;
                accA[1] = b0;
                tile_mma2(lds0 + X_OFF + xslot * SLOTB + pa[0], lds0 + X_OFF + xslot * SLOTB + pa[1], tapA, std::integral_constant<int, PLANEB>{}, w0, accA[0], accA[1]);
            } else {
                accA[0] = tile_mma(lds0 + X_OFF + xslot * SLOTB + pa[0], tapA, std::integral_constant<int, PLANEB>{}, w0, b0);
                accA[1] = b0;
            }
#pragma unroll
            for (int j = 0; j < TA; ++j) {
                if (j >= nA) break;
                const f32x4 acc = accA[j];
                const int iy = UA.gy0 - 1 + ta_y[j], ix = UA.gx0 - 1 + ta_x[j];
                const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                if (ta_ok[j]) {
                    uint32_t h01, h23, l01, l23;
                    Fmt<PREC>::split2(relu_lim_bits(acc[0], inside ? 0x7f800000 : 0), relu_lim_bits(acc[1], inside ? 0x7f800000 : 0), h01, l01);
                    Fmt<PREC>::split2(relu_lim_bits(acc[2], inside ? 0x7f800000 : 0), relu_lim_bits(acc[3], inside ? 0x7f800000 : 0), h23, l23);
                    lds_store8(tA + ta_st[j] - T_OFF, h01, h23);
                    if constexpr (PARTS == 2) lds_store8(tA + ta_st[j] - T_OFF + TPLANEB, l01, l23);
                }
            }
        }
        if (hasA) {   // stage B's residual pixels of this slice, for the next step
            const unsigned xp = lds0 + X_OFF + xslot * SLOTB + pb_res;
            asm volatile("ds_read_b64 %0, %1" : "=v"(rnh) : "v"(xp));
            if constexpr (PARTS == 2) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(rnl) : "v"(xp), "n"(PLANEB));
        }
        // ---- stage B of position p - 1 ---------------------------------------------------------------------------------------------
        if (hasB) {
            if constexpr (!(ABL & 4)) {
                const unsigned fslot_off = F_OFF + ((p - 1) % 3) * FSLOTB;
                const f32x4 acc = tile_mma(lds0 + tB + pbo, tapB, std::integral_constant<int, TPLANEB>{}, w2, b2);
                float r0, r1, r2, r3;
                Fmt<PREC>::join2(rch[0], rcl[0], r0, r1);
                Fmt<PREC>::join2(rch[1], rcl[1], r2, r3);
                f32x4 v;
                v[0] = relu_bits(acc[0] + r0);
                v[1] = relu_bits(acc[1] + r1);
                v[2] = relu_bits(acc[2] + r2);
                v[3] = relu_bits(acc[3] + r3);
                uint32_t fh01, fh23, fl01, fl23;
                Fmt<PREC>::split2(v[0], v[1], fh01, fl01);
                Fmt<PREC>::split2(v[2], v[3], fh23, fl23);
                lds_store8(fslot_off + pb_f + g * 8, fh01, fh23);
                if constexpr (PARTS == 2) lds_store8(fslot_off + FPLANEB + pb_f + g * 8, fl01, fl23);
                fop = u32x4v{fh01, fh23, fl01, fl23};   // feat of position p - 1, channels 4g..4g+3 as [hi x4 | lo x4]: stage C's K octet for the slice behind it
                vq1 = vq0;
                vq0 = v;
            }
        } else {
            vq1 = vq0;
            fop = u32x4v{0u, 0u, 0u, 0u};
        }
        // ---- stage C of position q = p - 2: attention for slice zC of column UC (feat[zC + 1] = what stage B just wrote, unless the column ends here) ----
        if (hasC && !(ABL & 1)) {
            const int q = p - 2;
            const unsigned sm = F_OFF + ((q + 2) % 3) * FSLOTB, sc = F_OFF + (q % 3) * FSLOTB;
            if (zC == 0) {   // feat[-1] = 0: the ring slot behind holds the previous column's last slice, which nothing needs any more (the wave's own pixels)
                lds_store8(sm + pb_f + g * 8, 0u, 0u);
                if constexpr (PARTS == 2) lds_store8(sm + FPLANEB + pb_f + g * 8, 0u, 0u);
            }
            // chunk 0: K octet g = (slice zC - 1 + (g >> 1), channel octet g & 1) out of the ring; chunk 1: K octet g = channels 4g..4g+3 of feat[zC + 1] as
            // [hi x4 | lo x4], straight from stage B's registers (fragments [w_hi w_hi] and [w_lo 0]: two MFMAs)
            const unsigned ad0 = lds0 + ((g >> 1) ? sc : sm) + pb_f + (g & 1) * 16;
            short8 fh0, fl0;
            asm volatile("ds_read_b128 %0, %1" : "=v"(fh0) : "v"(ad0));
            if constexpr (PARTS == 2) {
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fl0) : "v"(ad0), "n"(FPLANEB));
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh0), "+v"(fl0));
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh0));
            }
            const u32x4v fz = zC == a.N - 1 ? u32x4v{0u, 0u, 0u, 0u} : fop;   // feat[N] = 0
            const short8 f1op = __builtin_bit_cast(short8, fz);
            f32x4 at = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PARTS == 2) {
                at = mma<F16>(w3f[1][1], f1op, at);
                at = mma<F16>(w3f[0][1], fh0, at);
                at = mma<F16>(w3f[0][0], fl0, at);
            }
            at = mma<F16>(w3f[1][0], f1op, at);
            at = mma<F16>(w3f[0][0], fh0, at);
            uint32_t ah01, ah23, al01, al23;
            Fmt<PREC>::split2(relu_bits(at[0]), relu_bits(at[1]), ah01, al01);
            Fmt<PREC>::split2(relu_bits(at[2]), relu_bits(at[3]), ah23, al23);
            const u32x4v bq = {ah01, ah23, al01, al23};
            const short8 b2op = __builtin_bit_cast(short8, bq);
            f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PARTS == 2) o = mma<F16>(w1f[1], b2op, o);
            o = mma<F16>(w1f[0], b2op, o);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = vq1[i] + relu_bits(o[i]);
            uint32_t h01, h23, l01, l23;
            Fmt<PREC>::split2(v[0], v[1], h01, l01);
            Fmt<PREC>::split2(v[2], v[3], h23, l23);
            const int64_t pix = (((int64_t)UC.b * a.N + zC) * a.H + UC.gy0 + pb_y) * a.W + UC.gx0 + pb_x;
            if constexpr (POOL) {   // 2x2 block: column neighbour = lane r ^ 1, row neighbour = lane r ^ 8
                float m[4];
                Fmt<PREC>::join2(h01, l01, m[0], m[1]);
                Fmt<PREC>::join2(h23, l23, m[2], m[3]);
                uint32_t ph01, ph23, pl01, pl23;
#pragma unroll
                for (int i = 0; i < 4; ++i) {   // non-negative values (sums of two ReLU results): maxima on the bit patterns
                    uint32_t mu = __float_as_uint(m[i]);
                    mu = max(mu, (uint32_t)__builtin_amdgcn_mov_dpp((int)mu, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
                    mu = max(mu, (uint32_t)__builtin_amdgcn_mov_dpp((int)mu, 0x128, 0xF, 0xF, true));   // row_ror:8
                    m[i] = __uint_as_float(mu);
                }
                Fmt<PREC>::split2(m[0], m[1], ph01, pl01);
                Fmt<PREC>::split2(m[2], m[3], ph23, pl23);
                if constexpr (PARTS == 2) {
                    swap16(ph01, pl01);
                    swap16(ph23, pl23);
                }
                if ((r & 9) == 0 && !(ABL & 32)) {
                    const int64_t pp = (((int64_t)UC.b * a.N + zC) * (a.H / 2) + (UC.gy0 / 2 + (wave >> 1))) * (a.W / 2) + UC.gx0 / 2 + 4 * (wave & 1) + ((r & 7) >> 1);
                    if constexpr (PARTS == 2) *reinterpret_cast<uint4 *>(a.pooled + pp * rec + (g & 1) * C + (g >> 1) * 8) = make_uint4(ph01, ph23, pl01, pl23);
                    else *reinterpret_cast<uint2 *>(a.pooled + pp * rec + g * 4) = make_uint2(ph01, ph23);
                }
            }
            if constexpr (PARTS == 2) {
                swap16(h01, l01);
                swap16(h23, l23);
                if ((ABL & 32) == 0 || h01 == 0x12345u) *reinterpret_cast<uint4 *>(a.out + pix * rec + (g & 1) * C + (g >> 1) * 8) = make_uint4(h01, h23, l01, l23);
            } else {
                *reinterpret_cast<uint2 *>(a.out + pix * rec + g * 4) = make_uint2(h01, h23);
            }
        }
        // ---- the positions move on --------------------------------------------------------------------------------------------------------
        UC = UB;
        zC = zB;
        UB = UA;
        zB = zA;
        if (hasA) {
            xslot = (xslot + 1 == RX) ? 0 : xslot + 1;
            if (++zA == a.N) {
                zA = 0;
                cuA += wgs_per_xcd;
                if (cuA < uend) UA = decode(cuA);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- srd_attention_mfma: the attention tail of the 32-channel SRD block (`FM_conv2.1.N_ch_attention`) on the matrix cores ------
//     out = feat + relu(conv1x1x1(relu(conv3x1x1(feat))))     (DEN.py:322-329; no BatchNorm, no bias)
// The fused VALU kernel (srd_attention_kernel) stops at 16 channels (C*C*4 FMAs per pixel); at 32 channels the two convs ran as
// two gather-GEMM launches with the intermediate in HBM.  Pointwise in space, so no LDS: a wave owns 16 consecutive pixels of a
// row and walks the slices with feat[z-1], feat[z], feat[z+1] as MFMA operand fragments in registers (each record is read once);
// conv3x1x1 = 3 chunks (one per slice) x 2 output tiles; its ReLU'd result, split to hi/lo in registers, is the operand of the
// 1x1x1 conv in place (K octet = the lane's own 4 channels as [hi | lo], fragments [w_hi w_hi] and [w_lo 0]).
template <int PREC>
__global__ __launch_bounds__(256) void srd_attention_mfma(const uint16_t *__restrict__ feat, uint16_t *__restrict__ out,
                                                          const uint16_t *__restrict__ w3f, const uint16_t *__restrict__ w1f, int B, int N,
                                                          int H, int W) {
    constexpr int PARTS = Fmt<PREC>::PARTS;
    constexpr bool F16 = (PREC == P_FP16);
    constexpr int C = 32, REC = PARTS * C;
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int64_t strip = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int strips_per_row = W / 16;
    const int64_t nstrips = (int64_t)B * H * strips_per_row;
    if (strip >= nstrips) return;
    const int sx = (int)(strip % strips_per_row);
    const int64_t by = strip / strips_per_row;
    const int y = (int)(by % H), b = (int)(by / H);
    const int64_t hw = (int64_t)H * W;
    const int64_t pix0 = ((int64_t)b * N * H + y) * W + sx * 16 + r;   // the lane's pixel in slice 0

    short8 w3[3][2][PARTS], w1[2][2][2];   // [slice chunk][output tile][part], [channel chunk][fragment][output tile]
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int pt = 0; pt < PARTS; ++pt) w3[k][nt][pt] = reinterpret_cast<const short8 *>(w3f)[((k * 2 + nt) * PARTS + pt) * 64 + lane];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int fr = 0; fr < PARTS; ++fr)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) w1[c][fr][nt] = reinterpret_cast<const short8 *>(w1f)[((c * PARTS + fr) * 2 + nt) * 64 + lane];

    auto load = [&](int z, short8 (&f)[PARTS]) {   // the lane's K octet (channels 8g..8g+7) of feat[z]; zeros outside the stack
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) f[pt] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if ((unsigned)z < (unsigned)N) {
            const uint16_t *p = feat + (pix0 + (int64_t)z * hw) * REC + g * 8;
#pragma unroll
            for (int pt = 0; pt < PARTS; ++pt) f[pt] = *reinterpret_cast<const short8 *>(p + pt * C);
        }
    };
    // feat[z] at the lane's RESULT channels nt*16 + 4g .. +3 (the residual; the operand octet holds other channels): requested one slice ahead
    auto load_res = [&](int z, uint2 (&rh)[2], uint2 (&rl)[2]) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            rh[nt] = make_uint2(0, 0);
            rl[nt] = make_uint2(0, 0);
            if (z < N) {
                const uint16_t *cp = feat + (pix0 + (int64_t)z * hw) * REC + nt * 16 + g * 4;
                rh[nt] = *reinterpret_cast<const uint2 *>(cp);
                if constexpr (PARTS == 2) rl[nt] = *reinterpret_cast<const uint2 *>(cp + C);
            }
        }
    };
    // The slice walk is a chain of dependent loads unless they run ahead: operand records two slices ahead, the residual one slice ahead (the
    // kernel has only 8 waves of work per SIMD, 3 resident: with each slice's loads consumed in the iteration that issued them it ran at 3.1 TB/s)
    short8 f[4][PARTS];
    uint2 rh[2][2], rl[2][2];
    load(-1, f[0]);
    load(0, f[1]);
    load(1, f[2]);
    load_res(0, rh[0], rl[0]);
    for (int z = 0; z < N; ++z) {
        load(z + 2, f[3]);
        load_res(z + 1, rh[1], rl[1]);
        f32x4 at[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            at[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if constexpr (PARTS == 2) {
                    at[nt] = mma<F16>(w3[k][nt][1], f[k][0], at[nt]);
                    at[nt] = mma<F16>(w3[k][nt][0], f[k][1], at[nt]);
                }
                at[nt] = mma<F16>(w3[k][nt][0], f[k][0], at[nt]);
            }
        }
        short8 b2[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            uint32_t ah01, ah23, al01, al23;
            Fmt<PREC>::split2(relu_bits(at[c][0]), relu_bits(at[c][1]), ah01, al01);
            Fmt<PREC>::split2(relu_bits(at[c][2]), relu_bits(at[c][3]), ah23, al23);
            typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
            const u32x4v bq = {ah01, ah23, al01, al23};
            b2[c] = __builtin_bit_cast(short8, bq);
        }
        const int64_t pix = pix0 + (int64_t)z * hw;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if constexpr (PARTS == 2) o = mma<F16>(w1[c][1][nt], b2[c], o);
                o = mma<F16>(w1[c][0][nt], b2[c], o);
            }
            float c0, c1, c2, c3;
            Fmt<PREC>::join2(rh[0][nt].x, rl[0][nt].x, c0, c1);
            Fmt<PREC>::join2(rh[0][nt].y, rl[0][nt].y, c2, c3);
            uint32_t h01, h23, l01, l23;
            Fmt<PREC>::split2(c0 + relu_bits(o[0]), c1 + relu_bits(o[1]), h01, l01);
            Fmt<PREC>::split2(c2 + relu_bits(o[2]), c3 + relu_bits(o[3]), h23, l23);
            if constexpr (PARTS == 2) {
                swap16(h01, l01);
                swap16(h23, l23);
                *reinterpret_cast<uint4 *>(out + pix * REC + (g & 1) * C + (nt * 2 + (g >> 1)) * 8) = make_uint4(h01, h23, l01, l23);
            } else {
                *reinterpret_cast<uint2 *>(out + pix * REC + nt * 16 + g * 4) = make_uint2(h01, h23);
            }
        }
#pragma unroll
        for (int pt = 0; pt < PARTS; ++pt) {
            f[0][pt] = f[1][pt];
            f[1][pt] = f[2][pt];
            f[2][pt] = f[3][pt];
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            rh[0][nt] = rh[1][nt];
            rl[0][nt] = rl[1][nt];
        }
    }
}

hipError_t launch_srd_attention_mfma(int prec, const uint16_t *feat, uint16_t *out, const uint16_t *w3f, const uint16_t *w1f, int B, int N,
                                     int H, int W, hipStream_t s) {
    if (W % 16) return hipErrorInvalidValue;
    const int64_t nstrips = (int64_t)B * H * (W / 16);
    const dim3 grid((unsigned)((nstrips + 3) / 4)), block(256);
    switch (prec) {
        case P_BF16X3: hipLaunchKernelGGL((srd_attention_mfma<P_BF16X3>), grid, block, 0, s, feat, out, w3f, w1f, B, N, H, W); break;
        case P_FP16: hipLaunchKernelGGL((srd_attention_mfma<P_FP16>), grid, block, 0, s, feat, out, w3f, w1f, B, N, H, W); break;
        case P_BF16: hipLaunchKernelGGL((srd_attention_mfma<P_BF16>), grid, block, 0, s, feat, out, w3f, w1f, B, N, H, W); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

void srd_roll_tile(int *ty, int *tx) {
    *ty = 8;
    *tx = 16;
}

// The three fused blocks' tables: [prec][plain | pooled]; beside them (make ABL=1) the timing ablations of the split-bf16 pooled form, selected
// with DFFW_SRD_ABL (wrong results with any bit set).  The production rows' names are labels, not the symbols (which end in the defaulted ", 0"): the
// spelling the dispatch pins and the profile tools were recorded with; srd_pipe16's always carried it.
#define DFFW_SRD_ROWS(kernel, P)                                                                      \
    {"dffw::" #kernel "<" #P ", false>", kernel<P, false>, 256}, {"dffw::" #kernel "<" #P ", true>", kernel<P, true>, 256}

static const KernelRow<SrdArgs, const float *, const float *> kSrdRoll[] = {
    DFFW_SRD_ROWS(srd_roll_kernel, 0), DFFW_SRD_ROWS(srd_roll_kernel, 1), DFFW_SRD_ROWS(srd_roll_kernel, 2),
};
#ifdef DFFW_ABL_BUILD
#define R(A) {A, DFFW_ROW(256, srd_roll_kernel, 0, true, A)}
static const AblRow<KernelRow<SrdArgs, const float *, const float *>> kSrdRollAbl[] = {R(1), R(2), R(4), R(6), R(7), R(8), R(16), R(32), R(40), R(23)};
#undef R
#endif
static const KernelRow<SrdArgs, const float *, const float *> *select_srd_roll(int prec, bool pool) {
#ifdef DFFW_ABL_BUILD
    if (prec == P_BF16X3 && pool)
        if (const auto *row = abl_row(kSrdRollAbl, "DFFW_SRD_ABL")) return row;
#endif
    return prec_row(kSrdRoll, prec, 2, pool);
}
void srd_roll_kernel_name(int prec, bool pool, char *buf, int n) { copy_row_name(select_srd_roll(prec, pool), buf, n); }
hipError_t launch_srd_roll(int prec, const SrdArgs &a, hipStream_t s) {
    return launch_row(select_srd_roll(prec, a.pooled != nullptr), a.total_tiles, a.wgs > 0 ? a.wgs : 768, 1, s, a, a.w3, a.w1);   // 768: three resident workgroups per CU
}

void srd_roll16_tile(int *ty, int *tx) {
    *ty = 4;
    *tx = 16;
}

static const SrdRow kSrdRoll16[] = {
    DFFW_SRD_ROWS(srd_roll16_kernel, 0), DFFW_SRD_ROWS(srd_roll16_kernel, 1), DFFW_SRD_ROWS(srd_roll16_kernel, 2),
};
#ifdef DFFW_ABL_BUILD
#define R(A) {A, DFFW_ROW(256, srd_roll16_kernel, 0, true, A)}
static const AblRow<SrdRow> kSrdRoll16Abl[] = {R(1), R(2), R(4), R(6), R(7), R(8), R(16), R(32), R(40), R(23)};
#undef R
#endif
static const SrdRow *select_srd_roll16(int prec, bool pool) {
#ifdef DFFW_ABL_BUILD
    if (prec == P_BF16X3 && pool)
        if (const SrdRow *row = abl_row(kSrdRoll16Abl, "DFFW_SRD_ABL")) return row;
#endif
    return prec_row(kSrdRoll16, prec, 2, pool);
}
void srd_roll16_kernel_name(int prec, bool pool, char *buf, int n) { copy_row_name(select_srd_roll16(prec, pool), buf, n); }
hipError_t launch_srd_roll16(int prec, const SrdArgs &a, hipStream_t s) {
    return launch_row(select_srd_roll16(prec, a.pooled != nullptr), a.total_tiles, a.wgs > 0 ? a.wgs : 512, 1, s, a);   // 512: two resident workgroups per CU
}

static const SrdRow kSrdPipe16[] = {   // [prec][plain | pooled]
#define R(...) DFFW_ROW(256, srd_pipe16_kernel, __VA_ARGS__)
    R(0, false, 0), R(0, true, 0), R(1, false, 0), R(1, true, 0), R(2, false, 0), R(2, true, 0),
#undef R
};
void srd_pipe16_kernel_name(int prec, bool pool, char *buf, int n) { copy_row_name(prec_row(kSrdPipe16, prec, 2, pool), buf, n); }
hipError_t launch_srd_pipe16(int prec, const SrdArgs &a, hipStream_t s) {
    return launch_row(prec_row(kSrdPipe16, prec, 2, a.pooled != nullptr), a.total_tiles, a.wgs > 0 ? a.wgs : 512, 1, s, a);   // 512: two resident workgroups per CU
}
#undef DFFW_SRD_ROWS

}  // namespace dffw
