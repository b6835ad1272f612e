// The fused SRD blocks of the depth network (srd_roll, srd_roll16, srd_pipe16) and the MFMA attention tail of its 32-channel block
// (dffw_srd_roll.hip): host/device declarations.  SrdArgs is also the argument block of the alignment network's streaming feature
// blocks (dffw_align.h).
#pragma once
#include "dffw_internal.h"

namespace dffw {

struct SrdArgs {
    const uint16_t *x;        // block input (B,N,H,W,8) in storage format
    uint16_t *out;            // block output, same shape
    uint16_t *pooled;         // (B,N,H/2,W/2,8) max-pool (1,2,2) of out, or null
    const uint16_t *w0, *w2;  // conv.0 / conv.2 filters as MFMA A-fragments [3 chunks][part][64 lanes][8] in pixel-pair form (chunk = filter row, pack_conv)
    const float *b0, *b2;     // their BatchNorm shifts (>= 16 floats, zero padded)
    const float *w3, *w1;     // attention weights fp32 [kz][ci][co] and [ci][co] (unused by the MFMA form, kept for reference)
    const uint16_t *w3f, *w1f;   // the same as MFMA A-fragments: conv3x1x1 [2 chunks][part][64][8], conv1x1x1 [part][64][8] (pack_conv)
    const uint16_t *zero;     // >= 16 zero bytes (out-of-image LDS-DMA lanes)
    int B, N, H, W;
    int tiles_y, tiles_x, total_tiles;   // 8 x 16 columns per sample, B * tiles_y * tiles_x
    int wgs;                  // workgroups to launch (0: three per CU)
#ifdef DFFW_TRACE_BUILD
    unsigned long long *trace;   // debug step timeline (make TRACE=1, DFFW_TRACE_LAYER); the field exists in trace builds only (a larger
                                 // argument block changes the kernels' register allocation)
#endif
};

constexpr int SRD_CHUNKS = 3;
void srd_roll_tile(int *ty, int *tx);
hipError_t launch_srd_roll(int prec, const SrdArgs &a, hipStream_t s);
void srd_roll_kernel_name(int prec, bool pool, char *buf, int n);
// the 16-channel block (columns of 4 x 16 pixels; 1x3x3 filters as 5 chunks of 2 taps x 16 channels)
constexpr int SRD16_CHUNKS = 5;
void srd_roll16_tile(int *ty, int *tx);
hipError_t launch_srd_roll16(int prec, const SrdArgs &a, hipStream_t s);
void srd_roll16_kernel_name(int prec, bool pool, char *buf, int n);
// srd_pipe16 (round 6): the same block as a software pipeline over the slice stream (stage A of position p, B of p - 1, C of p - 2 in one step, one barrier)
hipError_t launch_srd_pipe16(int prec, const SrdArgs &a, hipStream_t s);
void srd_pipe16_kernel_name(int prec, bool pool, char *buf, int n);

// the attention tail of the 32-channel block on the matrix cores (no LDS; W % 16 == 0).  w3f: [3 slices][2 output tiles][part][64][8],
// w1f: [2 channel chunks][fragment][2 output tiles][64][8] (pack_conv)
hipError_t launch_srd_attention_mfma(int prec, const uint16_t *feat, uint16_t *out, const uint16_t *w3f, const uint16_t *w1f, int B, int N,
                                     int H, int W, hipStream_t s);

}  // namespace dffw
