// What the three MFMA weight-gradient kernels share (conv_wgrad_kernel of dffw_conv_wgrad.hip, conv_pw_wgrad_kernel of dffw_conv_pw_wgrad.hip,
// stem_wgrad_kernel of dffw_stem_wgrad.hip).  The contraction runs over pixels while the records are channels-last, so the MFMA operands come out
// of a [pixel][channel] LDS image through ds_read_b64_tr_b16 (both operands of the two conv kernels, the row operand of the stem's); every step
// is the forward's three products, and every accumulator row is flushed into float64.
#pragma once
#include <hip/hip_runtime.h>

#include "dffw_device.h"

namespace dffw {

typedef __attribute__((ext_vector_type(4))) short tr_s4;

// 4 pixels x 16 channels of a [pixel][channel] LDS image, transposed: this lane addresses 8 bytes (4 channels of one pixel), and receives one
// channel of the group's 4 pixels.  All 64 lanes must be active
__device__ __forceinline__ tr_s4 tr_read(const char *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr_s4 *)p);
}
__device__ __forceinline__ short8 tr_pair(const char *p0, const char *p1) {
    const tr_s4 u = tr_read(p0), v = tr_read(p1);
    return short8{u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
}

// This lane's piece of a transposed read: pixel q of its 16-lane group's 4, channels 4p .. 4p + 3.  The four groups of a wave are (half, gl): the
// two 16-pixel halves of a 32-deep MFMA step, and in each the pixels 4 gl .. 4 gl + 3 of the first read (8 pixels on for the second)
struct TrLane {
    int q, p, half, gl;
};
__device__ __forceinline__ TrLane tr_lane(int lane) { return TrLane{(lane >> 2) & 3, lane & 3, lane >> 5, (lane >> 4) & 1}; }

// One 32-deep step on the parts of both operands: the three products of every forward kernel, small ones first
template <int PREC, int PARTS>
__device__ __forceinline__ f32x4 mma3(const short8 (&ag)[PARTS], const short8 (&bf)[PARTS], f32x4 acc) {
    static_assert(PARTS == Fmt<PREC>::PARTS, "one operand per part of the precision");
    if constexpr (PARTS == 2) {
        acc = mma<false>(ag[1], bf[0], acc);
        acc = mma<false>(ag[0], bf[1], acc);
    }
    return mma<PREC == P_FP16>(ag[0], bf[0], acc);
}

// One accumulator value into its float64 sum: the first flush of a block is a plain store (the workspace need not be cleared)
__device__ __forceinline__ void flush_f64(double *d, float v, bool first) { *d = first ? (double)v : *d + (double)v; }

}  // namespace dffw
