// Transposed LDS reads of the weight-gradient kernels (dffw_conv_wgrad.hip, dffw_conv_pw_wgrad.hip): the contraction runs over pixels while the
// records are channels-last, so both MFMA operands come out of a [pixel][channel] LDS image through ds_read_b64_tr_b16.
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

}  // namespace dffw
