// The Adam step over a list of fp32 tensors: the launch contract between dffw_optim.hip (kernel) and dffw_optim.cpp (C ABI).
// The tensor table travels as the kernel's argument: no device allocation, no copy, nothing to keep alive after the launch is enqueued.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dffw {

constexpr int ADAM_TENSORS_PER_LAUNCH = 80;   // 80 * 40 bytes of table + the scalars: 3 240 bytes of kernarg (the static_assert below holds it under 4 KB)
constexpr int ADAM_BLOCK = 256;
constexpr int ADAM_CHUNK = 4096;              // elements per workgroup: 256 lanes x 4 rounds x 16 bytes; a chunk never spans two tensors
// a launch takes at most this many chunks (2^34 elements), so that grid.x * ADAM_BLOCK stays below 2^32; one tensor (numel < 2^31) never has more
constexpr int64_t ADAM_CHUNKS_PER_LAUNCH = (int64_t)1 << 22;

// Entry i of the table is chunks [chunk_start[i], chunk_start[i + 1]) of the grid: chunk c of it covers elements [c * ADAM_CHUNK, min(numel, (c + 1) *
// ADAM_CHUNK)).  Every entry has numel >= 1 (the host drops empty tensors), so chunk_start is strictly increasing and chunk_start[n_tensors] = grid.x.
struct AdamTable {
    float *param[ADAM_TENSORS_PER_LAUNCH];
    const float *grad[ADAM_TENSORS_PER_LAUNCH];
    float *exp_avg[ADAM_TENSORS_PER_LAUNCH];
    float *exp_avg_sq[ADAM_TENSORS_PER_LAUNCH];
    int numel[ADAM_TENSORS_PER_LAUNCH];
    int chunk_start[ADAM_TENSORS_PER_LAUNCH + 1];
    int n_tensors;
    // the step's scalars, computed in double by the host and rounded once: beta1, beta2, 1 - beta1, 1 - beta2, sqrt(1 - beta2^t), lr / (1 - beta1^t), eps
    float beta1, beta2, c1, c2, bc2_sqrt, step_size, eps;
};
static_assert(sizeof(AdamTable) <= 4096 - 256, "the Adam table and the launch's hidden arguments must fit 4 KB of kernarg");

const char *adam_kernel_name();
hipError_t launch_adam(const AdamTable &t, hipStream_t s);   // grid = t.chunk_start[t.n_tensors] workgroups of ADAM_BLOCK

}  // namespace dffw
