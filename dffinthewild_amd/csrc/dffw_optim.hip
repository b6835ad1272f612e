// The Adam step over a list of fp32 tensors in one launch.  Memory-bound streaming: 16 bytes read and 12 written per element, no
// reuse, no LDS, no atomics.  A workgroup owns one chunk of ADAM_CHUNK elements of ONE tensor and finds it by a binary search of the chunk prefix
// sums in the kernarg (wave-uniform scalar loads).  Every element goes through adam_one(), whichever path loads it: the bits of a tensor's result
// do not depend on its alignment, its place in the list, the launch it lands in or the grid.
#include "dffw_optim.h"

namespace dffw {

namespace {

struct AdamScalars {
    float beta1, beta2, c1, c2, bc2_sqrt, step_size, eps;
};

// One element, every operation rounded once to fp32 in exactly this order (no contraction into fma; `/` and sqrtf are the correctly rounded ones):
//   m' = beta1 m + c1 g    v' = beta2 v + c2 (g g)    d = sqrt(v') / bc2_sqrt + eps    p' = p - step_size (m' / d)
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamScalars &k) {
#pragma clang fp contract(off)
    const float m1 = k.beta1 * m;
    const float gm = k.c1 * g;
    const float mn = m1 + gm;
    const float v1 = k.beta2 * v;
    const float gg = g * g;
    const float gv = k.c2 * gg;
    const float vn = v1 + gv;
    const float r = sqrtf(vn);
    const float rs = r / k.bc2_sqrt;
    const float d = rs + k.eps;
    const float q = mn / d;
    const float u = k.step_size * q;
    p = p - u;
    m = mn;
    v = vn;
}

__device__ __forceinline__ void adam_four(float4 &p, const float4 &g, float4 &m, float4 &v, const AdamScalars &k) {
    adam_one(p.x, g.x, m.x, v.x, k);
    adam_one(p.y, g.y, m.y, v.y, k);
    adam_one(p.z, g.z, m.z, v.z, k);
    adam_one(p.w, g.w, m.w, v.w, k);
}

}  // namespace

__global__ __launch_bounds__(ADAM_BLOCK) void adam_kernel(const AdamTable t) {
    const int chunk = blockIdx.x;
    // chunk_start[lo] <= chunk < chunk_start[hi]: at most 7 uniform steps for 80 entries
    int lo = 0, hi = t.n_tensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.chunk_start[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    const int64_t base = (int64_t)(chunk - t.chunk_start[lo]) * ADAM_CHUNK;
    const int n = (int)min((int64_t)ADAM_CHUNK, (int64_t)t.numel[lo] - base);   // elements of this chunk, 1 .. ADAM_CHUNK
    float *__restrict__ p = t.param[lo] + base;
    const float *__restrict__ g = t.grad[lo] + base;
    float *__restrict__ m = t.exp_avg[lo] + base;
    float *__restrict__ v = t.exp_avg_sq[lo] + base;
    const AdamScalars k{t.beta1, t.beta2, t.c1, t.c2, t.bc2_sqrt, t.step_size, t.eps};
    const int tid = threadIdx.x;

    // base is a multiple of 16 KB, so a chunk is 16-byte aligned exactly when its tensor is
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    if (!vec) {
        for (int i = tid; i < n; i += ADAM_BLOCK) adam_one(p[i], g[i], m[i], v[i], k);
        return;
    }
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    const int nv = n >> 2;
    if (nv == ADAM_CHUNK / 4) {
        // a whole chunk: all 16 loads of the lane are in flight before the first use
        constexpr int R = ADAM_CHUNK / 4 / ADAM_BLOCK;
        float4 pp[R], gg[R], mm[R], vv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * ADAM_BLOCK + tid;
            pp[r] = p4[i]; gg[r] = g4[i]; mm[r] = m4[i]; vv[r] = v4[i];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * ADAM_BLOCK + tid;
            adam_four(pp[r], gg[r], mm[r], vv[r], k);
            p4[i] = pp[r]; m4[i] = mm[r]; v4[i] = vv[r];
        }
        return;
    }
    for (int i = tid; i < nv; i += ADAM_BLOCK) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        adam_four(pp, g4[i], mm, vv, k);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    const int i = (nv << 2) + tid;   // the tensor's tail: at most 3 elements
    if (i < n) adam_one(p[i], g[i], m[i], v[i], k);
}

const char *adam_kernel_name() { return "dffw::adam_kernel"; }

hipError_t launch_adam(const AdamTable &t, hipStream_t s) {
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)t.chunk_start[t.n_tensors]), dim3(ADAM_BLOCK), 0, s, t);
    return hipGetLastError();
}

}  // namespace dffw
