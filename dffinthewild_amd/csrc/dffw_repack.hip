// Repacking conv weights on the GPU: BatchNorm folding and the operand layouts of dffw_pack.cpp, from parameters that live in device
// memory.  Two kernels, both enqueue-only, without atomics and with a fixed element -> thread assignment:
//   repack_fold_kernel    per packed layer: scratch = [weights * scale | shortcut weights | shift | raw conv bias], float64 in the host's operation order
//   repack_gather_kernel  every operand buffer of every layer from the scratch, through the source maps of the plan
// Bit-identity with the host packer rests on two things: no expression here is contracted into an fma (the host build has none), and nothing flushes
// subnormals (the kernels run in the default IEEE denormal mode; `v - bf2f(hi)` is exact in fp32, subnormal results included).
#include "dffw_device.h"
#include "dffw_repack.h"

#pragma clang fp contract(off)   // the whole file: the host packer's build has no fma

namespace dffw {

namespace {

// sqrt(x) correctly rounded: one residual step on the library's result.  x - s * s is exact in one fma when s is within an ulp of the root, and
// fma(r, 1 / (2 s), s) then rounds to the nearest double; a result that was already the nearest one is left as it is (|r / (2 s)| < ulp / 2).
__device__ __forceinline__ double sqrt_rn(double x) {
    const double s = sqrt(x);
    if (!(s > 0.0) || !(s < 1.7976931348623157e308)) return s;
    const double r = __fma_rn(-s, s, x);
    return __fma_rn(r, 0.5 / s, s);
}

// scale[c] and shift[c] as pack_conv computes them: every operation a separate float64 rounding
__device__ __forceinline__ double fold_scale(const FoldLayer &L, int c) {
    if (!L.g) return 1.0;
    const double g = (double)L.g[c], v = (double)L.v[c];
    const double ve = __dadd_rn(v, 1e-5);
    return g / sqrt_rn(ve);
}
__device__ __forceinline__ double fold_shift(const FoldLayer &L, int c, double scale) {
    double shift = 0.0;
    if (L.g) {
        const bool zs = (L.flags & FOLD_ZERO_SHIFT) != 0;
        const double b = zs ? 0.0 : (double)L.b[c], m = zs ? 0.0 : (double)L.m[c];
        shift = __dsub_rn(b, __dmul_rn(m, scale));
    }
    if (L.cb) shift = __dadd_rn(shift, __dmul_rn((double)L.cb[c], scale));
    return shift;
}

}  // namespace

__global__ __launch_bounds__(FOLD_BLOCK) void repack_fold_kernel(const FoldTable t) {
    __shared__ double s_scale[FOLD_MAX_COUT];
    const int blk = blockIdx.x;
    int lo = 0, hi = t.n_layers;   // block_start[lo] <= blk < block_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.layer[mid].block_start <= blk) lo = mid;
        else hi = mid;
    }
    const FoldLayer &L = t.layer[lo];
    const int chunk = blk - L.block_start, tid = threadIdx.x;
    float *__restrict__ out = t.scratch + L.scratch_off;
    if (tid < L.cout) {
        const double sc = fold_scale(L, tid);
        s_scale[tid] = sc;
        if (chunk == 0) {   // the layer's first workgroup also writes the per-channel tail of the scratch
            out[L.n_w + L.n_sc + tid] = (float)fold_shift(L, tid, sc);
            if (L.cb) out[L.n_w + L.n_sc + L.cout + tid] = L.cb[tid];
        }
    }
    __syncthreads();
    const int n = L.n_w + L.n_sc;
    const int e0 = chunk * FOLD_CHUNK;
#pragma unroll
    for (int k = 0; k < FOLD_CHUNK / FOLD_BLOCK; ++k) {
        const int i = e0 + k * FOLD_BLOCK + tid;
        if (i >= n) break;
        if (i >= L.n_w) {
            out[i] = L.sc[i - L.n_w];   // the folded shortcut is not scaled by this layer's BatchNorm
            continue;
        }
        const int co = (L.flags & FOLD_TRANSPOSED) ? (i / L.kvol) % L.cout : i / L.row;
        const int r = i - co * L.row;   // (not used by the transposed layout: src_row = row, src_off = 0, the source index is i)
        const int si = (L.flags & FOLD_TRANSPOSED) ? i : co * L.src_row + L.src_off + r;
        out[i] = (float)__dmul_rn((double)L.w[si], s_scale[co]);
    }
}

template <int PREC>
__global__ __launch_bounds__(GATHER_BLOCK) void repack_gather_kernel(const GatherJob *__restrict__ jobs, int n_jobs) {
    const int blk = blockIdx.x;
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].block_start <= blk) lo = mid;
        else hi = mid;
    }
    const GatherJob J = jobs[lo];
    const int unit = (blk - J.block_start) * GATHER_BLOCK + threadIdx.x;
    if (unit >= J.units) return;
    const float *__restrict__ src = J.src;
    constexpr int PARTS = Fmt<PREC>::PARTS;
    if (J.kind == RK_F32) {
        const int m = J.map[unit];
        reinterpret_cast<float *>(J.dst)[unit] = m < 0 ? 0.f : src[m];
        return;
    }
    // 8 map entries = 32 bytes, one 16-byte store per part
    const int4 m0 = reinterpret_cast<const int4 *>(J.map)[2 * (size_t)unit], m1 = reinterpret_cast<const int4 *>(J.map)[2 * (size_t)unit + 1];
    const int m[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    uint16_t h[8], l[8];
    if (J.kind == RK_FRAGS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) Fmt<PREC>::split(m[j] < 0 ? 0.f : src[m[j]], h[j], l[j]);
        const int f = unit >> 6, lane = unit & 63;
        uint16_t *dst = reinterpret_cast<uint16_t *>(J.dst) + ((size_t)f * PARTS * 512 + (size_t)lane * 8);
        *reinterpret_cast<uint4 *>(dst) = make_uint4(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16, h[4] | (uint32_t)h[5] << 16, h[6] | (uint32_t)h[7] << 16);
        if constexpr (PARTS == 2)
            *reinterpret_cast<uint4 *>(dst + 512) = make_uint4(l[0] | (uint32_t)l[1] << 16, l[2] | (uint32_t)l[3] << 16, l[4] | (uint32_t)l[5] << 16, l[6] | (uint32_t)l[7] << 16);
        return;
    }
    // RK_SLOTS: 8 consecutive 16-bit slots, each 2 * source + part
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint16_t a, b;
        Fmt<PREC>::split(m[j] < 0 ? 0.f : src[m[j] >> 1], a, b);
        h[j] = m[j] < 0 ? (uint16_t)0 : ((m[j] & 1) ? b : a);
    }
    uint16_t *dst = reinterpret_cast<uint16_t *>(J.dst) + (size_t)unit * 8;
    *reinterpret_cast<uint4 *>(dst) = make_uint4(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16, h[4] | (uint32_t)h[5] << 16, h[6] | (uint32_t)h[7] << 16);
}

const char *fold_kernel_name() { return "dffw::repack_fold_kernel"; }
const char *gather_kernel_name() { return "dffw::repack_gather_kernel"; }

hipError_t launch_repack_fold(const FoldTable &t, hipStream_t s) {
    hipLaunchKernelGGL(repack_fold_kernel, dim3((unsigned)t.n_blocks), dim3(FOLD_BLOCK), 0, s, t);
    return hipGetLastError();
}

hipError_t launch_repack_gather(int prec, const GatherJob *jobs, int n_jobs, int n_blocks, hipStream_t s) {
    const dim3 g((unsigned)n_blocks), b(GATHER_BLOCK);
    if (prec == P_BF16X3) hipLaunchKernelGGL(repack_gather_kernel<P_BF16X3>, g, b, 0, s, jobs, n_jobs);
    else if (prec == P_FP16) hipLaunchKernelGGL(repack_gather_kernel<P_FP16>, g, b, 0, s, jobs, n_jobs);
    else hipLaunchKernelGGL(repack_gather_kernel<P_BF16>, g, b, 0, s, jobs, n_jobs);
    return hipGetLastError();
}

}  // namespace dffw
