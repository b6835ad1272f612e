// Training loss of the five training scripts (train_codes/train_code_*.py) and its gradient through the four regression heads
// (Depth_Estimation_Network.py:89-98, 118-134) down to the score volumes: the first link of the backward chain.
//
//   v_n = bilinear(score_k[b,n], i)   p_n = softplus(v_n) + 1e-6   S = sum_n p_n   d_k = sum_n f_n p_n / S      (the forward heads, bit for bit)
//   Loss_k = sum_i c_i m_i ((d_k - gt)/r)^2 / Z,  Z = sum_i c_i m_i,  Total = sum_k w_k Loss_k
//   dTotal/dv_n(i) = [2 w_k c_i m_i (d_k - gt) / (r^2 Z)] * (f_n - d_k)/S * sigmoid(v_n);  dTotal/dscore_k = upsample^T(dTotal/dv)
//
// Launches: loss_norm_partial / loss_norm_finish (Z, float64, fixed two-stage order), one head kernel per head, loss_finish.
// The adjoint of the upsample is a GATHER: a workgroup owns a tile of the low-resolution grid, evaluates every output pixel whose bilinear taps
// touch the tile (the tile's footprint plus half a cell on every side) once, parks the N per-slice adjoints of those pixels in LDS and then sums,
// per low-resolution element, its 2s x 2s contributors (s = H/h) in a fixed order, separably: along x into row sums, then along y.  No atomics,
// no run-order-dependent sum: two runs are bit-identical.  Nothing of size (B,N,H,W) goes through HBM; slices beyond the LDS plan (LOSS_NCH at a
// time) are served by re-evaluating v_n and sigmoid(v_n) from the scores.  The full-resolution head is pointwise.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/dffw.h"
#include "dffw_device.h"
#include "dffw_heads.h"
#include "dffw_internal.h"

namespace dffw {

constexpr int LOSS_NORM_BLKS = 256;    // block partials of the normaliser pass
constexpr int LOSS_FULL_BLKS = 2048;   // persistent grid of the pointwise head (one loss partial per workgroup)

struct LossArgs {
    const float *fd;
    int64_t fsb, fsn, fsh, fsw;
    const float *gt;
    const uint8_t *mask;
    const float *conf;
    int B, N, H, W;
    double scale;   // 2 w_k / r^2: times (d - gt) c / Z = dTotal/dd
};

// sum over the 256 threads of a workgroup in a fixed order (wave butterflies, then the four waves)
__device__ __forceinline__ double block_sum_256(double v, double *sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- normaliser: Z = sum_i c_i m_i in float64 (block partials, then one thread in block order, as dffw_metrics) ----
__global__ __launch_bounds__(256) void loss_norm_partial_kernel(const uint8_t *__restrict__ mask, const float *__restrict__ conf, int64_t total,
                                                                 double *__restrict__ partial) {
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        if (mask[i]) s += conf ? (double)conf[i] : 1.0;
    __shared__ double sh[4];
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void loss_norm_finish_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ Z) {
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int i = 0; i < nblk; ++i) v += partial[i];
        *Z = v;
    }
}

// dTotal/dd of one pixel (0 for a pixel outside the mask, by selection: its gt may be NaN) and its loss term c (d - gt)^2 in float64
__device__ __forceinline__ float pixel_loss(const LossArgs &a, int64_t gi, float d, float kf, bool owned, double &lsum) {
#pragma clang fp contract(off)
    if (!a.mask[gi]) return 0.f;
    const float c = a.conf ? a.conf[gi] : 1.f, g = a.gt[gi];
    if (owned) {
        const double df = (double)d - (double)g;
        lsum += (double)c * (df * df);
    }
    return (kf * c) * (d - g);
}

// ---- upsampled heads (s = 2, 4, 8): grid (tiles of TY x TX low-resolution elements, B) ----
template <int S, int TY, int TX>
__global__ __launch_bounds__(256) void loss_head_tile_kernel(const LossArgs a, const float *__restrict__ score, int h, int w, float *__restrict__ pred,
                                                              float *__restrict__ grad, const double *__restrict__ Zp, double *__restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int RH = S * TY + S, RW = S * TX + S, P = RH * RW, Q = (P + 255) / 256;
    static_assert(Q <= 4, "at most four footprint pixels per thread");
    __shared__ float adj[LOSS_NCH * P];        // [slice of the chunk][footprint pixel]: sigmoid(v_n), then dTotal/dv_n
    __shared__ float tmp[LOSS_NCH * RH * TX];  // [slice][footprint row][element column]: the x-sums
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const int tiles_x = (w + TX - 1) / TX;
    const int tj = blockIdx.x / tiles_x, ti = blockIdx.x - tj * tiles_x;
    const int64_t b = blockIdx.y;
    const int j0 = tj * TY, i0 = ti * TX, Y0 = S * j0 - S / 2, X0 = S * i0 - S / 2;
    const int N = a.N, H = a.H, W = a.W;
    const int64_t hw = (int64_t)h * w;
    const float *__restrict__ sp = score + b * N * hw;
    const float sch = (float)h / (float)H, scw = (float)w / (float)W;
    const float kf = (float)(a.scale / *Zp);
    const int nch0 = N < LOSS_NCH ? N : LOSS_NCH;
    float gS[Q], dd[Q];
    double lsum = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int pix = q * 256 + tid;
        gS[q] = 0.f;
        dd[q] = 0.f;
        if (pix >= P) continue;
        const int ry = pix / RW, rx = pix - ry * RW, Y = Y0 + ry, X = X0 + rx;
        if (Y < 0 || Y >= H || X < 0 || X >= W) {
            for (int n = 0; n < nch0; ++n) adj[n * P + pix] = 0.f;
            continue;
        }
        const Taps t = make_taps(X, Y, h, w, sch, scw);
        const float *__restrict__ fp = a.fd + b * a.fsb + Y * a.fsh + X * a.fsw;
        float num = 0.f, den = 0.f;
        for (int n = 0; n < N; ++n) {
            const float v = tap_value(sp + n * hw, t, n % 5 >= 2);
            const float p = softplus_fast(v) + 1e-6f;
            den += p;
            num += fp[n * a.fsn] * p;
            if (n < LOSS_NCH) adj[n * P + pix] = sigmoid_fast(v);
        }
        const float d = num / den;
        const int64_t gi = (b * H + Y) * W + X;
        const bool owned = (unsigned)(Y / S - j0) < (unsigned)TY && (unsigned)(X / S - i0) < (unsigned)TX;
        const float g = pixel_loss(a, gi, d, kf, owned, lsum);
        if (owned && pred) pred[gi] = d;
        gS[q] = g / den;
        dd[q] = d;
        if (grad) {
            for (int n = 0; n < nch0; ++n) {
                const float fm = N == 1 ? 0.f : fp[n * a.fsn] - d;   // one slice: d is f itself, the head has no gradient
                adj[n * P + pix] = (gS[q] * fm) * adj[n * P + pix];
            }
        }
    }
    lsum = block_sum_256(lsum, sh);
    if (tid == 0) partial[b * gridDim.x + blockIdx.x] = lsum;
    if (!grad) return;
    for (int c0 = 0; c0 < N; c0 += LOSS_NCH) {
        const int nc = N - c0 < LOSS_NCH ? N - c0 : LOSS_NCH;
        if (c0 > 0) {   // slices beyond the LDS plan: v_n and sigmoid(v_n) once more (pixels outside the image keep the zeros of the first chunk)
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int pix = q * 256 + tid;
                if (pix >= P) continue;
                const int ry = pix / RW, rx = pix - ry * RW, Y = Y0 + ry, X = X0 + rx;
                if (Y < 0 || Y >= H || X < 0 || X >= W) continue;
                const Taps t = make_taps(X, Y, h, w, sch, scw);
                const float *__restrict__ fp = a.fd + b * a.fsb + Y * a.fsh + X * a.fsw;
                for (int k = 0; k < nc; ++k) {
                    const int n = c0 + k;
                    const float v = tap_value(sp + n * hw, t, k % 5 >= 2);
                    adj[k * P + pix] = (gS[q] * (fp[n * a.fsn] - dd[q])) * sigmoid_fast(v);
                }
            }
        }
        __syncthreads();
        // x: the 2S footprint columns of element column i0 + tx, left to right
        for (int item = tid; item < nc * (RH * TX); item += 256) {
            const int k = item / (RH * TX), rem = item - k * (RH * TX), ry = rem / TX, tx = rem - ry * TX;
            const float *row = adj + k * P + ry * RW + S * tx;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 2 * S; ++e) s = __builtin_fmaf(tap_weight(X0 + S * tx + e, i0 + tx, w, scw), row[e], s);
            tmp[item] = s;
        }
        __syncthreads();
        // y: the 2S footprint rows of element row j0 + ty, top to bottom
        for (int item = tid; item < nc * (TY * TX); item += 256) {
            const int k = item / (TY * TX), rem = item - k * (TY * TX), ty = rem / TX, tx = rem - ty * TX;
            const int j = j0 + ty, i = i0 + tx;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 2 * S; ++e) s = __builtin_fmaf(tap_weight(Y0 + S * ty + e, j, h, sch), tmp[(k * RH + S * ty + e) * TX + tx], s);
            if (j < h && i < w) grad[(b * N + c0 + k) * hw + (int64_t)j * w + i] = s;
        }
    }
}

// ---- full-resolution head (h == H): pointwise, the upsample is the identity ----
__global__ __launch_bounds__(256) void loss_head_full_kernel(const LossArgs a, const float *__restrict__ score, float *__restrict__ pred,
                                                              float *__restrict__ grad, const double *__restrict__ Zp, double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    const int N = a.N;
    const int64_t hw = (int64_t)a.H * a.W, total = hw * a.B;
    const float kf = (float)(a.scale / *Zp);
    double lsum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw, q = i - b * hw;
        const int Y = (int)(q / a.W), X = (int)(q - (int64_t)Y * a.W);
        const float *__restrict__ sp = score + b * N * hw + q;
        const float *__restrict__ fp = a.fd + b * a.fsb + Y * a.fsh + X * a.fsw;
        float num = 0.f, den = 0.f;
        for (int n = 0; n < N; ++n) {
            const float p = softplus_fast(sp[n * hw]) + 1e-6f;
            den += p;
            num += fp[n * a.fsn] * p;
        }
        const float d = num / den;
        const float g = pixel_loss(a, i, d, kf, true, lsum);
        if (pred) pred[i] = d;
        if (grad) {
            const float gs = g / den;
            float *__restrict__ gp = grad + b * N * hw + q;
            for (int n = 0; n < N; ++n) {
                const float fm = N == 1 ? 0.f : fp[n * a.fsn] - d;
                gp[n * hw] = (gs * fm) * sigmoid_fast(sp[n * hw]);
            }
        }
    }
    lsum = block_sum_256(lsum, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = lsum;
}

// ---- losses: per head sum_i c m (d - gt)^2 / (r^2 Z) from the workgroup partials (256 strided sums, then a fixed tree), then the weighted total ----
struct LossFinish {
    int n;
    int cnt[4];
    int64_t off[4];
    float w[4];
    double inv_r2;
};
__global__ __launch_bounds__(256) void loss_finish_kernel(const LossFinish f, const double *__restrict__ ws, double *__restrict__ losses) {
    __shared__ double sh[256];
    __shared__ double lk[4];
    const int tid = threadIdx.x;
    const double Z = ws[0];
    for (int k = 0; k < f.n; ++k) {
        const double *p = ws + f.off[k];
        double v = 0.0;
        for (int i = tid; i < f.cnt[k]; i += 256) v += p[i];
        sh[tid] = v;
        __syncthreads();
        for (int o = 128; o; o >>= 1) {
            if (tid < o) sh[tid] += sh[tid + o];
            __syncthreads();
        }
        if (tid == 0) lk[k] = sh[0] * f.inv_r2 / Z;
        __syncthreads();
    }
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < f.n; ++k) {
            losses[k] = lk[k];
            t += (double)f.w[k] * lk[k];
        }
        losses[f.n] = t;
    }
}

// loss partials (= workgroups) of a head at scale s
static int64_t head_partials(int s, int B, int H, int W) {
    if (s == 1) return std::min<int64_t>(LOSS_FULL_BLKS, ((int64_t)B * H * W + 255) / 256);
    return (int64_t)B * tile_count(s, H / s, W / s);
}

template <int S>
static void launch_tile(const LossArgs &a, const float *score, int h, int w, float *pred, float *grad, const double *Z, double *partial, hipStream_t s) {
    hipLaunchKernelGGL((loss_head_tile_kernel<S, LossTile<S>::TY, LossTile<S>::TX>), dim3((unsigned)tile_count(S, h, w), (unsigned)a.B), dim3(256), 0, s,
                       a, score, h, w, pred, grad, Z, partial);
}

}  // namespace dffw

using namespace dffw;

#define LOSS_HIPCHK(x)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return dffw_fail(DFFW_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

extern "C" {

int64_t dffw_loss_workspace_bytes(int B, int N, int H, int W) {
    if (B < 1 || N < 1 || H < 1 || W < 1) return 0;
    int64_t most = 0;   // any of the four heads may have any of the four scales
    for (int s = 1; s <= 8; s *= 2)
        if (H % s == 0 && W % s == 0) most = std::max(most, head_partials(s, B, H, W));
    return (1 + LOSS_NORM_BLKS + 4 * most) * (int64_t)sizeof(double);
}

int dffw_loss_heads(int device, int n_heads, const float *const score[4], const int h[4], const int w[4], int B, int N, int H, int W,
                    const float *focus_dists, const int64_t fd_strides[4], const float *gt, const uint8_t *mask, const float *conf,
                    const float weights[4], int use_range, float lo, float hi, float *const pred[4], float *const grad[4], double *losses,
                    void *workspace, int64_t workspace_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (n_heads < 1 || n_heads > 4) return dffw_fail(DFFW_EINVAL, "n_heads %d not in 1..4", n_heads);
    if (!score || !h || !w || !focus_dists || !fd_strides || !gt || !mask || !weights || !losses || !workspace)
        return dffw_fail(DFFW_EINVAL, "null argument");
    if (B < 1 || N < 1 || H < 1 || W < 1) return dffw_fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (B > 65535) return dffw_fail(DFFW_EINVAL, "B=%d: at most 65535 samples per call", B);
    if ((int64_t)H * W >= (1ll << 31)) return dffw_fail(DFFW_EINVAL, "H*W = %lld does not fit 31 bits", (long long)H * W);
    int scale[4];
    for (int k = 0; k < n_heads; ++k) {
        if (!score[k]) return dffw_fail(DFFW_EINVAL, "score[%d] is null", k);
        scale[k] = h[k] > 0 && w[k] > 0 ? head_scale(H, W, h[k], w[k]) : 0;
        if (!scale[k]) return dffw_fail(DFFW_EINVAL, "head %d: %dx%d is not %dx%d divided by 1, 2, 4 or 8", k, h[k], w[k], H, W);
    }
    double inv_r2 = 1.0;
    if (use_range) {
        const double r = (double)hi - (double)lo;
        if (!(r != 0.0) || !std::isfinite(r)) return dffw_fail(DFFW_EINVAL, "depth range (%g, %g) is empty", (double)lo, (double)hi);
        inv_r2 = 1.0 / (r * r);
    }
    if (workspace_bytes < dffw_loss_workspace_bytes(B, N, H, W)) return dffw_fail(DFFW_ENOMEM, "loss workspace too small");
    LOSS_HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    double *ws = (double *)workspace;   // [0] Z, [1 .. LOSS_NORM_BLKS] its block partials, then the loss partials head by head
    const int64_t total = (int64_t)B * H * W;
    const int nblk = (int)std::min<int64_t>(LOSS_NORM_BLKS, (total + 255) / 256);
    std::string names = "dffw::loss_norm_partial;dffw::loss_norm_finish";
    hipLaunchKernelGGL(loss_norm_partial_kernel, dim3(nblk), dim3(256), 0, s, mask, conf, total, ws + 1);
    hipLaunchKernelGGL(loss_norm_finish_kernel, dim3(1), dim3(64), 0, s, (const double *)(ws + 1), nblk, ws);
    LOSS_HIPCHK(hipGetLastError());
    LossFinish fin{};
    fin.n = n_heads;
    fin.inv_r2 = inv_r2;
    int64_t off = 1 + LOSS_NORM_BLKS;
    for (int k = 0; k < n_heads; ++k) {
        LossArgs a{focus_dists, fd_strides[0], fd_strides[1], fd_strides[2], fd_strides[3], gt, mask, conf, B, N, H, W,
                   2.0 * (double)weights[k] * inv_r2};
        float *pk = pred ? pred[k] : nullptr, *gk = grad ? grad[k] : nullptr;
        fin.off[k] = off;
        fin.cnt[k] = (int)head_partials(scale[k], B, H, W);
        fin.w[k] = weights[k];
        switch (scale[k]) {
            case 1:
                hipLaunchKernelGGL(loss_head_full_kernel, dim3((unsigned)fin.cnt[k]), dim3(256), 0, s, a, score[k], pk, gk, (const double *)ws, ws + off);
                names += ";dffw::loss_head_full";
                break;
            case 2: launch_tile<2>(a, score[k], h[k], w[k], pk, gk, ws, ws + off, s); names += ";dffw::loss_head_tile<2>"; break;
            case 4: launch_tile<4>(a, score[k], h[k], w[k], pk, gk, ws, ws + off, s); names += ";dffw::loss_head_tile<4>"; break;
            default: launch_tile<8>(a, score[k], h[k], w[k], pk, gk, ws, ws + off, s); names += ";dffw::loss_head_tile<8>"; break;
        }
        LOSS_HIPCHK(hipGetLastError());
        off += fin.cnt[k];
    }
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, fin, (const double *)ws, losses);
    LOSS_HIPCHK(hipGetLastError());
    names += ";dffw::loss_finish";
    dffw_set_last_op_kernels(names.c_str());
    return DFFW_OK;
}

}  // extern "C"
