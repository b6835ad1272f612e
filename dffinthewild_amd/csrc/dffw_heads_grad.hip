// Backward of the four regression heads (Depth_Estimation_Network.py:89-98, 118-134) under ANY upstream gradient: the node behind
// pipeline.regress_heads, whose depth maps a caller's own PyTorch loss differentiates.
//
//   v_n = bilinear(score_k[b,n], i)   p_n = softplus(v_n) + 1e-6   S = sum_n p_n   d_k = sum_n f_n p_n / S      (the forward heads)
//   dL/dv_n(i) = gp(i) * (f_n - d_k)/S * sigmoid(v_n),  gp = dL/dd_k;  dL/dscore_k = upsample^T(dL/dv)
//
// The gather-form adjoint of dffw_loss.hip with the loss bracket replaced by gp: a workgroup owns a tile of the low-resolution grid,
// evaluates every output pixel of the tile's footprint once, parks the per-slice adjoints in LDS and sums each element's 2s x 2s
// contributors separably in a fixed order.  No mask, gt, conf, Z, loss partials or finish kernel; no atomics, no workspace: one launch
// per head, and two calls give identical bits.  The full-resolution head is pointwise.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/dffw.h"
#include "dffw_device.h"
#include "dffw_heads.h"
#include "dffw_internal.h"

namespace dffw {

constexpr int HEADS_GRAD_FULL_BLKS = 2048;   // persistent grid of the pointwise head

struct HeadsGradArgs {
    const float *fd;
    int64_t fsb, fsn, fsh, fsw;
    int B, N, H, W;
};

// ---- upsampled heads (s = 2, 4, 8): grid (tiles of TY x TX low-resolution elements, B); tiles, footprint and order of loss_head_tile_kernel ----
template <int S, int TY, int TX>
__global__ __launch_bounds__(256) void heads_grad_tile_kernel(const HeadsGradArgs a, const float *__restrict__ score, int h, int w,
                                                               const float *__restrict__ gpred, float *__restrict__ grad) {
#pragma clang fp contract(off)
    constexpr int RH = S * TY + S, RW = S * TX + S, P = RH * RW, Q = (P + 255) / 256;
    static_assert(Q <= 4, "at most four footprint pixels per thread");
    __shared__ float adj[LOSS_NCH * P];        // [slice of the chunk][footprint pixel]: sigmoid(v_n), then dL/dv_n
    __shared__ float tmp[LOSS_NCH * RH * TX];  // [slice][footprint row][element column]: the x-sums
    const int tid = threadIdx.x;
    const int tiles_x = (w + TX - 1) / TX;
    const int tj = blockIdx.x / tiles_x, ti = blockIdx.x - tj * tiles_x;
    const int64_t b = blockIdx.y;
    const int j0 = tj * TY, i0 = ti * TX, Y0 = S * j0 - S / 2, X0 = S * i0 - S / 2;
    const int N = a.N, H = a.H, W = a.W;
    const int64_t hw = (int64_t)h * w;
    const float *__restrict__ sp = score + b * N * hw;
    const float sch = (float)h / (float)H, scw = (float)w / (float)W;
    const int nch0 = N < LOSS_NCH ? N : LOSS_NCH;
    float gS[Q], dd[Q];
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
        gS[q] = gpred[(b * H + Y) * W + X] / den;
        dd[q] = d;
        for (int n = 0; n < nch0; ++n) {
            const float fm = N == 1 ? 0.f : fp[n * a.fsn] - d;   // one slice: d is f itself, the head has no gradient
            adj[n * P + pix] = (gS[q] * fm) * adj[n * P + pix];
        }
    }
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
__global__ __launch_bounds__(256) void heads_grad_full_kernel(const HeadsGradArgs a, const float *__restrict__ score, const float *__restrict__ gpred,
                                                               float *__restrict__ grad) {
#pragma clang fp contract(off)
    const int N = a.N;
    const int64_t hw = (int64_t)a.H * a.W, total = hw * a.B;
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
        const float gs = gpred[i] / den;
        float *__restrict__ gp = grad + b * N * hw + q;
        for (int n = 0; n < N; ++n) {
            const float fm = N == 1 ? 0.f : fp[n * a.fsn] - d;
            gp[n * hw] = (gs * fm) * sigmoid_fast(sp[n * hw]);
        }
    }
}

template <int S>
static void launch_grad_tile(const HeadsGradArgs &a, const float *score, int h, int w, const float *gpred, float *grad, hipStream_t s) {
    hipLaunchKernelGGL((heads_grad_tile_kernel<S, LossTile<S>::TY, LossTile<S>::TX>), dim3((unsigned)tile_count(S, h, w), (unsigned)a.B), dim3(256), 0, s,
                       a, score, h, w, gpred, grad);
}

}  // namespace dffw

using namespace dffw;

extern "C" {

int dffw_heads_backward(int device, int n_heads, const float *const score[4], const int h[4], const int w[4], int B, int N, int H, int W,
                        const float *focus_dists, const int64_t fd_strides[4], const float *const grad_pred[4], float *const grad_score[4],
                        void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (n_heads < 1 || n_heads > 4) return dffw_fail(DFFW_EINVAL, "n_heads %d not in 1..4", n_heads);
    if (!score || !h || !w || !focus_dists || !fd_strides || !grad_pred || !grad_score) return dffw_fail(DFFW_EINVAL, "null argument");
    if (B < 1 || N < 1 || H < 1 || W < 1) return dffw_fail(DFFW_EINVAL, "bad shape B=%d N=%d H=%d W=%d", B, N, H, W);
    if (B > 65535) return dffw_fail(DFFW_EINVAL, "B=%d: at most 65535 samples per call", B);
    if ((int64_t)H * W >= (1ll << 31)) return dffw_fail(DFFW_EINVAL, "H*W = %lld does not fit 31 bits", (long long)H * W);
    int scale[4];
    for (int k = 0; k < n_heads; ++k) {
        if (!score[k]) return dffw_fail(DFFW_EINVAL, "score[%d] is null", k);
        scale[k] = h[k] > 0 && w[k] > 0 ? head_scale(H, W, h[k], w[k]) : 0;
        if (!scale[k]) return dffw_fail(DFFW_EINVAL, "head %d: %dx%d is not %dx%d divided by 1, 2, 4 or 8", k, h[k], w[k], H, W);
        if (!grad_pred[k] != !grad_score[k]) return dffw_fail(DFFW_EINVAL, "head %d: grad_pred and grad_score are both given or both null", k);
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return dffw_fail(DFFW_EHIP, "hipSetDevice: %s", hipGetErrorString(e));
    hipStream_t s = (hipStream_t)hip_stream;
    const HeadsGradArgs a{focus_dists, fd_strides[0], fd_strides[1], fd_strides[2], fd_strides[3], B, N, H, W};
    std::string names;
    for (int k = 0; k < n_heads; ++k) {
        if (!grad_pred[k]) continue;   // a head without a gradient: skipped
        const char *name;
        switch (scale[k]) {
            case 1: {
                const int64_t blks = ((int64_t)B * H * W + 255) / 256;
                hipLaunchKernelGGL(heads_grad_full_kernel, dim3((unsigned)(blks < HEADS_GRAD_FULL_BLKS ? blks : HEADS_GRAD_FULL_BLKS)), dim3(256), 0, s, a,
                                   score[k], grad_pred[k], grad_score[k]);
                name = "dffw::heads_grad_full";
                break;
            }
            case 2: launch_grad_tile<2>(a, score[k], h[k], w[k], grad_pred[k], grad_score[k], s); name = "dffw::heads_grad_tile<2>"; break;
            case 4: launch_grad_tile<4>(a, score[k], h[k], w[k], grad_pred[k], grad_score[k], s); name = "dffw::heads_grad_tile<4>"; break;
            default: launch_grad_tile<8>(a, score[k], h[k], w[k], grad_pred[k], grad_score[k], s); name = "dffw::heads_grad_tile<8>"; break;
        }
        e = hipGetLastError();
        if (e != hipSuccess) return dffw_fail(DFFW_EHIP, "%s: %s", name, hipGetErrorString(e));
        names += names.empty() ? "" : ";";
        names += name;
    }
    dffw_set_last_op_kernels(names.c_str());
    return DFFW_OK;
}

}  // extern "C"
