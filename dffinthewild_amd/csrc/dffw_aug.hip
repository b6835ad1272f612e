// Training-sample assembly: what the reference's five training loaders do to a decoded sample between the
// decode and the loss (train_codes/train_Dataloader.py with train_codes/augmentation.py) -- random crop, the photometric
// chain image_augmentation (contrast, brightness, clamp, gamma, clamp, /0.5 - 1), horizontal flip, vertical flip, rot90, the
// ground-truth range rule with its validity mask, and the transpose to (3,N,h,w) float32 -- as two streaming kernels on the
// caller's stream.  Bandwidth-bound: 3 B (uint8) or 12 B (float32) in and 12 B out per pixel and channel triple.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

#include "../../include/dffw.h"
#include "dffw_internal.h"

// NumPy multiplies, then adds: nothing in this file may be contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace dffw {

// ---- pose ---------------------------------------------------------------------------------------------------------------
// Output pixel (i, j) of a sample reads window pixel (y, x) = (yi*i + yj*j + y0, xi*i + xj*j + x0): the composition of
// np.flip(axis 1) if flip_x, np.flip(axis 0) if flip_y and np.rot90(k) in the loaders' order, inverted.  One of the two
// coefficients of each line is 0 and the other +-1: eight poses, a signed permutation plus offset.
struct Pose {
    int yi, yj, y0, xi, xj, x0;
    int tr;   // 1: the pose transposes (odd k): output is (w, h)
};

// p: the sample's record (DFFW_AUG_* doubles).  (h, w): window size.  transposed: the parity the host sized the output for; where
// h != w it overrides the record's (the output has one shape per batch), so no coordinate can leave the window.
__device__ __forceinline__ Pose make_pose(const double *p, int h, int w, int transposed) {
    int k = (int)p[DFFW_AUG_ANGLE] & 3;
    if (h != w) k = (k & 2) | (transposed ? 1 : 0);
    const bool fx = p[DFFW_AUG_FLIP_X] > 0.5, fy = p[DFFW_AUG_FLIP_Y] > 0.5;
    Pose q;
    // np.rot90(a, k)[i][j]:  k=0 a[i][j]   k=1 a[j][w-1-i]   k=2 a[h-1-i][w-1-j]   k=3 a[h-1-j][i]
    q.tr = k & 1;
    q.yi = k == 0 ? 1 : (k == 2 ? -1 : 0);
    q.yj = k == 1 ? 1 : (k == 3 ? -1 : 0);
    q.y0 = (k == 2 || k == 3) ? h - 1 : 0;
    q.xi = k == 3 ? 1 : (k == 1 ? -1 : 0);
    q.xj = k == 0 ? 1 : (k == 2 ? -1 : 0);
    q.x0 = (k == 1 || k == 2) ? w - 1 : 0;
    if (fy) {   // the vertical flip precedes the rotation: y -> h-1-y
        q.yi = -q.yi;
        q.yj = -q.yj;
        q.y0 = h - 1 - q.y0;
    }
    if (fx) {
        q.xi = -q.xi;
        q.xj = -q.xj;
        q.x0 = w - 1 - q.x0;
    }
    return q;
}

// crop origin of the record, clamped so that the window lies inside the source whatever the record holds
__device__ __forceinline__ void crop_origin(const double *p, int H, int W, int h, int w, int *Y0, int *X0) {
    *Y0 = min(max((int)p[DFFW_AUG_Y0], 0), H - h);
    *X0 = min(max((int)p[DFFW_AUG_X0], 0), W - w);
}

// ---- photometric chain (augmentation.py:4-15), one IEEE operation per NumPy operation ---------------------------------------
// np.power is the one transcendental: evaluated in double in both chains (float32 chain: operands are the float32 values,
// the double result is rounded once).  gamma == 1 returns the base itself, as a correctly rounded pow does.
// (not inlined: its ~30 scalar constants would otherwise stay live across the tile loop beside the strides and the pose)
__device__ __attribute__((noinline)) double pow_f64(double x, double g) { return pow(x, g); }

template <bool NORM64>
struct Chain {
    using F = typename std::conditional<NORM64, double, float>::type;   // the seeds enter a float32 chain as float32 values
    F c, b, g;
    __device__ __forceinline__ explicit Chain(const double *p) : c((F)p[DFFW_AUG_CONTRAST]), b((F)p[DFFW_AUG_BRIGHTNESS]), g((F)p[DFFW_AUG_GAMMA]) {}
    __device__ __forceinline__ float operator()(float v) const {
        // plain operators under this file's `fp contract(off)`: the __fmul_rn / __fadd_rn wrappers are inlined from a header compiled
        // with contraction allowed, and their multiply and add were fused into one v_fma_f32 here
        if constexpr (NORM64) {
            double x = (double)v / 255.0;
            x = (0.5 + c * (x - 0.5)) + b;
            x = fmax(fmin(x, 1.0), 0.0);
            if (g != 1.0) x = pow_f64(x, g);
            x = fmax(fmin(x, 1.0), 0.0);
            return (float)(x / 0.5 - 1.0);
        } else {
            float x = v / 255.0f;
            x = (0.5f + c * (x - 0.5f)) + b;
            x = fmaxf(fminf(x, 1.0f), 0.0f);
            if (g != 1.0f) x = (float)pow_f64((double)x, (double)g);
            x = fmaxf(fminf(x, 1.0f), 0.0f);
            return x / 0.5f - 1.0f;
        }
    }
};

// ---- stack kernel -------------------------------------------------------------------------------------------------------
// Gather through LDS.  A workgroup owns sample blockIdx.y and walks tiles of AUG_TH x AUG_TW OUTPUT pixels of one slice, all
// three channels.  Per tile it (1) reads the tile's source rectangle row by row in SOURCE order (for interleaved-RGB sources
// consecutive lanes read consecutive bytes, whatever the pose) into LDS, (2) writes the output rows as 16-byte stores, each lane
// looking its four pixels up in LDS through the pose.  For the four transposing poses the LDS walk of a lane is down a column.
//   uint8 source: LDS holds the raw bytes; the chain is the sample's 256-entry float table, built once per workgroup (256 pows
//                 instead of one per element).   float32 source: LDS holds the chain's result, computed per element after loading.
// LDS pitch: one source row of the rectangle is 3*AUG_TW (not transposing) or 3*AUG_TH (transposing) elements.  A lane's four
// pixels sit in four successive rows on a transposing pose, so the 16 lanes of an output row step 4 pitches each: the pitch is the
// row length plus one dword (uint8: +4 bytes -> 49 or 25 dwords; float: +1 element -> 193 or 97 dwords), an ODD number of dwords, which
// spreads lanes * 4 * pitch over all 64 banks of the LDS (MI355X: 64 banks x 4 B) instead of folding them onto 16 (even pitch 24 / 48: 8).
constexpr int AUG_TH = 32, AUG_TW = 64;
constexpr int AUG_ROW = 3 * AUG_TW, AUG_ROW_T = 3 * AUG_TH;                                  // elements of a source row: 192, 96
template <typename T>
constexpr int aug_pad() { return sizeof(T) == 1 ? 4 : 1; }
template <typename T>
constexpr int aug_lds_elems() {
    return (AUG_TH * (AUG_ROW + aug_pad<T>()) > AUG_TW * (AUG_ROW_T + aug_pad<T>())) ? AUG_TH * (AUG_ROW + aug_pad<T>()) : AUG_TW * (AUG_ROW_T + aug_pad<T>());
}

template <typename T, bool NORM64>
__global__ __launch_bounds__(256) void augment_stack_kernel(const T *__restrict__ raw, int64_t sb, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int N,
                                                             int H, int W, int h, int w, const double *__restrict__ params, int transposed,
                                                             float *__restrict__ out) {
    constexpr bool U8 = sizeof(T) == 1;
    using L = typename std::conditional<U8, uint8_t, float>::type;
    __shared__ __attribute__((aligned(16))) L tile[aug_lds_elems<T>()];
    __shared__ float table[U8 ? 256 : 1];
    const int b = blockIdx.y, t = threadIdx.x;
    const double *p = params + (int64_t)b * DFFW_AUG_NPARAMS;
    const Chain<NORM64> chain(p);
    const Pose q = make_pose(p, h, w, transposed);
    int Y0, X0;
    crop_origin(p, H, W, h, w, &Y0, &X0);
    if constexpr (U8) {
        table[t] = chain((float)t);
        __syncthreads();
    }
    const int oh = transposed ? w : h, ow = transposed ? h : w;   // == the pose's own shape (make_pose forces the parity where h != w)
    const int tiles_x = (ow + AUG_TW - 1) / AUG_TW, tiles_y = (oh + AUG_TH - 1) / AUG_TH;
    const int ntiles = N * tiles_y * tiles_x;
    const int rowlen = q.tr ? AUG_ROW_T : AUG_ROW, pitch = rowlen + aug_pad<T>();
    const bool vec = (ow & 3) == 0;
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int tx = tl % tiles_x, ty = (tl / tiles_x) % tiles_y, n = tl / (tiles_x * tiles_y);
        const int i0 = ty * AUG_TH, j0 = tx * AUG_TW;
        const int th = min(AUG_TH, oh - i0), tw = min(AUG_TW, ow - j0);
        // source rectangle of the tile (window coordinates): its corners are the images of the tile's corners
        const int ya = q.yi * i0 + q.yj * j0 + q.y0, yb = q.yi * (i0 + th - 1) + q.yj * (j0 + tw - 1) + q.y0;
        const int xa = q.xi * i0 + q.xj * j0 + q.x0, xb = q.xi * (i0 + th - 1) + q.xj * (j0 + tw - 1) + q.x0;
        const int ys0 = min(ya, yb), xs0 = min(xa, xb);
        const int shh = q.tr ? tw : th, sww3 = 3 * (q.tr ? th : tw);
        const T *src = raw + (int64_t)b * sb + (int64_t)n * sn + (int64_t)(Y0 + ys0) * sy + (int64_t)(X0 + xs0) * sx;
        // (1) source rows -> LDS, element order (row, col, channel)
        for (int e = t; e < AUG_TH * AUG_ROW; e += 256) {
            const int r = q.tr ? e / AUG_ROW_T : e / AUG_ROW;
            const int rem = e - r * rowlen;
            if (r < shh && rem < sww3) {
                const int col = rem / 3, c = rem - 3 * col;
                const T v = src[(int64_t)r * sy + (int64_t)col * sx + (int64_t)c * sc];
                tile[r * pitch + rem] = v;
            }
        }
        __syncthreads();
        if constexpr (!U8) {
            // the chain in place, in a loop of its own: all loads of the tile are in flight before the first pow, and the pow's
            // constants do not compete with the addressing for scalar registers (pad and unused elements are transformed too: harmless)
            for (int e = t; e < shh * pitch; e += 256) tile[e] = chain(tile[e]);
            __syncthreads();
        }
        // (2) output rows: lane -> 4 pixels of one (channel, row)
        const int dy = q.yj * pitch, dx = q.xj * 3;   // LDS step per output column
        for (int o = t; o < 3 * AUG_TH * (AUG_TW / 4); o += 256) {
            const int lj = (o % (AUG_TW / 4)) * 4, li = (o / (AUG_TW / 4)) % AUG_TH, c = o / (AUG_TH * (AUG_TW / 4));
            if (li >= th || lj >= tw) continue;
            const int i = i0 + li, j = j0 + lj;
            const int a = (q.yi * i + q.yj * j + q.y0 - ys0) * pitch + (q.xi * i + q.xj * j + q.x0 - xs0) * 3 + c;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = 0.f;
                if (lj + k < tw) {
                    if constexpr (U8) v[k] = table[tile[a + k * (dy + dx)]];
                    else v[k] = tile[a + k * (dy + dx)];
                }
            }
            float *dst = out + ((((int64_t)b * 3 + c) * N + n) * oh + i) * ow + j;
            if (vec) {
                *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lj + k < tw) dst[k] = v[k];
            }
        }
        __syncthreads();
    }
}

// ---- label kernel -------------------------------------------------------------------------------------------------------
// gt / conf (B,H,W) float32 -> the window in the sample's pose; values < lo or > hi become the sentinel (float32 comparisons, as NumPy
// compares a float32 array with a Python float); mask = (gt != sentinel), so NaN counts as valid like np.where(gt == s, 0., 1.).
// Pure data movement; one thread per output pixel, sample = blockIdx.y.
__global__ __launch_bounds__(256) void augment_labels_kernel(const float *__restrict__ gt, const float *__restrict__ conf, int H, int W, int h, int w,
                                                              const double *__restrict__ params, int transposed, int use_range, float lo, float hi,
                                                              float sentinel, float *__restrict__ gt_out, uint8_t *__restrict__ mask_out,
                                                              float *__restrict__ conf_out) {
    const int b = blockIdx.y;
    const double *p = params + (int64_t)b * DFFW_AUG_NPARAMS;
    const Pose q = make_pose(p, h, w, transposed);
    int Y0, X0;
    crop_origin(p, H, W, h, w, &Y0, &X0);
    const int ow = transposed ? h : w;
    const int hw = h * w;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < hw; o += gridDim.x * 256) {
        const int i = o / ow, j = o - i * ow;
        const int64_t s = (int64_t)b * H * W + (int64_t)(Y0 + q.yi * i + q.yj * j + q.y0) * W + (X0 + q.xi * i + q.xj * j + q.x0);
        const int64_t d = (int64_t)b * hw + o;
        if (gt) {
            float v = gt[s];
            if (use_range && (v < lo || v > hi)) v = sentinel;
            gt_out[d] = v;
            mask_out[d] = v != sentinel ? 1 : 0;
        }
        if (conf) conf_out[d] = conf[s];
    }
}

}  // namespace dffw

using namespace dffw;

extern "C" int dffw_augment_stack(int device, const void *raw, int dtype, const int64_t strides[5], int B, int N, int H, int W, int h, int w,
                                  const double *params, int transposed, float *FS, const float *gt, const float *conf, float *gt_out,
                                  uint8_t *mask_out, float *conf_out, int use_range, float lo, float hi, float sentinel, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!raw || !strides || !params || !FS) return dffw_fail(DFFW_EINVAL, "null argument");
    if ((gt && (!gt_out || !mask_out)) || (conf && !conf_out)) return dffw_fail(DFFW_EINVAL, "gt needs gt_out and mask_out, conf needs conf_out");
    const bool norm64 = (dtype & DFFW_RAW_NORM_F64) != 0;
    dtype &= ~DFFW_RAW_NORM_F64;
    if (dtype != DFFW_RAW_U8 && dtype != DFFW_RAW_F32) return dffw_fail(DFFW_EINVAL, "unknown raw dtype %d", dtype);
    if (B < 1 || N < 1 || h < 1 || w < 1 || h > H || w > W || B > 65535)
        return dffw_fail(DFFW_EINVAL, "window %dx%d must fit the %dx%d source (B=%d N=%d)", h, w, H, W, B, N);
    if ((int64_t)h * w > INT32_MAX / 4) return dffw_fail(DFFW_EINVAL, "window %dx%d too large", h, w);
    transposed = transposed ? 1 : 0;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return dffw_fail(DFFW_EHIP, "hipSetDevice -> %s", hipGetErrorString(e));
    hipStream_t s = (hipStream_t)hip_stream;
    const int oh = transposed ? w : h, ow = transposed ? h : w;
    const int64_t ntiles = (int64_t)N * ((oh + AUG_TH - 1) / AUG_TH) * ((ow + AUG_TW - 1) / AUG_TW);
    // about 8 workgroups per CU over the batch; a workgroup keeps its sample, so its table serves every tile it walks
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ntiles, (2048 + B - 1) / B));
#define DFFW_AUG(T, N64)                                                                                                                   \
    hipLaunchKernelGGL((augment_stack_kernel<T, N64>), dim3(gx, B), dim3(256), 0, s, (const T *)raw, strides[0], strides[1], strides[2], strides[3], \
                       strides[4], N, H, W, h, w, params, transposed, FS)
    const char *name;
    if (dtype == DFFW_RAW_U8) {
        if (norm64) DFFW_AUG(uint8_t, true);
        else DFFW_AUG(uint8_t, false);
        name = norm64 ? "dffw::augment_stack<u8,f64>" : "dffw::augment_stack<u8,f32>";
    } else {
        if (norm64) DFFW_AUG(float, true);
        else DFFW_AUG(float, false);
        name = norm64 ? "dffw::augment_stack<f32,f64>" : "dffw::augment_stack<f32,f32>";
    }
#undef DFFW_AUG
    if (gt || conf) {
        const unsigned lx = (unsigned)std::min<int64_t>(((int64_t)h * w + 255) / 256, 1024);
        hipLaunchKernelGGL(augment_labels_kernel, dim3(lx, B), dim3(256), 0, s, gt, conf, H, W, h, w, params, transposed, use_range, lo, hi, sentinel,
                           gt_out, mask_out, conf_out);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return dffw_fail(DFFW_EHIP, "augment launch -> %s", hipGetErrorString(e));
    char names[96];
    snprintf(names, sizeof names, "%s%s", name, (gt || conf) ? ";dffw::augment_labels" : "");
    dffw_set_last_op_kernels(names);
    return DFFW_OK;
}
