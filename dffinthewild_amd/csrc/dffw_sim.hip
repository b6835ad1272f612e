// dffw_sim.hip — the synthetic focal-stack simulator (Simulator/synthetic_blur_movement.py:155-280) on gfx950.
//
//   sim_minmax      per-sample min / max of the raw depth (float64) and status = 0
//   sim_plan        one thread per (b, n): the float64 scalars and the CoC layer table of the slice (sim_plan_slice, the same
//                   function dffw_sim_plan_host runs), written to the workspace: nothing returns to the host
//   sim_render<L>   per (b, n, 32x32 tile): layer lookup, defocus, depth_out / status (last slice), the warped-image tap, and the
//                   variable-radius disk blur.  L = true: the truncated warped image of the tile plus its halo is staged in LDS as
//                   per-row prefix sums (radius <= DFFW_SIM_LDS_RADIUS); a tile whose radius is larger, and every tile of
//                   L = false, sums its disks from global memory, warping each tap on the fly.
//
// The reference blurs the whole image once per CoC layer (cv2.filter2D) and keeps each pixel from the layer its unwarped depth
// falls in; here each output pixel gathers only its own layer's disk.  A disk row is one contiguous span, so with row prefix sums
// the sum over a radius-r disk costs 2r+1 differences, exact in integers.  DESIGN.md §10 has the contract.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/dffw.h"
#include "dffw_device.h"
#include "dffw_internal.h"

// Python / NumPy / torch evaluate every expression below one rounded operation at a time: no fused multiply-add anywhere in
// this file unless written as fmaf (the torch CPU kernels that do fuse: linspace, grid_sample's blend).
#pragma clang fp contract(off)

namespace dffw {

constexpr int SIM_TILE = 32;                       // output tile edge; one thread per output pixel
constexpr int SIM_RL = DFFW_SIM_LDS_RADIUS;
constexpr int SIM_EDGE = SIM_TILE + 2 * SIM_RL;    // staged rows of the largest halo
constexpr int SIM_PITCH = SIM_EDGE + 1;            // prefix-sum entries per staged row

// ---- host + device: scalars and CoC layer table of one slice (synthetic_blur_movement.py:173-244) ------------------------------
__host__ __device__ inline double sim_normalise(double d, double dmin, double dmax, double min_depth, double max_depth) {
    return max_depth * (d - dmin) / (dmax - dmin) + min_depth;   // :173-174
}

// Layer i of the table: [lo[i], hi[i]) blurred with radius |coc[i]|.  Returns the number of layers.  `sc` receives
// DFFW_SIM_NSCALARS values.  Python's left-to-right order throughout; round() is half-to-even (rint).
__host__ __device__ inline int sim_plan_slice(const dffw_sim_params &p, const double *cam, double dmin, double dmax, int N, int n,
                                              double *sc, int *coc, double *lo, double *hi) {
    const double ppm = p.pixel_per_meter;
    const double scene_min = sim_normalise(dmin, dmin, dmax, p.min_depth, p.max_depth);   // np.min / np.max of the normalised
    const double scene_max = sim_normalise(dmax, dmin, dmax, p.min_depth, p.max_depth);   // map: the normalisation is monotone
    const double f = cam[0] * ppm;                                                          // :178
    const double lens_dia = f / cam[1];
    // focus_dists = 1/np.linspace(1/max, 1/min, N): i*step + start, the last element = stop (:186)
    const double start = 1.0 / p.max_focus, stop = 1.0 / p.min_focus;
    const double step = (stop - start) / (double)(N - 1);
    const double y = n == N - 1 ? stop : (double)n * step + start;
    const double fd = 1.0 / y;
    const double fd_px = ppm * fd;                                                          // :207
    const double max_fd_px = p.max_focus * ppm, min_fd_px = p.min_focus * ppm;            // :189-194
    const double min_afov = 1.0 / (f * min_fd_px / (min_fd_px - f));
    const double max_afov = 1.0 / (f * max_fd_px / (max_fd_px - f));
    const double origin_max_afov = max_afov / min_afov + cam[2] * (1.0 / scene_max) + cam[3];
    const double lts = f * fd_px / (fd_px - f);                                             // :208
    double fov = 1.0;
    if (n != 0) {                                                                           // :209-214
        const double Fov = 1.0 / lts;
        const double alpha = cam[2] * (1.0 / fd) + cam[3];
        const double origin_fov = Fov / min_afov + alpha;
        fov = origin_max_afov / origin_fov;
    }
    const double coc_scale = lts * lens_dia / fd_px;                                        // :225
    sc[DFFW_SIM_FD] = fd;
    sc[DFFW_SIM_FD_PX] = fd_px;
    sc[DFFW_SIM_LENS_TO_SENSOR] = lts;
    sc[DFFW_SIM_FOV] = fov;
    sc[DFFW_SIM_COC_SCALE] = coc_scale;
    sc[DFFW_SIM_F_PX] = f;
    sc[DFFW_SIM_LENS_DIA] = lens_dia;
    sc[DFFW_SIM_SCENE_MIN] = scene_min;
    sc[DFFW_SIM_SCENE_MAX] = scene_max;
    sc[DFFW_SIM_MIN_AFOV] = min_afov;
    sc[DFFW_SIM_MAX_AFOV] = max_afov;
    sc[DFFW_SIM_ORIGIN_MAX_AFOV] = origin_max_afov;
    // :230-244: scan num_planes planes, merge runs of equal CoC; the last plane's upper edge grows by 0.1 only if it compares
    // equal to scene_max
    const int P = p.num_planes;
    int L = 0;
    for (int k = 0; k < P; ++k) {
        const double min_dis = (double)k / (double)P * (scene_max - scene_min) + scene_min;
        double max_dis = (double)(k + 1) / (double)P * (scene_max - scene_min) + scene_min;
        const double sub = min_dis + (max_dis - min_dis) / 2.0;
        const int c = (int)rint(coc_scale * (sub - fd) / sub);
        if (k > 0) {
            if (max_dis == scene_max) max_dis += 0.1;
            if (coc[L - 1] == c) {
                hi[L - 1] = max_dis;
                continue;
            }
        }
        coc[L] = c;
        if (lo) lo[L] = min_dis;
        hi[L] = max_dis;
        ++L;
    }
    return L;
}

// ---- host + device: the filled disk of cv2.circle(img, (r,r), r, 1, -1) (imgproc/drawing.cpp Circle(), restated in DESIGN.md) ---
// The midpoint walk fills rows +-dy over [-dx, dx] and rows +-dx over [-dy, dy]; a row's half-width is the widest fill.  Each
// step below emits every row exactly once: row dy at its only visit, and row dx at the last step with that dx if it is never
// visited as a dy (dx > dy then).  The device gather and dffw_sim_disk_rows both walk it, so a correction goes here only.
struct DiskWalk {
    int dx, dy, err, plus, minus;
    __host__ __device__ explicit DiskWalk(int r) : dx(r), dy(0), err(0), plus(1), minus(2 * r - 1) {}
    __host__ __device__ bool active() const { return dx >= dy; }
    // one step: row ya with half-width wa; row yb with half-width wb if yb >= 0
    __host__ __device__ void step(int &ya, int &wa, int &yb, int &wb) {
        const int x0 = dx, y0 = dy;
        ya = y0;
        wa = x0;
        ++dy;
        err += plus;
        plus += 2;
        const bool dec = err > 0;
        if (dec) {
            err -= minus;
            --dx;
            minus -= 2;
        }
        const bool last = dec || dx < dy;
        yb = (last && x0 > y0) ? x0 : -1;
        wb = y0;
    }
};

// cv2.borderInterpolate(p, len, BORDER_REFLECT_101) for any p: reflection is periodic with period 2(len-1)
__device__ __forceinline__ int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int T = 2 * (len - 1);
    int m = p % T;
    if (m < 0) m += T;
    return m < len ? m : T - m;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
struct SimSlice {          // per (b, n), written by sim_plan
    double dmin, dmax;     // raw depth range of the sample
    double fd, fd_px, coc_scale, scene_min;
    float fm1, beta, gamma;  // float32(FoV - 1), float32(beta), float32(gamma): the warp's torch scalars
    int nlayers, maxr;     // layers of the table; largest blur radius of the table
};

struct SimWs {
    double *mm;        // [B][2] raw depth min, max
    SimSlice *sl;      // [B*N]
    double *hi;        // [B*N][P]
    int *coc;          // [B*N][P]
};

__host__ __device__ inline int64_t sim_align(int64_t v) { return (v + 255) & ~(int64_t)255; }

static SimWs sim_carve(void *ws, int B, int N, int P, int64_t *total) {
    char *p = (char *)ws;
    SimWs w;
    int64_t o = 0;
    w.mm = (double *)(p + o);
    o += sim_align((int64_t)B * 2 * 8);
    w.sl = (SimSlice *)(p + o);
    o += sim_align((int64_t)B * N * sizeof(SimSlice));
    w.hi = (double *)(p + o);
    o += sim_align((int64_t)B * N * P * 8);
    w.coc = (int *)(p + o);
    o += sim_align((int64_t)B * N * P * 4);
    *total = o;
    return w;
}

__global__ __launch_bounds__(1024) void sim_minmax(const double *__restrict__ depth, int64_t hw, double *__restrict__ mm, int32_t *__restrict__ status) {
    const int b = blockIdx.x;
    const double *d = depth + (int64_t)b * hw;
    double lo = d[0], hi = d[0];
    for (int64_t i = threadIdx.x; i < hw; i += blockDim.x) {
        const double v = d[i];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    __shared__ double slo[1024], shi[1024];
    slo[threadIdx.x] = lo;
    shi[threadIdx.x] = hi;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            slo[threadIdx.x] = slo[threadIdx.x + s] < slo[threadIdx.x] ? slo[threadIdx.x + s] : slo[threadIdx.x];
            shi[threadIdx.x] = shi[threadIdx.x + s] > shi[threadIdx.x] ? shi[threadIdx.x + s] : shi[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mm[2 * b] = slo[0];
        mm[2 * b + 1] = shi[0];
        status[b] = 0;
    }
}

__global__ __launch_bounds__(64) void sim_plan(dffw_sim_params p, const double *__restrict__ cams, const double *__restrict__ shifts, int B, int N,
                                               SimWs w, double *__restrict__ slices) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * N) return;
    const int b = i / N, n = i % N;
    const double dmin = w.mm[2 * b], dmax = w.mm[2 * b + 1];
    double sc[DFFW_SIM_NSCALARS];
    const int P = p.num_planes;
    int *coc = w.coc + (int64_t)i * P;
    const int L = sim_plan_slice(p, cams + 4 * b, dmin, dmax, N, n, sc, coc, nullptr, w.hi + (int64_t)i * P);
    int maxr = 1;
    for (int l = 0; l < L; ++l) maxr = max(maxr, abs(coc[l]));
    SimSlice s;
    s.dmin = dmin;
    s.dmax = dmax;
    s.fd = sc[DFFW_SIM_FD];
    s.fd_px = sc[DFFW_SIM_FD_PX];
    s.coc_scale = sc[DFFW_SIM_COC_SCALE];
    s.scene_min = sc[DFFW_SIM_SCENE_MIN];
    s.fm1 = (float)(sc[DFFW_SIM_FOV] - 1.0);                     // (Fov - 1) in float64, a float32 scalar to torch
    s.beta = n ? (float)shifts[2 * i] : 0.0f;                    // 0-dim float64 tensors: float32 against the grid
    s.gamma = n ? (float)shifts[2 * i + 1] : 0.0f;
    s.nlayers = L;
    s.maxr = maxr;
    w.sl[i] = s;
    if (slices) {
        slices[2 * i] = sc[DFFW_SIM_FD];
        slices[2 * i + 1] = sc[DFFW_SIM_FOV];
    }
}

// grid_sample(bilinear, zeros, align_corners=True) as torch's CPU kernel computes it: weights from floor distances, then
// nw*v_nw + ne*v_ne + sw*v_sw + se*v_se with the last three accumulated by fused multiply-adds.  `get(y, x, v)` loads the C
// channels of an in-image pixel.
template <int C, typename Get>
__device__ __forceinline__ void sim_sample(const SimWarpPoint &wp, int H, int W, Get get, float (&out)[C]) {
    const float x0f = floorf(wp.sx), y0f = floorf(wp.sy);
    const float w = wp.sx - x0f, e = 1.0f - w, nn = wp.sy - y0f, s = 1.0f - nn;
    const float wt[4] = {s * e, s * w, nn * e, nn * w};   // nw ne sw se
    const bool vx[2] = {x0f >= 0.0f && x0f < (float)W, x0f + 1.0f >= 0.0f && x0f + 1.0f < (float)W};
    const bool vy[2] = {y0f >= 0.0f && y0f < (float)H, y0f + 1.0f >= 0.0f && y0f + 1.0f < (float)H};
    const int x0 = vx[0] || vx[1] ? (int)x0f : 0, y0 = vy[0] || vy[1] ? (int)y0f : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dy = k >> 1, dx = k & 1;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.0f;
        if (vy[dy] && vx[dx]) get(y0 + dy, x0 + dx, v);
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = k == 0 ? v[c] * wt[0] : fmaf(v[c], wt[k], out[c]);
    }
}

struct SimCtx {
    const float *img;      // (H,W,3) of sample b
    const double *depth;   // (H,W) of sample b
    int H, W, n;
    float fm1, beta, gamma;
};

// the float image slice n of the reference blurs before astype(uint8): the frame itself for n = 0, FOV_warp of it otherwise
__device__ __forceinline__ void sim_image_at(const SimCtx &c, int y, int x, float (&v)[3]) {
    if (c.n == 0) {
        const float *q = c.img + ((int64_t)y * c.W + x) * 3;
        v[0] = q[0];
        v[1] = q[1];
        v[2] = q[2];
        return;
    }
    const SimWarpPoint wp = sim_warp_point(x, y, c.H, c.W, c.fm1, c.beta, c.gamma);
    const float *img = c.img;
    const int W = c.W;
    sim_sample<3>(wp, c.H, c.W, [img, W](int yy, int xx, float (&v)[3]) {
        const float *q = img + ((int64_t)yy * W + xx) * 3;
        v[0] = q[0];
        v[1] = q[1];
        v[2] = q[2];
    }, v);
}

// the truncated uint8 value (astype(np.uint8)) of one channel triple
__device__ __forceinline__ void sim_trunc(const float (&v)[3], int (&u)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = (int)(uint8_t)(int)v[c];
}

template <bool LDS>
__global__ __launch_bounds__(1024) void sim_render(dffw_sim_params p, const float *__restrict__ image, const double *__restrict__ depth, int B, int N,
                                                   int H, int W, SimWs w, uint8_t *__restrict__ images, double *__restrict__ defocus,
                                                   float *__restrict__ depth_out, int32_t *__restrict__ status, float *__restrict__ warped_tap) {
    const int bn = blockIdx.z, b = bn / N, n = bn % N;
    const SimSlice sl = w.sl[bn];
    const int tx = threadIdx.x % SIM_TILE, ty = threadIdx.x / SIM_TILE;
    const int x0t = blockIdx.x * SIM_TILE, y0t = blockIdx.y * SIM_TILE;
    const int x = x0t + tx, y = y0t + ty;
    const bool inside = x < W && y < H;
    const int64_t hw = (int64_t)H * W;
    SimCtx c;
    c.img = image + (int64_t)b * hw * 3;
    c.depth = depth + (int64_t)b * hw;
    c.H = H;
    c.W = W;
    c.n = n;
    c.fm1 = sl.fm1;
    c.beta = sl.beta;
    c.gamma = sl.gamma;

    // layer of the pixel's unwarped normalised depth: the first layer whose hi exceeds it (the layers tile [scene_min, last hi));
    // none (black) at or beyond the last hi
    int r = 0;
    double dn = 0.0;
    if (inside) {
        dn = sim_normalise(c.depth[(int64_t)y * W + x], sl.dmin, sl.dmax, p.min_depth, p.max_depth);
        const double *hi = w.hi + (int64_t)bn * p.num_planes;
        int lo = 0, cnt = sl.nlayers;
        while (cnt > 0) {
            const int half = cnt >> 1;
            if (hi[lo + half] <= dn) {
                lo += half + 1;
                cnt -= half + 1;
            } else {
                cnt = half;
            }
        }
        if (lo < sl.nlayers && dn >= sl.scene_min) r = max(1, abs(w.coc[(int64_t)bn * p.num_planes + lo]));
    }

    // ---- defocus (:229), depth_out and status (:272-274), the warped-image tap ----
    if (inside) {
        const int64_t pix = (int64_t)bn * hw + (int64_t)y * W + x;
        const double ppm = p.pixel_per_meter;
        const double *dep = c.depth;
        const double dmin = sl.dmin, dmax = sl.dmax, mind = p.min_depth, maxd = p.max_depth;
        double dpn;
        SimWarpPoint wp{0.0f, 0.0f};
        if (n == 0) {
            dpn = dn * ppm;                 // depth_pixel, float64
        } else {
            wp = sim_warp_point(x, y, H, W, sl.fm1, sl.beta, sl.gamma);
            float v[1];
            sim_sample<1>(wp, H, W, [=](int yy, int xx, float (&o)[1]) {
                o[0] = (float)(sim_normalise(dep[(int64_t)yy * W + xx], dmin, dmax, mind, maxd) * ppm);
            }, v);
            dpn = (double)v[0];             // float32 warp, float64 arithmetic under NumPy 2 (see dffw.h)
        }
        defocus[pix] = fabs(sl.coc_scale * (dpn - sl.fd_px) / dpn);
        if (n == N - 1) {
            float v[1];
            sim_sample<1>(wp, H, W, [=](int yy, int xx, float (&o)[1]) {
                o[0] = (float)sim_normalise(dep[(int64_t)yy * W + xx], dmin, dmax, mind, maxd);
            }, v);
            depth_out[(int64_t)b * hw + (int64_t)y * W + x] = v[0];
            if (v[0] == 0.0f) atomicOr(status + b, DFFW_SIM_DISCARD);
        }
        if (warped_tap) {
            float v[3];
            sim_image_at(c, y, x, v);
            float *t = warped_tap + pix * 3;
            t[0] = v[0];
            t[1] = v[1];
            t[2] = v[2];
        }
    }

    // ---- the tile's radius ----
    __shared__ int s_r;
    if (threadIdx.x == 0) s_r = 0;
    __syncthreads();
    {
        int m = r;
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
        if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&s_r, m);
    }
    __syncthreads();
    const int R = s_r;
    if (R == 0) {   // every pixel of the tile is outside the image or black
        if (inside) {
            uint8_t *o = images + ((int64_t)bn * hw + (int64_t)y * W + x) * 3;
            o[0] = o[1] = o[2] = 0;
        }
        return;
    }

    int S[3] = {0, 0, 0};
    if (LDS && R <= SIM_RL) {
        // stage tile + halo (reflect-101 first, then the warp of the mapped pixel, then the uint8 truncation) as row prefix sums:
        // P[ch][row][0] = 0, P[ch][row][j+1] = sum of the first j+1 staged values (<= 97 * 255, fits uint16)
        __shared__ uint16_t P[3][SIM_EDGE][SIM_PITCH];
        const int rows = SIM_TILE + 2 * R, cols = SIM_TILE + 2 * R;
        for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) {
            const int row = i / cols, col = i % cols;
            const int sy = reflect101(y0t - R + row, H), sx = reflect101(x0t - R + col, W);
            float v[3];
            sim_image_at(c, sy, sx, v);
            int u[3];
            sim_trunc(v, u);
            P[0][row][col + 1] = (uint16_t)u[0];
            P[1][row][col + 1] = (uint16_t)u[1];
            P[2][row][col + 1] = (uint16_t)u[2];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * rows; i += blockDim.x) {
            uint16_t *q = &P[i / rows][i % rows][0];
            uint16_t acc = 0;
            q[0] = 0;
            for (int j = 1; j <= cols; ++j) {
                acc = (uint16_t)(acc + q[j]);
                q[j] = acc;
            }
        }
        __syncthreads();
        if (r > 0) {
            const int cx = tx + R, cy = ty + R;
            auto span = [&](int row, int h) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) S[ch] += (int)P[ch][row][cx + h + 1] - (int)P[ch][row][cx - h];
            };
            // lanes walk their own disks; the loop runs to the wave's largest radius with the finished lanes masked off
            DiskWalk dw(r);
            while (dw.active()) {
                int ya, wa, yb, wb;
                dw.step(ya, wa, yb, wb);
                span(cy + ya, wa);
                if (ya) span(cy - ya, wa);
                if (yb >= 0) {
                    span(cy + yb, wb);
                    span(cy - yb, wb);
                }
            }
        }
    } else if (r > 0) {
        // global-memory path: every tap is mapped, warped and truncated on its own
        auto span = [&](int row, int h) {
            const int sy = reflect101(y + row, H);
            for (int d = -h; d <= h; ++d) {
                float v[3];
                sim_image_at(c, sy, reflect101(x + d, W), v);
                int u[3];
                sim_trunc(v, u);
                S[0] += u[0];
                S[1] += u[1];
                S[2] += u[2];
            }
        };
        DiskWalk dw(r);
        while (dw.active()) {
            int ya, wa, yb, wb;
            dw.step(ya, wa, yb, wb);
            span(ya, wa);
            if (ya) span(-ya, wa);
            if (yb >= 0) {
                span(yb, wb);
                span(-yb, wb);
            }
        }
    }
    if (inside) {
        uint8_t *o = images + ((int64_t)bn * hw + (int64_t)y * W + x) * 3;
        if (r == 0) {
            o[0] = o[1] = o[2] = 0;
        } else {
            // the tap count K of radius r, then round(S/K) (K odd: never a tie); channels reversed (cvtColor BGR2RGB)
            int K = 0;
            DiskWalk dw(r);
            while (dw.active()) {
                int ya, wa, yb, wb;
                dw.step(ya, wa, yb, wb);
                K += (ya ? 2 : 1) * (2 * wa + 1) + (yb >= 0 ? 2 * (2 * wb + 1) : 0);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[2 - ch] = (uint8_t)((2 * S[ch] + K) / (2 * K));
        }
    }
}

}  // namespace dffw

using namespace dffw;

#define SIM_HIPCHK(expr)                                                                               \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return dffw_fail(DFFW_EHIP, "%s -> %s", #expr, hipGetErrorString(_e));   \
    } while (0)

extern "C" {

int64_t dffw_sim_workspace_bytes(int B, int N, int H, int W, int num_planes) {
    (void)H;
    (void)W;
    if (B < 1 || N < 1 || num_planes < 1) return 0;
    int64_t total;
    sim_carve(nullptr, B, N, num_planes, &total);
    return total;
}

int dffw_sim_plan_host(const dffw_sim_params *params, const double cam[4], double dmin, double dmax, int N, double *scalars, int *coc,
                       double *lo, double *hi, int *nlayers) {
    if (!params || !cam || !scalars || !coc || !lo || !hi || !nlayers) return dffw_fail(DFFW_EINVAL, "null argument");
    if (N < 2 || params->num_planes < 1) return dffw_fail(DFFW_EINVAL, "N = %d (>= 2), num_planes = %d (>= 1)", N, params->num_planes);
    const int P = params->num_planes;
    for (int n = 0; n < N; ++n)
        nlayers[n] = sim_plan_slice(*params, cam, dmin, dmax, N, n, scalars + (int64_t)n * DFFW_SIM_NSCALARS, coc + (int64_t)n * P,
                                    lo + (int64_t)n * P, hi + (int64_t)n * P);
    return DFFW_OK;
}

int dffw_sim_disk_rows(int r, int *halfwidths) {
    if (r < 0 || !halfwidths) return dffw_fail(DFFW_EINVAL, "radius %d", r);
    int K = 0;
    DiskWalk dw(r);
    while (dw.active()) {
        int ya, wa, yb, wb;
        dw.step(ya, wa, yb, wb);
        halfwidths[ya] = wa;
        K += (ya ? 2 : 1) * (2 * wa + 1);
        if (yb >= 0) {
            halfwidths[yb] = wb;
            K += 2 * (2 * wb + 1);
        }
    }
    return K;
}

int dffw_sim_render(int device, dffw_sim_params params, const double *cams, const float *image, const double *depth, const double *shifts,
                    int B, int N, int H, int W, uint8_t *images, double *defocus, float *depth_out, int32_t *status, double *slices,
                    float *warped_tap, void *workspace, int64_t ws_bytes, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!cams || !image || !depth || !shifts || !images || !defocus || !depth_out || !status || !workspace)
        return dffw_fail(DFFW_EINVAL, "null argument");
    if (B < 1 || N < 2 || H < 2 || W < 2) return dffw_fail(DFFW_EINVAL, "shape B=%d N=%d H=%d W=%d (N, H, W >= 2)", B, N, H, W);
    if ((int64_t)B * N > 65535) return dffw_fail(DFFW_EINVAL, "B*N = %lld exceeds 65535", (long long)B * N);
    if (params.num_planes < 1) return dffw_fail(DFFW_EINVAL, "num_planes = %d", params.num_planes);
    if (!(params.pixel_per_meter > 0) || !(params.min_focus > 0) || !(params.max_focus > 0))
        return dffw_fail(DFFW_EINVAL, "pixel_per_meter and the focus range must be positive");
    int64_t need;
    const SimWs w = sim_carve(workspace, B, N, params.num_planes, &need);
    if (ws_bytes < need) return dffw_fail(DFFW_ENOMEM, "workspace %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    SIM_HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(sim_minmax, dim3(B), dim3(1024), 0, s, depth, (int64_t)H * W, w.mm, status);
    hipLaunchKernelGGL(sim_plan, dim3((B * N + 63) / 64), dim3(64), 0, s, params, cams, shifts, B, N, w, slices);
    const dim3 grid((W + SIM_TILE - 1) / SIM_TILE, (H + SIM_TILE - 1) / SIM_TILE, B * N);
    const bool lds = params.max_radius <= SIM_RL;
    if (lds)
        hipLaunchKernelGGL(sim_render<true>, grid, dim3(SIM_TILE * SIM_TILE), 0, s, params, image, depth, B, N, H, W, w, images, defocus,
                           depth_out, status, warped_tap);
    else
        hipLaunchKernelGGL(sim_render<false>, grid, dim3(SIM_TILE * SIM_TILE), 0, s, params, image, depth, B, N, H, W, w, images, defocus,
                           depth_out, status, warped_tap);
    SIM_HIPCHK(hipGetLastError());
    dffw_set_last_op_kernels(lds ? "dffw::sim_minmax;dffw::sim_plan;dffw::sim_render<true>" : "dffw::sim_minmax;dffw::sim_plan;dffw::sim_render<false>");
    return DFFW_OK;
}

}  // extern "C"
