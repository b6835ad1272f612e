/* dffw.h — C ABI of the MI355X (gfx950) depth-from-focus engine, libdffw.so.
 *
 * The reference (wcy199705/DfFintheWild) has no FFI/plugin layer: its boundary is the Python
 * nn.Module call `Network()(FS, focus_dists)` (Depth_Estimation_Test/test.py:30,118,
 * Depth_Estimation_Test/Depth_Estimation_Network.py:7-13) whose arithmetic runs inside PyTorch
 * operators.  This header is what a binding for that call binds instead: plain pointers and
 * sizes, no torch types.  dffinthewild_amd/engine.py is the ctypes stub.
 *
 * Conventions: every function returns 0 on success or a negative DFFW_E* code; the message is
 * available from dffw_last_error() (thread-local).  No C++ exception crosses this boundary.
 * "device" pointers are HIP device memory on the engine's device; "host" pointers are ordinary
 * memory.  All launches are enqueue-only on the caller's HIP stream (no implicit sync), so
 * timing around a call behaves like the reference's asynchronous model() call (test.py:117-119).
 */
#ifndef DFFW_H
#define DFFW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFFW_OK 0
#define DFFW_EINVAL (-1)  /* bad argument / shape contract violated */
#define DFFW_EHIP (-2)    /* a HIP runtime call failed */
#define DFFW_ENOMEM (-3)  /* workspace too small */
#define DFFW_EMISSING (-4)/* a required state-dict tensor was not supplied */

/* Arithmetic of the conv contractions (accumulation is always fp32 in the MFMA). */
#define DFFW_PREC_BF16X3 0 /* split-bf16: x = hi+lo, 3 MFMA products hi*hi+hi*lo+lo*hi (default; ~1e-5 rel-L2) */
#define DFFW_PREC_FP16 1   /* single fp16 product (~1e-3 rel-L2, weight dependent) */
#define DFFW_PREC_BF16 2   /* single bf16 product (~5e-3..1e-2 rel-L2; does not meet the 1e-3 target) */

/* Which network of the reference an engine implements. */
#define DFFW_NET_DEPTH 0 /* Depth_Estimation_Network.Network  (DEN.py:7-13): DFF_net alone, 384 entries */
#define DFFW_NET_E2E 1   /* End_to_End.Network (End_to_End/End_to_End.py:9-16): FlowNetwork alignment + DFF_net, 522 entries */
#define DFFW_E2E_SLICES 10 /* the alignment heads end in AdaptiveAvgPool3d((10,1,1)) (End_to_End.py:46,57,68) */

typedef struct dffw_engine dffw_engine;

/* One state-dict entry handed to the engine: the reference's key (an optional leading "module."
 * is accepted, test.py:32,78 vs train_code_Defocus.py:66), host fp32 data in PyTorch layout
 * (Conv3d (Cout,Cin,kd,kh,kw); ConvTranspose3d (Cin,Cout,kd,kh,kw); BatchNorm vectors). */
typedef struct dffw_tensor {
    const char *name;
    const float *data;
    int64_t numel;
} dffw_tensor;

/* Optional debug tap: after the forward, the named intermediate volume is written to `dst`
 * (device, fp32, reference layout (B,C,N,h,w), or (B,N,h,w) for the 1-channel score volumes).
 * Names: V1 V2 V3 FS_volume conf cost1 cost2 cost3, stem (the stem conv's output, the
 * first SRD block's input), E1 E2 (the two EFD blocks' outputs, the inputs of the 16 and 32 channel SRD blocks); for dffw_forward_e2e also
 * head3 head2 head1 (each alpha head's output before the 0.001 damping, (B,3,N)), alpha3 alpha2 (the accumulated warp
 * parameters after the level-3 and level-2 heads, (B,3,N)), alpha (the accumulated warp parameters the stack is finally warped
 * with, (B,3,N)) and fe1 fe2 fe3 (the alignment network's three feature levels, (B,8,N,H,W), (B,16,N,H/2,W/2), (B,32,N,H/4,W/4)). */
typedef struct dffw_tap {
    const char *name;
    float *dst;
    int64_t numel;
} dffw_tap;

const char *dffw_version(void);
const char *dffw_last_error(void);
/* Name of the kernel instantiation the calling thread's most recent convolution launch used (as rocprofv3 spells
 * it, e.g. "dffw::conv_roll<0, 8, 16, 4>"); "" before any.  Parity tests use it to prove which kernel they hit. */
const char *dffw_last_conv_kernel(void);

/* The weight contract (replaces nn.Module.state_dict() of DEN.py:7-57): number of state-dict
 * entries of network `net`, and entry `index` in the reference's registration order.
 * flags bit0: buffer (BatchNorm running stats) rather than parameter; bit1: int64
 * num_batches_tracked scalar; bit2: dead (present in checkpoints, never read by forward). */
int dffw_param_count(int net);
int dffw_param_info(int net, int index, const char **name, int64_t shape[5], int *ndim, int *flags);

/* Replaces `Network(); model.load_state_dict(...); model.cuda()` (test.py:30,78,80): folds
 * BatchNorm into the convs, packs weights into MFMA fragment order for `precision` and uploads
 * them to `device`.  The engine owns only that packed copy. */
int dffw_engine_create(int device, int net, const dffw_tensor *tensors, int n_tensors,
                       int precision, dffw_engine **out);
void dffw_engine_destroy(dffw_engine *e);
int dffw_engine_precision(const dffw_engine *e);

/* Repack the engine's weights from parameters that live on its GPU (after an optimiser step or any in-place edit): BatchNorm folding and every
 * operand layout dffw_engine_create wrote, by two kernels (dffw::repack_fold_kernel, dffw::repack_gather_kernel) on hip_stream.  The packed bytes
 * are exactly those of a dffw_engine_create from the same values.  tensors: as for dffw_engine_create, but `data` are DEVICE pointers on the
 * engine's device, fp32, contiguous; they must stay valid until the stream has run the kernels.  Every name the live layers need is looked up,
 * with its element count and a null check, before the first launch: on any refusal (DFFW_EMISSING; DFFW_EINVAL for a null engine, null tensors,
 * a wrong element count or a null pointer) nothing is enqueued and the engine is unchanged.  The first call builds the engine's repack plan
 * (allocates and copies); from the second on the call is enqueue-only: no allocation, no copy, no synchronisation, no atomics, and two calls with
 * the same values give the same bytes.  The caller orders the stream behind forwards that still read the weights. */
int dffw_engine_update(dffw_engine *e, const dffw_tensor *tensors, int n_tensors, void *hip_stream);
/* Test side: the engine's packed device buffers, concatenated in a fixed order (layer name, then the order the packer wrote them in).
 * dffw_engine_packed_bytes: their total size.  dffw_engine_packed_read: copies them to host_dst (capacity >= that size) after a synchronise of
 * hip_stream.  A null engine or destination, or a short capacity: DFFW_EINVAL. */
/* What the engine's repack plan holds and moves, once the first dffw_engine_update has built it (before: DFFW_EINVAL): out[0] device bytes of
 * the plan (scratch, source maps, job table); out[1] bytes the fold launches read and write; out[2] bytes of source maps and out[3] bytes of
 * operand buffers one gather launch reads and writes. */
int dffw_engine_repack_stats(const dffw_engine *e, int64_t out[4]);
int64_t dffw_engine_packed_bytes(const dffw_engine *e);
int dffw_engine_packed_read(dffw_engine *e, void *host_dst, int64_t capacity, void *hip_stream);

/* Bytes of scratch the engine's forward (dffw_forward for DFFW_NET_DEPTH, dffw_forward_e2e for
 * DFFW_NET_E2E) needs for one (B,N,H,W) call; the caller allocates it (torch's caching allocator in the
 * Python binding) so nothing is hipMalloc'ed per call. */
int64_t dffw_workspace_bytes(const dffw_engine *e, int B, int N, int H, int W);

/* Replaces `mid, p1, p2, p3 = model(FS, focus_dists)` (test.py:118; DFF_net.forward DEN.py:74-127).
 *   FS            device fp32, contiguous (B,3,N,H,W) — channel BEFORE slice (test_Dataloader.py:39)
 *   focus_dists   device fp32, element strides fd_strides[4] over (B,N,H,W); stride 0 = broadcast
 *                 ((B,N,1,1) of End_to_End/Test_dataloader.py:52-54, or dense (B,N,H,W))
 *   out[4]        device fp32 (B,H,W) each: mid_out, pred1, pred2, pred3 (DEN.py:127); entries may
 *                 be NULL to skip storing that map
 *   H, W          multiples of 32 (else DFFW_EINVAL, as the reference fails in torch.cat / pooling)
 */
int dffw_forward(dffw_engine *e, const float *FS, const float *focus_dists,
                 const int64_t fd_strides[4], int B, int N, int H, int W, float *const out[4],
                 void *workspace, int64_t workspace_bytes, void *hip_stream);

/* Same, additionally exporting intermediate volumes for parity debugging. */
int dffw_forward_taps(dffw_engine *e, const float *FS, const float *focus_dists,
                      const int64_t fd_strides[4], int B, int N, int H, int W, float *const out[4],
                      void *workspace, int64_t workspace_bytes, void *hip_stream,
                      const dffw_tap *taps, int n_taps);

/* Replaces `mid, p1, p2, p3, aligned = model(FS, focus_dists, FOVs)` of the End_to_End variant
 * (End_to_End/End_to_End.py:13-16; call site End_to_End/TRS.py:44): FlowNetwork.forward (End_to_End.py:71-105)
 * estimates per-slice warp parameters coarse to fine and warps the stack (FOV_warp, End_to_End.py:106-134),
 * DFF_net runs on the aligned stack.  Engine must have been created with DFFW_NET_E2E.
 *   FS, focus_dists, fd_strides, out[4], workspace, hip_stream   as for dffw_forward, N must be 10
 *   fovs          device fp32 (B,N): relative field of view of every slice (Test_dataloader.py:56-70)
 *   aligned       device fp32 (B,3,N,H,W): receives the aligned focal stack (5th return value); required
 *   taps          optional (NULL, 0)
 * Batch > 1 uses per-sample warp parameters, i.e. equals a stack of batch-1 reference calls (the reference's
 * own batch>1 path broadcasts sample 0's scale term by accident and is only ever run with batch 1, TRS.py:23). */
int dffw_forward_e2e(dffw_engine *e, const float *FS, const float *focus_dists,
                     const int64_t fd_strides[4], const float *fovs, int B, int N, int H, int W,
                     float *const out[4], float *aligned, void *workspace, int64_t workspace_bytes,
                     void *hip_stream, const dffw_tap *taps, int n_taps);

/* ---- per-launch timing (bench.py's roofline figures) -------------------------------------------
 * With profiling enabled every kernel launch of the next forward is bracketed by HIP events on the
 * caller's stream; dffw_profile_collect waits for them and returns one entry per launch.  Strings
 * stay valid until the next forward or the engine's destruction. */
typedef struct dffw_prof_entry {
    const char *kernel; /* kernel name as rocprofv3 --kernel-trace prints it, e.g. "dffw::conv_igemm<0, 1, 4>" */
    const char *layer;  /* state-dict prefix of the conv (e.g. "DFF_net.dres4.conv0.0.0") or the op name */
    double flops;       /* algorithmic FLOPs of the launch: 2*MAC of the layer's definition (DEN.py), no packing padding */
    double bytes;       /* algorithmic HBM bytes: activations read once + written once (+ residuals) in storage format */
    float ms;           /* elapsed time between the two events */
} dffw_prof_entry;
int dffw_profile_enable(dffw_engine *e, int on);
int dffw_profile_collect(dffw_engine *e, dffw_prof_entry *out, int capacity); /* returns the number of entries */

/* ---- single-operator entry points (parity tests of each kernel family; they allocate their own
 * temporaries with hipMalloc and synchronise the stream before returning) -------------------- */

/* y = [relu]( BN(conv(x)) [+ residual] ) in the engine's arithmetic.  Replaces nn.Conv3d /
 * nn.ConvTranspose3d (+ nn.BatchNorm3d, DEN.py:286-289).  x, residual, y: device fp32 in the
 * reference layout (B,C,N,H,W).  weight: host fp32, PyTorch layout.  bn: host fp32 4*Cout
 * values gamma|beta|mean|var, or NULL.  conv_bias: host fp32 Cout or NULL.  For transposed != 0
 * the geometry is fixed to the reference's only form: k3, stride (1,2,2), pad 1, output_padding
 * (0,1,1).  relu: 0 none, 1 relu(acc+res), 2 relu(acc)+res. */
int dffw_op_conv3d(int device, int precision, const float *x, int B, int Cin, int N, int H, int W,
                   const float *weight, int Cout, const int kernel[3], const int stride[3],
                   const int pad[3], const int dilation[3], int transposed, const float *bn,
                   const float *conv_bias, const float *residual, int relu, float *y,
                   void *hip_stream);

/* The same operator with the two extras the hourglass's last layer uses (DEN.py:96-97, 260-284: `out_in = x + conv6(...)`,
 * `cost = classif(out_in)`): y_pre (device fp32, y's shape, or NULL) receives BN(conv(x)) BEFORE the residual add; cls_weight (host fp32
 * Cout values, or NULL) is a bias-free 1x1x1 Cout -> 1 classifier applied to the final value y, its scores written to cls_score (device
 * fp32 (B,No,Ho,Wo)).  Needs Cout % 8 == 0. */
int dffw_op_conv3d_ex(int device, int precision, const float *x, int B, int Cin, int N, int H, int W,
                      const float *weight, int Cout, const int kernel[3], const int stride[3],
                      const int pad[3], const int dilation[3], int transposed, const float *bn,
                      const float *conv_bias, const float *residual, int relu, float *y, float *y_pre,
                      const float *cls_weight, float *cls_score, void *hip_stream);

/* mode 0: max-pool (1,k,k) stride (1,k,k) (DEN.py:310); mode 1: average-pool (DEN.py:149-153). */
int dffw_op_pool(int device, int precision, int mode, int k, const float *x, int B, int C, int N,
                 int H, int W, float *y, void *hip_stream);

/* The pyramid's three average pools (1,2,2), (1,4,4), (1,8,8) of one volume (hourglassup.forward, DEN.py:212-216) in one pass, by the forward's own
 * dffw::pool3_kernel<precision> (dffw_last_op_kernels names it): p2 (B,C,N,H/2,W/2), p4 (B,C,N,H/4,W/4), p8 (B,C,N,H/8,W/8), device fp32, each
 * bit-identical to dffw_op_pool(mode 1, k).  Test-only; allocates, poisons its workspace with 0xFF and synchronises.  C, H or W no multiple
 * of 8 is DFFW_EINVAL. */
int dffw_op_pool3(int device, int precision, const float *x, int B, int C, int N, int H, int W, float *p2, float *p4, float *p8,
                  void *hip_stream);

/* One SRD block of the front end (DEN.py:317-330: feat = relu(x + BN(conv(relu(BN(conv(x)))))), y = feat +
 * relu(conv1x1x1(relu(conv3x1x1(feat))))) through the forward's own dispatch, C = 8, 16 or 32 (FM_measure.Focus_extraction.2,
 * FM_conv1.1, FM_conv2.1).  Test-only.  x, y: device fp32 (B,C,N,H,W).  w0, w2: host fp32 (C,C,1,3,3) with bn0, bn2 (4*C
 * values gamma|beta|mean|var); w3 (C,C,3,1,1), w1 (C,C,1,1,1).  pooled: device fp32 (B,C,N,H/2,W/2) or NULL: max_pool(1,2,2)
 * of y, from the fused kernel's side output where that path writes one, else from the pool kernel. */
int dffw_op_srd(int device, int precision, const float *x, int B, int C, int N, int H, int W,
                const float *w0, const float *bn0, const float *w2, const float *bn2, const float *w3,
                const float *w1, float *y, float *pooled, void *hip_stream);

/* One EFD block (DEN.py:306-315: y = relu(BN(conv3^3 s(1,2,2)(x)) + BN(conv3^3(maxpool(1,2,2)(x))))), Cin = 8 or 16,
 * Cout = 2*Cin (FM_conv1.0, FM_conv2.0), through the forward's own dispatch.  Test-only.  x: device fp32 (B,Cin,N,H,W),
 * H and W even; y: (B,Cout,N,H/2,W/2).  ws, wp: host fp32 (Cout,Cin,3,3,3) with bns, bnp.  pooled_at_hand != 0: x is first
 * max-pooled by the pool kernel and the copy handed to the block, as the forward's SRD block leaves it (the fused kernels
 * need it); 0: the block pools for itself. */
int dffw_op_efd(int device, int precision, const float *x, int B, int Cin, int N, int H, int W,
                const float *ws, const float *bns, const float *wp, const float *bnp, int pooled_at_hand,
                float *y, void *hip_stream);

/* One resnet_block_2d_OF of the alignment network (End_to_End.py:135-145: y = relu(feature(x) + BN2(conv(relu(BN0(conv_s(x))))))),
 * feature a bias-free 1x1x1 conv with the same (1,s,s) stride) through the forward's own dispatch.  Test-only.  (Cin, Cout, stride)
 * is one of (3,8,1) (8,8,1) (8,16,2) (16,16,1) (16,32,2) (32,32,1) (OF_feature.0 ... OF_feature2.1); for (3,8,1) x is the fp32 stack
 * and the first block's own dispatch (of_first_kernel, or the padded record volume and the general block) runs.  x: device fp32
 * (B,Cin,N,H,W), H and W multiples of the stride; y: (B,Cout,N,H/stride,W/stride).  w0: host fp32 (Cout,Cin,1,3,3), w2
 * (Cout,Cout,1,3,3) with bn0, bn2 (4*Cout values gamma|beta|mean|var); wf (Cout,Cin,1,1,1). */
int dffw_op_of_block(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, int Cout, int stride,
                     const float *w0, const float *bn0, const float *w2, const float *bn2, const float *wf, float *y,
                     void *hip_stream);

/* The back half of one alpha head of the alignment network (End_to_End.py:37-69, 86-103) through the forward's own dispatch: from the first
 * conv's output through convs .2 and .4 (1x3x3, BatchNorm, ReLU), the biased conv .6 (C -> 3) and the plane mean to
 *   raw[b,c,n] = m = bias6[c] + mean_{y,x} conv(y2, w6)[b,c,n],   alpha[b,c,n] += (c == 0 ? 0.001 * m : m).
 * Test-only.  C = 16, 32 or 64 selects the head (conv3, conv2, conv1) and the layer names the weights are packed under.  x: device fp32
 * (B,C,N,H,W): with start = 0 the first conv's output y0, with start = 2 the third conv's output y2 (only conv .6 and the mean then run,
 * on the stored-y2 forms).  w2, w4: host fp32 (C,C,1,3,3) with bn2, bn4 (4*C values gamma|beta|mean|var); w6 (3,C,1,3,3), bias6 (3).
 * alpha: device fp32 (B,3,N), read and updated in place; raw: device fp32 (B,3,N).  Refused with DFFW_EINVAL before any GPU call: a null
 * pointer, an unknown precision, C outside {16, 32, 64}, start outside {0, 2}, a size below 1, B * N * 3 > 65535. */
int dffw_op_head_tail(int device, int precision, const float *x, int B, int C, int N, int H, int W, const float *w2, const float *bn2,
                      const float *w4, const float *bn4, const float *w6, const float *bias6, int start, float *alpha, float *raw,
                      void *hip_stream);

/* The front half of one alpha head of the alignment network (End_to_End.py:77-101) through the forward's own dispatch: the level features
 * warped by the parameters accumulated so far (FOV_warp, bilinear in the plane, zeros outside) and the head's first conv over them,
 *   y0[b,:,n] = relu(BN(conv1x3x3([warp(fe)[b,:,N-1] | warp(fe)[b,:,n] | flow_x, flow_y of slice n], w0))),
 * as head_warp_kernel on the split filter, as the split filter over a [cur | flow] volume, or as the whole filter over the whole volume
 * (whichever the shape and the switches select).  Test-only.  C = 8, 16 or 32 selects the head (conv3, conv2, conv1) and the layer names the
 * filter is packed under.  fe: device fp32 (B,C,N,H,W); w0: host fp32 (2C,2C+2,1,3,3) with bn0 (4*2C values gamma|beta|mean|var); alpha:
 * device fp32 (B,3,N) (scale offset, x shift, y shift); fov: device fp32 (B,N); y0: device fp32 (B,2C,N,H,W).  Refused with DFFW_EINVAL
 * before any GPU call: a null pointer, an unknown precision, C outside {8, 16, 32}, a size below 1. */
int dffw_op_head_front(int device, int precision, const float *fe, int B, int C, int N, int H, int W, const float *w0, const float *bn0,
                       const float *alpha, const float *fov, float *y0, void *hip_stream);

/* Kernel names of every launch of the calling thread's last dffw_op_srd / dffw_op_efd / dffw_op_of_block / dffw_op_head_front / dffw_op_head_tail / dffw_op_regress_heads / dffw_sim_render / dffw_augment_stack call, in launch order, joined by
 * ';' (as dffw_profile_collect spells them); "" before any, or after a call that failed before launching. */
const char *dffw_last_op_kernels(void);

/* The regression block of DEN.py:86-90: bilinear resize (align_corners=False) of score (B,N,h,w) to
 * (H,W), softplus+1e-6, normalise over N, sum_N focus_dists*p -> depth (B,H,W).  All device fp32. */
int dffw_op_regress(int device, const float *score, int B, int N, int h, int w, int H, int W,
                    const float *focus_dists, const int64_t fd_strides[4], float *depth,
                    void *hip_stream);

/* 1..4 regression heads that share the output size and the focus distances, in ONE launch, as the forward runs them: score[k] device fp32
 * (B,N,h[k],w[k]) -> depth[k] device fp32 (B,H,W); any h[k], w[k] >= 1 (up- and downsampling).  focus_dists: device fp32 read through the
 * element strides fd_strides (any, 0 included) of dims (B,N,H,W).  fused != 0: the forward's choice -- dffw::regress_fused_kernel<10> (N <= 10)
 * or <16> (N <= 16) for two or more heads, dffw::regress_kernel (one workgroup row per head) otherwise; fused == 0: always dffw::regress_kernel
 * (the forward under DFFW_NO_REGRESS_FUSED).  dffw_last_op_kernels names the kernel launched.  Every head's depth map is bit-identical to
 * dffw_op_regress on that head alone.  Synchronises.  Both entry points refuse with DFFW_EINVAL before any GPU call: a null pointer, n_heads
 * outside 1..4, any of B, N, H, W, h[k], w[k] below 1. */
int dffw_op_regress_heads(int device, int n_heads, const float *const score[4], const int h[4], const int w[4],
                          float *const depth[4], int B, int N, int H, int W, const float *focus_dists,
                          const int64_t fd_strides[4], int fused, void *hip_stream);

/* The warp operator of the End_to_End alignment path on its own.
 * Replaces FlowNetwork.FOV_warp (End_to_End/End_to_End.py:106-134): warps x (B,C,N,H,W)
 * by the per-slice field-of-view scale and translation.  alpha: device fp32 (B,3,N) = (scale offset,
 * x shift, y shift) per slice; fovs: device fp32 (B,N); out: (B,C,N,H,W); flow: (B,2,N,H,W) or NULL (the
 * pixel-unit flow the reference returns as its second value).  alpha_from_sample0 != 0 reproduces the
 * reference's batch>1 broadcast quirk (End_to_End.py:112: `alpha[:,0,:,:] + FOVs` broadcasts to (B,B,N,1,1) and
 * `[:,0]` keeps alpha[0,n] + FOVs[b,n]: every sample uses SAMPLE 0's scale offset with its OWN FOV). */
int dffw_op_fov_warp(int device, const float *x, int B, int C, int N, int H, int W, const float *alpha,
                     const float *fovs, int alpha_from_sample0, float *out, float *flow, void *hip_stream);

/* ---- input pipeline ---------------------------------------------------------------
 * Replaces the NumPy tensor assembly of the reference's loaders: `FS/127.5 - 1.0`, the transpose to (3,N,H,W) and the
 * bottom/right padding to multiples of 32 with -1 (Depth_Estimation_Test/test_Dataloader.py:80-89 HCI, :122-141 DDFF,
 * :197-228 Smartphone; End_to_End/Test_dataloader.py:56-75 Real_Scenes: all float32 arrays, i.e. a float32 divide followed
 * by a float32 subtract).  The FS6 / DefocusNet loader (test_Dataloader.py:31-39) differs: it concatenates its images onto
 * np.zeros((256,256,3,0)), a FLOAT64 array, so its `/127.5 - 1.0` runs in float64 and torch.Tensor() rounds once at the end
 * (128 of the 256 byte values then differ by one float32 ulp from the float32 form): OR DFFW_RAW_NORM_F64 into `dtype` to get
 * that arithmetic, (float)((double)v / 127.5 - 1.0).
 *   raw      device uint8 (DFFW_RAW_U8) or fp32 0..255 (DFFW_RAW_F32) stack in ANY source layout, described by
 *            element strides {batch, slice, row, col, channel}: (N,H,W,3) hdf5 stacks, (H,W,3,N) / (H,W,N,3) image
 *            arrays; a crop (test_Dataloader.py:205, Test_dataloader.py:58) is a pointer offset by the caller
 *   h, w     rows / cols taken from the source;  Hp, Wp  padded size, multiples of 32, >= h, w
 *   FS       device fp32 (B,3,N,Hp,Wp): exactly the tensor the reference's loader yields (float32 divide, then
 *            subtract; -1 in the padding).  Enqueue-only on hip_stream. */
#define DFFW_RAW_U8 0
#define DFFW_RAW_F32 1
#define DFFW_RAW_NORM_F64 16 /* flag OR-ed into dtype: normalise in float64, round once (the FS6 loader) */
int dffw_pack_stack(int device, const void *raw, int dtype, const int64_t strides[5], int B, int N, int h, int w,
                    int Hp, int Wp, float *FS, void *hip_stream);

/* ---- training-sample assembly (train_codes/train_Dataloader.py with train_codes/augmentation.py) ---------------
 * What the reference's five training loaders do to a decoded sample: random crop to the training size, the photometric chain
 * image_augmentation (x/255, (0.5 + contrast*(x-0.5)) + brightness, clamp to [0,1], np.power(x, gamma), clamp, x/0.5 - 1.0),
 * horizontal flip, vertical flip, np.rot90, the ground-truth range rule with its mask, and the transpose to (3,N,h,w) float32.
 * Every arithmetic step is one IEEE operation in the reference's order, in float32 (sources the loaders hold as float32: DDFF,
 * HCI, Smartphone) or, with DFFW_RAW_NORM_F64, in float64 rounded once at the end (FS6, FlyingThings); the power is evaluated in
 * double in both.  With gamma == 1 the result is bit-identical to NumPy's; otherwise within 2^-22 absolute.
 *   raw / dtype / strides   as for dffw_pack_stack, but `raw` points at the WHOLE (H, W) source: the crop is per sample
 *   h, w       window taken from every sample (h <= H, w <= W)
 *   params     DEVICE fp64 (B, DFFW_AUG_NPARAMS), one record per sample in DFFW_AUG_* order: crop origin (row, col; clamped into
 *              the source), contrast, brightness, gamma, flip_x and flip_y (flip if > 0.5: the loaders' uniform draws or 0 / 1),
 *              angle (quarter turns, taken mod 4)
 *   transposed 1 if the angles are odd: FS is (B,3,N,w,h) instead of (B,3,N,h,w).  Where h != w every sample's angle must have
 *              this parity (its low bit is taken from here); where h == w angles may be mixed
 *   FS         device fp32 (B,3,N,h',w'), no padding
 *   gt, conf   device fp32 (B,H,W) contiguous, or NULL;  gt_out / conf_out fp32 (B,h',w'), mask_out uint8 (B,h',w') = (gt_out != sentinel).
 *              use_range != 0: gt values < lo or > hi become `sentinel` first (float32 comparisons); NaN stays NaN and is valid.
 * Enqueue-only on hip_stream, no allocation.  The kernel names are reported by dffw_last_op_kernels. */
#define DFFW_AUG_NPARAMS 8
enum { DFFW_AUG_Y0, DFFW_AUG_X0, DFFW_AUG_CONTRAST, DFFW_AUG_BRIGHTNESS, DFFW_AUG_GAMMA, DFFW_AUG_FLIP_X, DFFW_AUG_FLIP_Y, DFFW_AUG_ANGLE };
int dffw_augment_stack(int device, const void *raw, int dtype, const int64_t strides[5], int B, int N, int H, int W, int h, int w,
                       const double *params, int transposed, float *FS, const float *gt, const float *conf, float *gt_out,
                       uint8_t *mask_out, float *conf_out, int use_range, float lo, float hi, float sentinel, void *hip_stream);

/* dffw_forward on the raw stack: the stem kernel's loader applies `x/127.5 - 1` and the -1 padding while it stages its
 * tiles, so the normalised fp32 stack (4x the bytes of a uint8 source) is never written or read.  Bit-identical to
 * dffw_pack_stack followed by dffw_forward.  raw / dtype / raw_strides / h / w as for dffw_pack_stack; H, W are the
 * padded sizes (multiples of 32, >= h, w).  DFFW_NET_DEPTH engines.  Workspace: dffw_workspace_bytes(B,N,H,W) plus
 * B*3*N*H*W*4 bytes (used only when the shape is too small for the tiled stem kernel and the stack is expanded first). */
int dffw_forward_raw(dffw_engine *e, const void *raw, int dtype, const int64_t raw_strides[5], int h, int w,
                     const float *focus_dists, const int64_t fd_strides[4], int B, int N, int H, int W,
                     float *const out[4], void *workspace, int64_t workspace_bytes, void *hip_stream);

/* ---- output post-processing -------------------------------------------------------
 * dffw_colorize replaces the crop + normalise + `cm.get_cmap('jet')` + uint8 pass of Depth_Estimation_Test/test.py:124-133
 * and End_to_End/test_real_scenes.py:40-52:  rgb[b,y,x,:] = jet((depth[b,y,x] - lo) / (hi - lo)) for y < h, x < w.
 *   depth    device fp32 (B,H,W) as returned by dffw_forward (pred3)
 *   mode     DFFW_RANGE_FIXED: lo, hi given (test.py:132, the data set's depth range);
 *            DFFW_RANGE_MINMAX: each map's own min / max over the whole padded map (test_real_scenes.py:40)
 *   range    device fp32 (B,2) scratch AND result: the (lo, hi) pair used for every map
 *   rgb      device uint8 (B,h,w,3), RGB, `(255 * colour).astype(uint8)` truncation (test_real_scenes.py:48-49)
 * Colour-map semantics are matplotlib's: index = trunc(float32(x * 256)), x == 1 -> 255, x < 0 / x > 1 clamp, NaN -> black.
 * dffw_jet_lut writes the 256 x 3 uint8 table the kernel uses (host memory) for inspection / tests. */
#define DFFW_RANGE_FIXED 0
#define DFFW_RANGE_MINMAX 1
int dffw_colorize(int device, const float *depth, int B, int H, int W, int h, int w, int mode, float lo, float hi,
                  float *range, uint8_t *rgb, void *hip_stream);
int dffw_jet_lut(uint8_t *lut768);

/* dffw_unpack_stack replaces the warped-stack export of End_to_End/test_real_scenes.py:42-47:
 *     np.squeeze(127.5 * (warp + 1.0)).astype(np.uint8), transposed to (H,W,3,N) and written slice by slice cropped to (h,w).
 *   warp     device fp32 (B,3,N,H,W): the aligned stack dffw_forward returns in out[4] for DFFW_NET_E2E engines
 *   images   device uint8 (B,N,h,w,3): slice n of stack b as an interleaved image in the channel order of the input (the
 *            reference reads BGR with cv2 and writes it back with cv2)
 * Arithmetic: float32 `127.5f * (v + 1.0f)`, truncated toward zero; values in [-1,1] land in 0..255.  Outside that NumPy's cast is
 * platform-defined; this entry point follows x86 NumPy (conversion to int32, low byte kept; NaN and |t| >= 2^31 give 0). */
int dffw_unpack_stack(int device, const float *warp, int B, int N, int H, int W, int h, int w, uint8_t *images, void *hip_stream);

/* dffw_metrics replaces the masked NumPy metrics of Depth_Estimation_Test/metrics.py:90-127 as called from
 * test.py:144-158: est = pred3 (B,H,W) cropped to (h,w) (test.py:124-126); gt fp32 (B,h,w); mask uint8 (B,h,w)
 * (non-zero = valid); conf fp32 (B,h,w) or NULL (Smartphone confidence, test.py:145-146).
 *   out      device fp64 (B, DFFW_N_METRICS): valid pixels, abs_rel, sq_rel, mse, mae, rmse, rmse_log,
 *            accuracy(1.25), accuracy(1.25^2), accuracy(1.25^3), mse_w_conf, mae_w_conf (the last two NaN without conf)
 *   scratch  device memory of dffw_metrics_scratch_bytes(B)
 * Per-pixel terms are float32 like the NumPy expressions; sums are float64 in a fixed order (run-to-run identical). */
#define DFFW_N_METRICS 12
int64_t dffw_metrics_scratch_bytes(int B);
int dffw_metrics(int device, const float *est, int B, int H, int W, const float *gt, const uint8_t *mask,
                 const float *conf, int h, int w, double *out, void *scratch, int64_t scratch_bytes, void *hip_stream);

/* ---- training loss and regression-head backward (train_codes/train_code_*.py, Depth_Estimation_Network.py:89-98, 118-134) ----
 * dffw_loss_heads evaluates, for n_heads regression heads that share the output size, the focus distances and the ground truth,
 *     d_k    = the head's prediction (bit-identical to dffw_op_regress on the same scores)
 *     Loss_k = sum_i c_i m_i ((d_k - gt)/r)^2 / Z,  Z = sum_i c_i m_i   (c = 1 without conf: nn.MSELoss over est[mask]),  r = hi - lo or 1
 *     Total  = sum_k weights[k] Loss_k
 * and dTotal/dscore_k, the gradient through softplus, the normalisation over the slices and the bilinear upsample.
 *   score[k]      device fp32 (B,N,h[k],w[k]); H = s*h[k], W = s*w[k] with s in {1,2,4,8} (else DFFW_EINVAL)
 *   focus_dists   device fp32, element strides fd_strides (any, 0 included) for dims (B,N,H,W)
 *   gt, conf      device fp32 (B,H,W), conf may be NULL; mask uint8 (B,H,W), non-zero = valid.  A pixel outside the mask
 *                 contributes nothing, whatever its gt (NaN included)
 *   pred[k]       device fp32 (B,H,W), entries or the array may be NULL
 *   grad[k]       device fp32 (B,N,h[k],w[k]), entries or the array may be NULL (loss only)
 *   losses        device fp64, n_heads + 1: Loss_k per head, then Total.  Z == 0: NaN losses and all-zero gradients
 *   workspace     device memory of dffw_loss_workspace_bytes(B,N,H,W): Z and the workgroups' float64 loss partials; need not be cleared
 * Enqueue-only on hip_stream, no allocation; float64 sums and the gather-form upsample adjoint run in a fixed order (no atomics), so
 * two calls give identical bits.  B <= 65535, H*W < 2^31; B*H*W and N are free.  dffw_last_op_kernels lists the launches. */
int64_t dffw_loss_workspace_bytes(int B, int N, int H, int W);
int dffw_loss_heads(int device, int n_heads, const float *const score[4], const int h[4], const int w[4],
                    int B, int N, int H, int W, const float *focus_dists, const int64_t fd_strides[4],
                    const float *gt, const uint8_t *mask, const float *conf, const float weights[4],
                    int use_range, float lo, float hi, float *const pred[4], float *const grad[4],
                    double *losses, void *workspace, int64_t workspace_bytes, void *hip_stream);

/* ---- backward of the regression heads under any upstream gradient -------------------------------------------------------
 * dffw_heads_backward differentiates the heads of dffw_op_regress_heads on their own: given grad_pred[k] = dL/dd_k of any loss L,
 *     dL/dv_n(i) = grad_pred(i) (f_n - d_k)/S sigmoid(v_n)  (sigmoid = 1 for v > 20),   grad_score[k] = upsample^T(dL/dv)
 * with v, S and d_k as in dffw_loss_heads.  No mask, gt, conf or loss: those live in the caller's own graph.
 *   score[k]       device fp32 (B,N,h[k],w[k]); H = s*h[k], W = s*w[k] with s in {1,2,4,8} (else DFFW_EINVAL)
 *   focus_dists    device fp32, element strides fd_strides (any, 0 included) for dims (B,N,H,W)
 *   grad_pred[k]   device fp32 (B,H,W) contiguous; a zero contributes exactly zero, NaN / Inf reach the elements the pixel's taps touch
 *   grad_score[k]  device fp32 (B,N,h[k],w[k]) contiguous; every element is written.  N == 1: all zeros
 * A head whose grad_pred and grad_score are both NULL is skipped; one of the two NULL is DFFW_EINVAL.  n_heads outside 1..4, a null array
 * or score, a dimension below 1, B > 65535, H*W >= 2^31 or a head of another size: DFFW_EINVAL before the GPU is touched.
 * Enqueue-only on hip_stream: one launch per head that has a gradient (dffw_last_op_kernels lists them), no allocation, no workspace, no
 * atomics; the summation order is fixed, so two calls give identical bits. */
int dffw_heads_backward(int device, int n_heads, const float *const score[4], const int h[4], const int w[4],
                        int B, int N, int H, int W, const float *focus_dists, const int64_t fd_strides[4],
                        const float *const grad_pred[4], float *const grad_score[4], void *hip_stream);

/* ---- conv backward: data and weight gradients of the aggregation network's plain convs ------------------------------
 * Geometries (anything else, and dilation, is DFFW_EINVAL): 3x3x3 pad 1 stride 1 or (1,2,2); 1x3x3 pad (0,1,1) stride 1; the transposed
 * 3x3x3 stride (1,2,2) pad 1 output_padding (0,1,1).  Cin and Cout multiples of 8, at most 128; H and W even at stride (1,2,2).
 *   grad_x = d<grad_y, conv(x, weight)>/dx   the adjoint conv, through the forward's own kernel dispatch (dffw_last_conv_kernel shows it)
 *   grad_w = d<grad_y, conv(x, weight)>/dw   dffw::conv_wgrad_kernel + dffw::conv_wgrad_finish_kernel (dffw_last_op_kernels lists them)
 * in the engine's arithmetic: both operands rounded to the activation records of `precision`, fp32 MFMA accumulation; the weight gradient's
 * fp32 accumulators are flushed into float64 sums after at most 16 384 pixels, and those are added in a fixed order (no atomics: two calls
 * give identical bits).
 *
 * dffw_op_conv3d_backward: layouts as dffw_op_conv3d.  x (B,Cin,N,H,W) and grad_y (the forward's output shape: (B,Cout,N,H/s,W/s), or
 * (B,Cout,N,2H,2W) transposed) device fp32; weight host fp32 in PyTorch layout (may be NULL without grad_x); grad_x device fp32 like x, or
 * NULL; grad_w DEVICE fp32 in the weight's PyTorch layout, or NULL.  No bias: the plain conv's adjoint (train-mode BatchNorm with its ReLU
 * and residual gradients is dffw_bn_train_backward below).
 * Allocates its temporaries, poisons its workspace with 0xFF and synchronises.  grad_y's shape is implied by the geometry (the Python
 * binding checks the tensor against it).
 *
 * dffw_conv_wgrad: the enqueue-only form a training step calls.  x and grad_y are activation RECORDS [pixel][part][channel] (16-bit, the
 * engine's internal layout) of the same shapes; workspace: dffw_conv_wgrad_workspace_bytes(...) bytes, need not be cleared (0 for
 * arguments dffw_conv_wgrad refuses). */
int dffw_op_conv3d_backward(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *weight, int Cout,
                            const int kernel[3], const int stride[3], const int pad[3], int transposed, const float *grad_y, float *grad_x,
                            float *grad_w, void *hip_stream);
int64_t dffw_conv_wgrad_workspace_bytes(int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int stride[3],
                                        const int pad[3], int transposed);
int dffw_conv_wgrad(int device, int precision, const void *x, int B, int Cin, int N, int H, int W, const void *grad_y, int Cout,
                    const int kernel[3], const int stride[3], const int pad[3], int transposed, float *grad_w, void *workspace,
                    int64_t workspace_bytes, void *hip_stream);

/* ---- train-mode BatchNorm3d with its residual add and ReLU, forward and backward -------------------------------------
 * Per channel c over the M = B*N*H*W pixels of a volume (nn.BatchNorm3d in training mode, Depth_Estimation_Network.py convbn_3d):
 *     mean = sum x / M    var = sum (x - mean)^2 / M (biased)    invstd = 1 / sqrt(var + eps)
 *     y = [relu]( gamma (x - mean) invstd + beta [+ res] )
 *     running_mean <- (1 - momentum) running_mean + momentum mean      running_var <- ... + momentum var M / (M - 1)
 *     g = relu ? grad_y [y > 0] : grad_y     grad_res = g     grad_beta = sum g     grad_gamma = sum g (x - mean) invstd
 *     grad_x = gamma invstd ( g - grad_beta / M - (x - mean) invstd grad_gamma / M )
 * x is the value the records hold (hi + lo for split-bf16).  The sums are float64 sums of exact terms, per workgroup and then over the
 * workgroups in a fixed order (no atomics): two calls give identical bits; DFFW_BN_WGS (the launches' workgroups) changes only the
 * order of float64 additions.  Refused with DFFW_EINVAL before any launch: C outside {8, 16, 32, 64, 128}, M == 1 (PyTorch raises
 * there), M >= 2^31, eps <= 0, an unknown precision; a short workspace is DFFW_ENOMEM.  dffw_last_op_kernels lists the launches.
 *
 * Record forms (dffw_bn_train_forward / _backward): enqueue-only on hip_stream, no allocation.  x, res, y, grad_y, grad_x, grad_res
 * are activation RECORDS [pixel][part][channel] of `precision` (16-byte aligned), the layout dffw_conv_wgrad reads; gamma, beta,
 * running_*, save_*, grad_gamma, grad_beta device fp32 (C).  May be NULL: running_mean, running_var, res, grad_res; y in the forward
 * without ReLU and residual (statistics only) and in the backward without ReLU; grad_x (parameter gradients only; then grad_res too).
 * The ReLU mask of the backward is read from the stored y.  workspace: dffw_bn_train_workspace_bytes(...) bytes (0 for a refused
 * shape): the workgroups' float64 partial sums, nothing that scales with M; need not be cleared.
 *
 * Op forms (dffw_op_bn_train / _backward): the same on device fp32 tensors (B,C,N,H,W); they convert to records and back, allocate
 * their temporaries, poison the workspace with 0xFF and synchronise.  y of the backward is the forward's returned y. */
int64_t dffw_bn_train_workspace_bytes(int B, int C, int N, int H, int W);
int dffw_bn_train_forward(int device, int precision, const void *x, int B, int C, int N, int H, int W, const float *gamma, const float *beta,
                          double eps, double momentum, float *running_mean, float *running_var, const void *res, int relu, void *y,
                          float *save_mean, float *save_invstd, void *workspace, int64_t workspace_bytes, void *hip_stream);
int dffw_bn_train_backward(int device, int precision, const void *x, const void *y, const void *grad_y, int B, int C, int N, int H, int W,
                           const float *gamma, const float *save_mean, const float *save_invstd, int relu, void *grad_x, void *grad_res,
                           float *grad_gamma, float *grad_beta, void *workspace, int64_t workspace_bytes, void *hip_stream);
int dffw_op_bn_train(int device, int precision, const float *x, int B, int C, int N, int H, int W, const float *gamma, const float *beta,
                     double eps, double momentum, float *running_mean, float *running_var, const float *res, int relu, float *y,
                     float *save_mean, float *save_invstd, void *hip_stream);
int dffw_op_bn_train_backward(int device, int precision, const float *x, const float *y, const float *grad_y, int B, int C, int N, int H,
                              int W, const float *gamma, const float *save_mean, const float *save_invstd, int relu, float *grad_x,
                              float *grad_res, float *grad_gamma, float *grad_beta, void *hip_stream);

/* ---- backward of the convs without in-plane taps, and the gradient mask-and-add between them ------------------------
 * The attention tail of every Feature_Extraction block (Conv3d(C,C,(3,1,1), pad (1,0,0)) -> ReLU -> Conv3d(C,C,1) -> ReLU -> + Feature) and
 * the 1x1x1 convs redir1/2/3 and pre_conv.  Geometries: kernel (3,1,1) with pad (1,0,0), kernel (1,1,1) with pad 0; stride 1, dilation 1,
 * no bias; Cin and Cout multiples of 8 up to 128.  Anything else: DFFW_EINVAL before any launch.
 *   grad_x   the adjoint conv (filter flipped along the slice axis, in / out channels swapped) through the forward's own dispatch
 *   grad_w   dffw::conv_pw_wgrad_kernel + dffw::conv_pw_wgrad_finish_kernel (dffw_last_op_kernels lists them), (Cout, Cin, kd, 1, 1) fp32:
 *            fp32 MFMA partials of at most 16 384 pixels, summed in float64 in a fixed order -- two calls give identical bits
 * dffw_op_conv_pw_backward: x, grad_y (B,C,N,H,W) device fp32, weight host fp32 (may be NULL without grad_x), grad_x / grad_w device fp32 or
 * NULL; allocates, poisons its workspace with 0xFF and synchronises.  dffw_conv_pw_wgrad: the enqueue-only form on activation RECORDS
 * (16-byte aligned); workspace: dffw_conv_pw_wgrad_workspace_bytes(...) bytes, need not be cleared (0 for refused arguments; too short: DFFW_ENOMEM).
 *
 * dffw_grad_combine: out = [y > 0] a (+ b) on records of C channels (a multiple of 8 up to 128): the ReLU mask of a conv that has no
 * BatchNorm, read from the STORED y, and / or the sum of two gradients of one tensor.  y and b may each be NULL, not both (DFFW_EINVAL);
 * out may alias a, y or b.  Without b the record of a passes bit for bit where the mask passes and is +0 elsewhere; with b the two record
 * values are added in fp32 (one rounding) and split into a record.  One launch, enqueue-only, no workspace.  dffw_op_grad_combine: the same
 * on device fp32 tensors (B,C,N,H,W). */
int dffw_op_conv_pw_backward(int device, int precision, const float *x, int B, int Cin, int N, int H, int W, const float *weight, int Cout,
                             const int kernel[3], const int pad[3], const float *grad_y, float *grad_x, float *grad_w, void *hip_stream);
int64_t dffw_conv_pw_wgrad_workspace_bytes(int B, int Cin, int N, int H, int W, int Cout, const int kernel[3], const int pad[3]);
int dffw_conv_pw_wgrad(int device, int precision, const void *x, int B, int Cin, int N, int H, int W, const void *grad_y, int Cout,
                       const int kernel[3], const int pad[3], float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream);
int dffw_grad_combine(int device, int precision, const void *a, const void *y, const void *b, int B, int C, int N, int H, int W, void *out,
                      void *hip_stream);
int dffw_op_grad_combine(int device, int precision, const float *a, const float *y, const float *b, int B, int C, int N, int H, int W,
                         float *out, void *hip_stream);

/* ---- backward of the attention tail as one node ---------------------------------------------------------------------------
 * y = x + relu(conv111(relu(conv311(x)))) with a = relu(conv311(x)) and t = relu(conv111(a)) kept by the forward; C is 8, 16 or 32, no bias.
 *   gt = [t > 0] grad_y;  ga = [a > 0] W1^T gt;  grad_x = grad_y + the adjoint 3x1x1 conv of ga;  grad_w1 = sum gt a;  grad_w3 = sum ga x
 * in ONE kernel, dffw::att_tail_bwd_kernel, that reads x, a, t and grad_y once and writes grad_x once (ga stays on chip, rounded to the record
 * format), plus dffw::att_tail_bwd_finish_kernel for the weight gradients (dffw_last_op_kernels lists them): fp32 MFMA partials of at most 16 384
 * pixels, added in float64 in a fixed order, no atomics -- two calls give identical bits.  The masks are those of the STORED a and t.
 * dffw_att_tail_backward: enqueue-only on activation RECORDS (16-byte aligned), no allocation; w3 (C,C,3,1,1) and w1 (C,C,1,1,1) device fp32 in
 * PyTorch layout (split by the kernel itself).  grad_x may be NULL, grad_w3 and grad_w1 may be NULL together (one without the other:
 * DFFW_EINVAL); w3 may be NULL without grad_x (w1 is always read: ga needs it); a call with no output launches nothing.  grad_x may alias
 * grad_y.  workspace: dffw_att_tail_backward_workspace_bytes(...) bytes, need not be cleared (0 for refused arguments; too short:
 * DFFW_ENOMEM), and may be NULL without the weight gradients.  Refused with DFFW_EINVAL before the GPU is touched: C outside {8, 16, 32},
 * dimensions < 1, 2^31 units (128-pixel columns) or more, an unknown precision.
 * dffw_op_att_tail_backward: the same on device fp32 tensors (B,C,N,H,W) with HOST fp32 weights; allocates, poisons its workspace with 0xFF
 * and synchronises. */
int64_t dffw_att_tail_backward_workspace_bytes(int B, int C, int N, int H, int W);
int dffw_att_tail_backward(int device, int precision, const void *x, const void *a, const void *t, const void *grad_y, int B, int C, int N, int H,
                           int W, const float *w3, const float *w1, void *grad_x, float *grad_w3, float *grad_w1, void *workspace,
                           int64_t workspace_bytes, void *hip_stream);
int dffw_op_att_tail_backward(int device, int precision, const float *x, const float *a, const float *t, const float *grad_y, int B, int C, int N,
                              int H, int W, const float *w3, const float *w1, float *grad_x, float *grad_w3, float *grad_w1, void *hip_stream);

/* ---- backward of the pools ---------------------------------------------------------------------------------------------
 * The adjoints of MaxPool3d((1,2,2)) (the second branch of both res_stride_conv_3d blocks), of AvgPool3d((1,k,k)), k = 2, 4, 8, and of the
 * pyramid's three average pools of one volume (hourglassup) in one pass.  B, C, N, H, W describe the pools' INPUT, which is where the
 * gradient `out` is written; C a multiple of 8 up to 128, H and W divisible by k (pyramid: by 8), fewer than 2^31 pixels.
 *   mode 0, max (k = 2)   g goes to the FIRST maximum of its 2x2 window of x in row-major order (dy, then dx), as torch does; the values
 *                          compared are those of the stored records of x, the forward's input (-0 and +0 are equal; inputs are finite).
 *                          Without b the record of g passes bit for bit and the other three pixels are +0.
 *   mode 1, avg           out = g[p / k] / k^2 (exact in fp32).  x is not read.
 *   pyramid               out = ((g8[p / 8] / 64 + g4[p / 4] / 16) + g2[p / 2] / 4), fp32 additions in this order.
 * b, or NULL: a second gradient of the input (B,C,N,H,W), added in fp32 before the one split into a record; out may alias b.  Every element
 * of out is written exactly once (out need not be cleared): no atomics, no workspace, identical bits from call to call and grid to grid.
 * dffw_pool_backward / dffw_pool3_backward: on activation RECORDS (16-byte aligned), enqueue-only, one launch (dffw::pool_bwd_kernel /
 * dffw::pool3_bwd_kernel; dffw_last_op_kernels names it), no allocation.  dffw_op_*: the same on device fp32 tensors; allocates, poisons
 * its workspace with 0xFF and synchronises.  Anything not served is DFFW_EINVAL before any launch and before the GPU is touched. */
int dffw_pool_backward(int device, int precision, int mode, int k, const void *g, const void *x, const void *b, int B, int C, int N, int H,
                       int W, void *out, void *hip_stream);
int dffw_pool3_backward(int device, int precision, const void *g2, const void *g4, const void *g8, const void *b, int B, int C, int N, int H,
                        int W, void *out, void *hip_stream);
int dffw_op_pool_backward(int device, int precision, int mode, int k, const float *g, const float *x, const float *b, int B, int C, int N,
                          int H, int W, float *out, void *hip_stream);
int dffw_op_pool3_backward(int device, int precision, const float *g2, const float *g4, const float *g8, const float *b, int B, int C, int N,
                           int H, int W, float *out, void *hip_stream);

/* ---- backward of the stem ------------------------------------------------------------------------------------------------
 * The weight gradient of FM_measure.Focus_extraction.0.0, Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2), no bias), whose input is the
 * image stack: there is no data gradient.
 *   grad_w[co][ci][0][ky][kx] = sum over (b, n, y, x) of grad_y[b,co,n,y,x] * x[b,ci,n, y + 2 ky - 8, x + 2 kx - 8]   (zero outside the image)
 *   x        device fp32 (B,3,N,H,W) contiguous, the layout dffw_op_conv3d takes for the stem; rounded to the parts of `precision` in the kernel
 *   grad_w   (8, 3, 1, 9, 9) device fp32, by dffw::stem_wgrad_kernel + dffw::stem_wgrad_finish_kernel (dffw_last_op_kernels lists them):
 *            fp32 MFMA partials of at most 16 384 pixels, summed in float64 in a fixed order -- two calls give identical bits
 * dffw_stem_wgrad: enqueue-only, no allocation; grad_y an 8-channel activation RECORD [pixel][part][channel], 16-byte aligned (what
 * dffw_bn_train_backward writes); workspace: dffw_stem_wgrad_workspace_bytes(...) bytes, need not be cleared (0 for refused arguments; too
 * short: DFFW_ENOMEM).  dffw_op_stem_backward: grad_y (B,8,N,H,W) device fp32; allocates, poisons its workspace with 0xFF and synchronises.
 * A null pointer, a dimension below 1, an unknown precision or 2^31 pixels and more: DFFW_EINVAL before any launch and before the GPU is
 * touched. */
int64_t dffw_stem_wgrad_workspace_bytes(int B, int N, int H, int W);
int dffw_stem_wgrad(int device, int precision, const float *x, const void *grad_y, int B, int N, int H, int W, float *grad_w, void *workspace,
                    int64_t workspace_bytes, void *hip_stream);
int dffw_op_stem_backward(int device, int precision, const float *x, const float *grad_y, int B, int N, int H, int W, float *grad_w,
                          void *hip_stream);

/* ---- backward of the score convs, Cin -> 1 -------------------------------------------------------------------------------
 * The four convs that produce the fp32 score volumes dffw_loss_heads differentiates: classif1.0 / classif2.0 / classif3.0, Conv3d(Cin, 1, 1),
 * and confidence.2, Conv3d(32, 1, 3, padding=1).  Geometries: kernel (1,1,1) with pad 0, kernel (3,3,3) with pad (1,1,1); one output channel,
 * stride 1, dilation 1, no bias; Cin a multiple of 8 from 8 to 128; B, N, h, w >= 1 and fewer than 2^31 pixels.  Anything else, a null
 * pointer or a misaligned one: DFFW_EINVAL before any launch and before the GPU is touched.
 *   grad_score  device fp32 planar (B,N,h,w), exactly as dffw_loss_heads writes it (4-byte aligned); never rounded to records
 *   weight      DEVICE fp32 (1,Cin,kd,kh,kw), PyTorch layout
 *   grad_x[b,n,y,x,c]  = sum_k weight[c,k] grad_score[b, n+1-kz, y+1-ky, x+1-kx] (+ b[b,n,y,x,c]), taps outside the volume contribute 0.
 *                        k111: one fp32 rounding (fmaf(w, g, b), or w * g); k333: 27 fmaf in row-major tap order from 0, then + b in fp32;
 *                        then the one split into a record.  b, or NULL: a second gradient of the input; out may alias b.
 *   grad_w[c,k]        = sum over (b,n,y,x) of grad_score[b,n,y,x] * x[b, n+kz-1, y+ky-1, x+kx-1, c] at the STORED record of x (hi + lo in
 *                        split-bf16), summed in float64 (the products are exact there) per thread, workgroup and, in workgroup order, over
 *                        the grid; device fp32 (1,Cin,kd,kh,kw).  No atomics: two calls give identical bits; DFFW_SCORE_WGS (the launches'
 *                        workgroups, default 512) changes only the order of the float64 additions.
 * dffw_score_conv_dgrad (dffw::score_dgrad_kernel) and dffw_score_conv_wgrad (dffw::score_wgrad_kernel + dffw::score_wgrad_finish_kernel):
 * on activation RECORDS of Cin channels (16-byte aligned), enqueue-only, no allocation.  workspace: dffw_score_conv_wgrad_workspace_bytes(...)
 * = grid * Cin * taps float64, 8-byte aligned, need not be cleared (0 for refused arguments; too short: DFFW_ENOMEM).
 * dffw_op_score_conv_backward: x, b, grad_x (B,Cin,N,h,w) device fp32, grad_x / grad_w may each be NULL (with both NULL nothing is launched
 * and only the refusals are returned); allocates, poisons its workspace with 0xFF and synchronises.  dffw_last_op_kernels lists the launches. */
int dffw_score_conv_dgrad(int device, int precision, const float *grad_score, int B, int Cin, int N, int h, int w, const float *weight,
                          const int kernel[3], const int pad[3], const void *b, void *out, void *hip_stream);
int64_t dffw_score_conv_wgrad_workspace_bytes(int B, int Cin, int N, int h, int w, const int kernel[3], const int pad[3]);
int dffw_score_conv_wgrad(int device, int precision, const void *x, const float *grad_score, int B, int Cin, int N, int h, int w,
                          const int kernel[3], const int pad[3], float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream);
int dffw_op_score_conv_backward(int device, int precision, const float *x, int B, int Cin, int N, int h, int w, const float *weight,
                                const int kernel[3], const int pad[3], const float *grad_score, const float *b, float *grad_x, float *grad_w,
                                void *hip_stream);

/* ---- the Adam step -----------------------------------------------------------------------------------------------------------
 * What the reference's training scripts do after backward(): torch.optim.Adam(lr, betas=(0.9, 0.99)) without weight decay, amsgrad or gradient
 * scaling, for the WHOLE parameter list in a handful of launches of dffw::adam_kernel.  With t = step, the count after the increment (t >= 1):
 *     m' = beta1 m + (1 - beta1) g          v' = beta2 v + (1 - beta2) g^2
 *     d  = sqrt(v') / sqrt(1 - beta2^t) + eps          p' = p - (lr / (1 - beta1^t)) m' / d
 * The scalars are computed on the host in double and rounded once to fp32, as torch's single-tensor path has them; every element operation is
 * one fp32 rounding (correctly rounded sqrt and division, no fma contraction).  param, exp_avg and exp_avg_sq are updated in place, grad is only
 * read; NaN and Inf propagate and no step is skipped.  All pointers are device fp32, 4-byte aligned, of numel elements; a tensor whose four
 * pointers are 16-byte aligned moves in 16-byte accesses, any other element by element, with the same bits either way.
 * The list travels as the kernel's argument, at most dffw_adam_tensors_per_launch() tensors (and 2^34 elements) per launch; a longer list takes
 * several launches on hip_stream.  Enqueue-only: no device allocation, no copy, no synchronisation, no atomics.  A tensor's result does not depend
 * on its place in the list, the launch it lands in or the grid: passed alone it gives identical bits.  Tensors must not overlap.
 * DFFW_EINVAL before any launch and before the GPU is touched: tensors NULL or n_tensors < 1; numel < 0 or >= 2^31; a NULL pointer in an entry
 * with numel > 0; a pointer that is not 4-byte aligned; step < 1; lr, eps or a beta that is not finite; lr < 0, eps < 0, a beta outside [0, 1).
 * An entry with numel == 0 is skipped; a list of such entries only is DFFW_OK without a launch.  dffw_last_op_kernels names the kernel once per
 * launch. */
typedef struct dffw_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t numel;
} dffw_adam_tensor;
int dffw_adam_tensors_per_launch(void);
int dffw_adam_step(int device, const dffw_adam_tensor *tensors, int n_tensors, int64_t step, double lr, double beta1, double beta2, double eps,
                   void *hip_stream);

/* ---- backward of a conv over a channel concatenation ------------------------------------------------------------------------
 * The five convs of the aggregation network whose input is torch.cat([xa, xb], 1): dres2/3/4.conv0, SPP_module.combine1 and combine2.  One
 * geometry, so it is no argument: kernel (3,3,3), stride 1, pad (1,1,1), not transposed, no bias.  xa (Ca channels) and xb (Cb channels) share
 * one volume (B,N,H,W); Ca, Cb and Cout multiples of 8 from 8 to 128, Ca + Cb <= 192.  The concatenation is never materialised.
 *   grad_w   (Cout, Ca + Cb, 3,3,3) device fp32 = d<grad_y, conv(cat(xa, xb), weight)>/dweight by dffw::conv_wgrad_cat_kernel +
 *            dffw::conv_wgrad_finish_kernel (dffw_last_op_kernels lists them): the arithmetic of dffw_conv_wgrad, the footprint read from the
 *            two record tensors; where Ca + Cb <= 128 the bits are those of dffw_conv_wgrad on the concatenated records.
 *   grad_xa, grad_xb   two adjoint convs through the forward's own dispatch, on the weight's channels [0, Ca) and [Ca, Ca + Cb): each carries
 *            the bits a single adjoint conv would give that half.  A skip tensor's other gradient is added by dffw_grad_combine.
 * dffw_conv_cat_wgrad: enqueue-only on activation RECORDS (16-byte aligned), no allocation; workspace:
 * dffw_conv_cat_wgrad_workspace_bytes(...) bytes, 8-byte aligned, need not be cleared (0 for refused arguments; too short: DFFW_ENOMEM); for
 * Ca + Cb <= 128 it is dffw_conv_wgrad_workspace_bytes of the concatenation.  DFFW_EINVAL before any launch and before the GPU is touched, in
 * this order: an unknown precision; B, N, H or W below 1; Cout out of range; 2^31 units of 4 x 16 pixels and more; Ca or Cb out of range or
 * Ca + Cb > 192 (the message names both); a null pointer; a misaligned one.
 * dffw_op_conv_cat_backward: xa (B,Ca,N,H,W), xb (B,Cb,N,H,W), grad_y (B,Cout,N,H,W) device fp32; weight host fp32 (Cout, Ca + Cb, 3,3,3) (may
 * be NULL without grad_xa and grad_xb); grad_xa, grad_xb, grad_w device fp32 or NULL (with all three NULL nothing is launched and only the
 * refusals are returned); allocates, poisons its workspace with 0xFF and synchronises. */
int64_t dffw_conv_cat_wgrad_workspace_bytes(int B, int Ca, int Cb, int N, int H, int W, int Cout);
int dffw_conv_cat_wgrad(int device, int precision, const void *xa, int Ca, const void *xb, int Cb, int B, int N, int H, int W, const void *grad_y,
                        int Cout, float *grad_w, void *workspace, int64_t workspace_bytes, void *hip_stream);
int dffw_op_conv_cat_backward(int device, int precision, const float *xa, int Ca, const float *xb, int Cb, int B, int N, int H, int W,
                              const float *weight, int Cout, const float *grad_y, float *grad_xa, float *grad_xb, float *grad_w, void *hip_stream);

/* dffw_op_conv3d_cat: the FORWARD conv over the same virtual concatenation, one operator for the kernel tests (tests/test_gpu_conv_cat.py,
 * DESIGN.md §26): y = [relu](BN(conv3d(cat([xa, xb], 1), weight)) [+ residual]), kernel (3,3,3), stride 1, pad 1, not transposed -- the
 * geometry of the five layers whose input is two tensors (the hourglass conv0 layers, the pyramid's combine1 / combine2).  xa (B,Ca,N,H,W),
 * xb (B,Cb,N,H,W), residual (B,Cout,N,H,W) or NULL and y (B,Cout,N,H,W) device fp32; weight host fp32 (Cout, Ca + Cb, 3,3,3); bn, conv_bias,
 * relu as dffw_op_conv3d takes them.  One layer of Ca + Cb input channels is packed, each tensor is staged into activation records of its
 * own and the conv runs through the forward's own dispatch with the second tensor as ConvOpt::in1: the kernel choice, and the fill that reads
 * two tensors, are the forward's.  The concatenation is never materialised.  dffw_last_conv_kernel() names the launch.  Allocates, poisons
 * its workspace with 0xFF and synchronises.  DFFW_EINVAL with a message, before the GPU is touched: a null xa, xb, weight or y; a precision
 * outside 0..2; B, N, H or W below 1; Ca or Cb below 8 or no multiple of 8; Ca + Cb > 192; Cout below 8, above 128 or no multiple of 8. */
int dffw_op_conv3d_cat(int device, int precision, const float *xa, int Ca, const float *xb, int Cb, int B, int N, int H, int W,
                       const float *weight, int Cout, const float *bn, const float *conv_bias, const float *residual, int relu, float *y,
                       void *hip_stream);

/* ---- synthetic focal stacks (Simulator/synthetic_blur_movement.py:155-280) ---------------------------------------------
 * Replaces the reference's per-image NumPy / OpenCV loop that made End_to_End's training data: for every sample b an RGB-D
 * frame at working size (H, W) and a camera, N slices focused at 1/linspace(1/max_focus, 1/min_focus, N); slice n >= 1 is
 * warped by its field of view and a (beta, gamma) pixel shift; every pixel is blurred by the disk of its depth layer's
 * circle of confusion.  DESIGN.md §10 states the arithmetic contract (all float64 scalars and layer tables
 * as Python evaluates them; the warp as torch CPU float32; the disk blur as an exact integer sum rounded to nearest).
 * The defocus map follows NumPy >= 2 promotion (NEP 50): for n >= 1 the float32 warped depth meets the float64 focus distance
 * in float64 (the reference's pinned NumPy 1.21 would have computed it in float32).  Warped-out pixels give inf, as there. */
typedef struct dffw_sim_params {
    double pixel_per_meter;        /* args.pixel_vs_meter */
    double min_depth, max_depth;   /* depth normalisation: d' = max_depth*(d - min d)/(max d - min d) + min_depth */
    double min_focus, max_focus;   /* focus range in metres (the reference fixes 0.1, 0.9) */
    int num_planes;                /* depth planes scanned for the CoC layer table (args.num_planes) */
    int max_radius;                /* upper bound of every blur radius, or -1 if unknown.  Steers speed only: above
                                    * DFFW_SIM_LDS_RADIUS the global-memory kernel is launched; a tile whose radius exceeds
                                    * the LDS halo reads global memory in either kernel. */
} dffw_sim_params;
#define DFFW_SIM_LDS_RADIUS 32     /* largest blur radius the render kernel stages in LDS */
#define DFFW_SIM_DISCARD 1         /* status bit 0: the warped depth has a 0 minimum; the reference drops the sample (:274) */
/* per-slice scalars of dffw_sim_plan_host, in this order (FoV is 1 for slice 0, which is not warped) */
#define DFFW_SIM_NSCALARS 12
enum { DFFW_SIM_FD, DFFW_SIM_FD_PX, DFFW_SIM_LENS_TO_SENSOR, DFFW_SIM_FOV, DFFW_SIM_COC_SCALE, DFFW_SIM_F_PX, DFFW_SIM_LENS_DIA,
       DFFW_SIM_SCENE_MIN, DFFW_SIM_SCENE_MAX, DFFW_SIM_MIN_AFOV, DFFW_SIM_MAX_AFOV, DFFW_SIM_ORIGIN_MAX_AFOV };

/* Bytes of workspace dffw_sim_render needs. */
int64_t dffw_sim_workspace_bytes(int B, int N, int H, int W, int num_planes);

/* Enqueue-only on hip_stream; every pointer is device memory.
 *   cams       fp64 (B,4): focal length (m), F-number, alpha slope, alpha intercept of sample b's camera
 *   image      fp32 (B,H,W,3), 0..255, channel order as cv2 reads it
 *   depth      fp64 (B,H,W) raw depth (normalised inside; a constant map is outside the contract)
 *   shifts     fp64 (B,N,2) beta, gamma in pixels (already scaled by the size ratio); slice 0's entry is ignored
 *   images     uint8 (B,N,H,W,3): the blurred slices, channels reversed (the array the reference hands to imwrite)
 *   defocus    fp64 (B,N,H,W): |coc_scale*(d_px - fd_px)/d_px|
 *   depth_out  fp32 (B,H,W): normalised depth warped by the last slice's FoV and shift
 *   status     int32 (B): DFFW_SIM_DISCARD bits
 *   slices     fp64 (B,N,2) or NULL: focus distance (m) and FoV of every slice
 *   warped_tap fp32 (B,N,H,W,3) or NULL: the warped float image before the uint8 truncation (debug tap)
 * N >= 2, H, W >= 2, num_planes >= 1.  dffw_last_op_kernels() lists the launches. */
int dffw_sim_render(int device, dffw_sim_params params, const double *cams, const float *image, const double *depth,
                    const double *shifts, int B, int N, int H, int W, uint8_t *images, double *defocus, float *depth_out,
                    int32_t *status, double *slices, float *warped_tap, void *workspace, int64_t ws_bytes, void *hip_stream);

/* The same per-slice scalars and CoC layer tables on the CPU, from one camera and the raw depth's (min, max): scalars
 * (N, DFFW_SIM_NSCALARS); coc / lo / hi (N, num_planes), layer i of slice n = [lo, hi) blurred with radius |coc| (0 -> 1);
 * nlayers (N).  The device's plan kernel runs the same function. */
int dffw_sim_plan_host(const dffw_sim_params *params, const double cam[4], double dmin, double dmax, int N, double *scalars,
                       int *coc, double *lo, double *hi, int *nlayers);

/* Half-widths of the rows 0..r of the radius-r disk (cv2.circle filled, restated in DESIGN.md); returns the tap count K. */
int dffw_sim_disk_rows(int r, int *halfwidths);

/* ---- measured ceilings of the GPU at hand (bench.py prints them beside the datasheet peaks) -------------------------------
 * mfma_tflops: v_mfma_f32_16x16x32_bf16 issued back to back out of registers on every SIMD (no memory traffic);
 * hbm_gbs: float4 streaming (copy of 1 GiB with read + write counted, or a pure read of 2 GiB: the better).  Synchronises;
 * allocates 2 GiB for the duration of the call. */
int dffw_probe_peaks(int device, float *mfma_tflops, float *hbm_gbs, void *hip_stream);

/* ---- multi-GPU: RCCL all-gather of the depth maps ---------------------------------------------
 * The forward has no cross-sample operation, so a batch is sharded on dim 0 over the GPUs of a node with no data-path
 * collective; what the reference's nn.DataParallel does after the replicas finish (Depth_Estimation_Test/test.py:32:
 * gather the outputs on device 0) becomes ONE ncclAllGather (RCCL over xGMI) of every rank's (b,H,W) fp32 maps, enqueued
 * on the compute stream behind the last head kernel.  librccl.so is bound with dlopen at the first call (override the
 * path with the environment variable DFFW_RCCL_LIB); nothing here is needed for single-GPU use.
 *   one process per GPU:  rank 0 calls dffw_comm_unique_id and hands the 128 bytes to the other ranks (file, pipe, MPI ...);
 *                         every rank calls dffw_comm_init_rank(device, nranks, rank, id, &comm)
 *   one process, n GPUs:  dffw_comm_init_all(n, devices, comms); calls for several comms from one thread go between
 *                         dffw_comm_group_start / dffw_comm_group_end
 *   dffw_allgather        recv[r*count .. (r+1)*count) on every rank = rank r's send[0 .. count) (device fp32); equal
 *                         counts on all ranks; enqueue-only on hip_stream. */
#define DFFW_COMM_ID_BYTES 128
typedef struct dffw_comm dffw_comm;
int dffw_comm_unique_id(char id[DFFW_COMM_ID_BYTES]);
int dffw_comm_init_rank(int device, int nranks, int rank, const char id[DFFW_COMM_ID_BYTES], dffw_comm **out);
int dffw_comm_init_all(int ndev, const int *devices, dffw_comm **out /* [ndev] */);
void dffw_comm_destroy(dffw_comm *c);
int dffw_comm_rank(const dffw_comm *c);
int dffw_comm_size(const dffw_comm *c);
int dffw_allgather(dffw_comm *c, const float *send, float *recv, int64_t count, void *hip_stream);
int dffw_comm_group_start(void);
int dffw_comm_group_end(void);

#ifdef __cplusplus
}
#endif
#endif /* DFFW_H */
