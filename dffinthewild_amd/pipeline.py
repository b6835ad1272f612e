"""Input and output side of the forward on the GPU: host-side mirror of what the
reference's loaders and scripts do in NumPy around `model(FS, focus_dists)`.

    FS = pack_stack(raw_u8, "NHWC")                       # test_Dataloader.py:121-141: /127.5-1, transpose, pad to x32 with -1
    FS, gt, mask = augment_stack(raw_u8, "HWCN", gt=gt, **train_seeds(rng, B))   # train_Dataloader.py + augmentation.py: a training sample
    fd = focus_dists(values, B)                           # (B,N,1,1): broadcast instead of np.tile(..., [1,H,W]) (test_Dataloader.py:24)
    _, _, _, pred3 = model(FS, fd)
    rgb = colorize(pred3, size=(H, W), vrange=(lo, hi))   # test.py:124-133;  vrange=None: test_real_scenes.py:40-52
    m = masked_metrics(pred3, gt, mask)                   # metrics.py:90-127 as called from test.py:144-158

Everything stays in device memory; the kernels live in libdffw.so (csrc/dffw_io.hip, csrc/dffw_aug.hip) and are reached through the C ABI
(include/dffw.h: dffw_pack_stack, dffw_augment_stack, dffw_colorize, dffw_metrics).  No CPU fallback: CPU tensors raise."""
from ctypes import c_void_p, c_int64

import numpy as np
import torch

from . import engine
from .engine import lib, _check, _stream_ptr

# element order of every source layout the reference's loaders build, as (slice, row, col, channel) axis positions
_LAYOUTS = {
    "NHWC": (0, 1, 2, 3),   # hdf5 stacks (N,H,W,3): DDFF test_Dataloader.py:121, HCI :78
    "HWCN": (3, 0, 1, 2),   # image arrays (H,W,3,N): FS6 test_Dataloader.py:31-35, Real_Scenes Test_dataloader.py:24
    "HWNC": (2, 0, 1, 3),   # image arrays (H,W,N,3): Smartphone test_Dataloader.py:197
}
METRIC_NAMES = ("valid", "abs_rel", "sq_rel", "mse", "mae", "rmse", "rmse_log", "accuracy_1", "accuracy_2", "accuracy_3",
                "mse_w_conf", "mae_w_conf")


def _dev(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor: dffinthewild_amd has no CPU path")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _norm_flag(norm):
    if norm not in ("f32", "f64"):
        raise ValueError(f"norm must be 'f32' or 'f64', got {norm!r}")
    return engine.RAW_NORM_F64 if norm == "f64" else 0


def pack_stack(raw, layout="NHWC", crop=None, multiple=32, norm="f32"):
    """raw: uint8 or float32 (0..255) CUDA tensor in `layout`, with or without a leading batch dim (any strides: a
    view of a larger buffer is fine).  crop = (y0, x0, h, w).  Returns float32 (B,3,N,Hp,Wp) = raw/127.5-1, padded at
    the bottom/right to multiples of 32 with -1: the tensor the reference's loaders hand to the model.
    norm="f32": float32 divide then subtract (the DDFF / HCI / Smartphone / Real_Scenes loaders); norm="f64": the FS6 /
    DefocusNet loader's arithmetic (test_Dataloader.py:31-39 builds a float64 array, torch.Tensor() rounds once)."""
    nflag = _norm_flag(norm)
    if layout not in _LAYOUTS:
        raise ValueError(f"unknown layout {layout!r} (one of {sorted(_LAYOUTS)})")
    dev = _dev(raw, "raw stack")
    if raw.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"raw stack must be uint8 or float32, got {raw.dtype}")
    if raw.dim() == 4:
        raw = raw.unsqueeze(0)
    if raw.dim() != 5:
        raise ValueError(f"raw stack must have 4 or 5 dims, got {tuple(raw.shape)}")
    an, ay, ax, ac = (1 + a for a in _LAYOUTS[layout])
    if raw.shape[ac] != 3:
        raise ValueError(f"layout {layout}: expected 3 colour channels on axis {ac}, got {raw.shape[ac]}")
    B, N, H, W = raw.shape[0], raw.shape[an], raw.shape[ay], raw.shape[ax]
    y0, x0, h, w = (0, 0, H, W) if crop is None else crop
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(f"crop {crop} does not fit the {H}x{W} source")
    Hp, Wp = -(-h // multiple) * multiple, -(-w // multiple) * multiple
    st = raw.stride()
    strides = (c_int64 * 5)(st[0], st[an], st[ay], st[ax], st[ac])
    off = (y0 * st[ay] + x0 * st[ax]) * raw.element_size()
    FS = torch.empty((B, 3, N, Hp, Wp), dtype=torch.float32, device=raw.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_pack_stack(dev, c_void_p(raw.data_ptr() + off), (0 if raw.dtype == torch.uint8 else 1) | nflag, strides, B, N, h, w,
                                   Hp, Wp, c_void_p(FS.data_ptr()), _stream_ptr(dev)), "dffw_pack_stack")
    return FS


def train_seeds(rng, batch, cropping=None):
    """The random draws of the training loaders' get_seeds() (train_Dataloader.py:80,141,215,268,379) for `batch` samples, in the
    reference's order, from a random.Random (or the random module): with cropping=(cy, cx) first randint(0, cy-1), randint(0, cx-1),
    then uniform(0.4,1.6), uniform(-0.1,0.1), uniform(0.5,2.0), uniform(0,1), uniform(0,1), randint(0,3).  Returns the keyword
    arguments of augment_stack as a dict of per-sample lists (crop: (y0, x0) pairs; the caller adds size=)."""
    out = {k: [] for k in ((("crop",) if cropping is not None else ()) + ("contrast", "brightness", "gamma", "flip_x", "flip_y", "angle"))}
    for _ in range(batch):
        if cropping is not None:
            y0 = rng.randint(0, cropping[0] - 1)
            out["crop"].append((y0, rng.randint(0, cropping[1] - 1)))
        out["contrast"].append(rng.uniform(0.4, 1.6))
        out["brightness"].append(rng.uniform(-0.1, 0.1))
        out["gamma"].append(rng.uniform(0.5, 2.0))
        out["flip_x"].append(rng.uniform(0, 1.0))
        out["flip_y"].append(rng.uniform(0, 1.0))
        out["angle"].append(rng.randint(0, 3))
    return out


def _per_sample(v, B, what):
    """One float per sample from a scalar, a sequence of length B (or 1) or a tensor (a device tensor is read back: one
    synchronisation; pass host values to stay enqueue-only)."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().reshape(-1).tolist()
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, B)
    if a.size != B:
        raise ValueError(f"{what}: expected one value or {B}, got {a.size}")
    return a


def augment_stack(raw, layout="NHWC", *, contrast, brightness, gamma, flip_x, flip_y, angle, crop=None, size=None, norm="f32",
                  gt=None, conf=None, gt_range=None, sentinel=0.0):
    """What the reference's training loaders do to a decoded sample (train_Dataloader.py with augmentation.py): crop, the photometric
    chain image_augmentation(x, contrast, brightness, gamma), horizontal flip (flip_x > 0.5), vertical flip (flip_y > 0.5), np.rot90 by
    `angle` quarter turns, the ground-truth range rule and the transpose to (3,N,h,w) float32, on the GPU.

    raw: as for pack_stack (uint8 or float32 0..255, `layout`, optional batch dim, any strides).  contrast ... angle: one value per
    sample (scalar, sequence of length B, or tensor); the flips take the loaders' uniform draws or booleans.  crop: (y0, x0) for all or
    one pair per sample, with size=(h, w) the window (default: the whole image).  norm: "f32" for the loaders that hold float32 arrays
    (DDFF, HCI, Smartphone), "f64" for FS6 / FlyingThings (float64 chain, rounded once).
    Returns FS float32 (B,3,N,h',w') with (h',w') = (h,w), or (w,h) for odd angles (h != w: all angles of a batch need one parity).
    gt / conf: float (B,H,W) at source size.  Then returns (FS, gt, mask[, conf]) in the same crop and pose: gt float32 with values
    < gt_range[0] or > gt_range[1] set to `sentinel` (gt_range=None: no rule), mask bool = (gt != sentinel) (NaN counts as valid)."""
    nflag = _norm_flag(norm)
    if layout not in _LAYOUTS:
        raise ValueError(f"unknown layout {layout!r} (one of {sorted(_LAYOUTS)})")
    dev = _dev(raw, "raw stack")
    if raw.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"raw stack must be uint8 or float32, got {raw.dtype}")
    if raw.dim() == 4:
        raw = raw.unsqueeze(0)
    if raw.dim() != 5:
        raise ValueError(f"raw stack must have 4 or 5 dims, got {tuple(raw.shape)}")
    an, ay, ax, ac = (1 + a for a in _LAYOUTS[layout])
    if raw.shape[ac] != 3:
        raise ValueError(f"layout {layout}: expected 3 colour channels on axis {ac}, got {raw.shape[ac]}")
    B, N, H, W = raw.shape[0], raw.shape[an], raw.shape[ay], raw.shape[ax]
    h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
    if h < 1 or w < 1 or h > H or w > W:
        raise ValueError(f"window {h}x{w} does not fit the {H}x{W} source")
    if isinstance(crop, torch.Tensor):
        crop = crop.detach().cpu().tolist()
    origin = np.asarray((0, 0) if crop is None else crop, dtype=np.int64).reshape(-1, 2)
    if origin.shape[0] == 1:
        origin = np.repeat(origin, B, axis=0)
    if origin.shape[0] != B:
        raise ValueError(f"crop: expected one (y0, x0) pair or {B}, got {origin.shape[0]}")
    if (origin < 0).any() or (origin[:, 0] + h > H).any() or (origin[:, 1] + w > W).any():
        raise ValueError(f"crop {origin.tolist()} with window {h}x{w} does not fit the {H}x{W} source")
    rec = np.empty((B, engine.AUG_NPARAMS), dtype=np.float64)
    rec[:, 0:2] = origin
    for k, (v, what) in enumerate(((contrast, "contrast"), (brightness, "brightness"), (gamma, "gamma"), (flip_x, "flip_x"),
                                   (flip_y, "flip_y"), (angle, "angle")), start=2):
        rec[:, k] = _per_sample(v, B, what)
    turns = rec[:, 7]
    if (turns != np.floor(turns)).any():
        raise ValueError(f"angle must be whole quarter turns, got {turns.tolist()}")
    rec[:, 7] = turns = np.mod(turns, 4)
    odd = (turns.astype(np.int64) & 1).astype(bool)
    if h != w and odd.any() and not odd.all():
        raise ValueError(f"a batch with a {h}x{w} window needs angles of one parity (the output has one shape), got {turns.tolist()}")
    transposed = bool(odd.all())
    oh, ow = (w, h) if transposed else (h, w)
    labels = []
    for name, t in (("gt", gt), ("conf", conf)):
        if t is None:
            labels.append(None)
            continue
        if _dev(t, name) != dev:
            raise ValueError(f"{name} is on another device")
        t = t.unsqueeze(0) if t.dim() == 2 else t
        if tuple(t.shape) != (B, H, W):
            raise ValueError(f"{name} must be ({B}, {H}, {W}) like the source, got {tuple(t.shape)}")
        labels.append(t.to(torch.float32).contiguous())
    gt32, conf32 = labels
    if conf32 is not None and gt32 is None:
        raise ValueError("conf needs gt")
    lo, hi = (-np.inf, np.inf) if gt_range is None else (-np.inf if gt_range[0] is None else gt_range[0], np.inf if gt_range[1] is None else gt_range[1])
    params = torch.from_numpy(rec).to(raw.device)
    st = raw.stride()
    strides = (c_int64 * 5)(st[0], st[an], st[ay], st[ax], st[ac])
    FS = torch.empty((B, 3, N, oh, ow), dtype=torch.float32, device=raw.device)
    gt_out = mask = conf_out = None
    if gt32 is not None:
        gt_out = torch.empty((B, oh, ow), dtype=torch.float32, device=raw.device)
        mask = torch.empty((B, oh, ow), dtype=torch.bool, device=raw.device)
    if conf32 is not None:
        conf_out = torch.empty((B, oh, ow), dtype=torch.float32, device=raw.device)
    ptr = lambda t: c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    with torch.cuda.device(dev):
        _check(lib.dffw_augment_stack(dev, c_void_p(raw.data_ptr()), (0 if raw.dtype == torch.uint8 else 1) | nflag, strides, B, N, H, W, h, w,
                                      ptr(params), int(transposed), ptr(FS), ptr(gt32), ptr(conf32), ptr(gt_out), ptr(mask), ptr(conf_out),
                                      0 if gt_range is None else 1, float(np.float32(lo)), float(np.float32(hi)), float(np.float32(sentinel)),
                                      _stream_ptr(dev)), "dffw_augment_stack")
    if gt32 is None:
        return FS
    return (FS, gt_out, mask) + ((conf_out,) if conf32 is not None else ())


def focus_dists(values, batch=1, device="cuda"):
    """(batch,N,1,1) float32 focus distances: the forward broadcasts them over the map, so the (N,H,W) tile of
    test_Dataloader.py:24,71,113,166 is never materialised."""
    v = torch.as_tensor(values, dtype=torch.float32, device=device).reshape(1, -1, 1, 1)
    return v.expand(batch, -1, -1, -1).contiguous()


def real_scene_crop(height, width):
    """(y0, x0, h, w) of the border crop End_to_End/Test_dataloader.py:20-23 applies to every slice (1/12 of each side, integer
    division) - the `crop=` argument of pack_stack."""
    cy, cx = height // 12, width // 12
    if cy < 1 or cx < 1:
        raise ValueError(f"the loader's [c:-c] crop is empty for a {height}x{width} image")    # NumPy: x[0:-0] is empty
    return cy, cx, height - 2 * cy, width - 2 * cx


def real_scene_inputs(focus_distances, focal_length, device="cuda"):
    """The two small inputs of End_to_End.Network besides the stack, from the values of a scene's focus_distance.txt /
    focal_length.txt, as End_to_End/Test_dataloader.py:37-53 builds them (float64 arithmetic, rounded to float32 by torch.Tensor)
    and the batch-1 DataLoader of test_real_scenes.py:24 stacks them:
        focus_dists  (1,N,1,1) float32 = 1 / d          relative_fov  (1,1,N,1,1) float32 = (1/f - 1/d) / min(1/f - 1/d)"""
    d = np.asarray([float(v) for v in focus_distances], dtype=np.float64)
    if d.ndim != 1 or d.size < 1:
        raise ValueError("focus_distances must be a non-empty sequence")
    rel = 1 / float(focal_length) - 1 / d
    rel = rel / np.min(rel)
    fd = torch.from_numpy((1 / d).astype(np.float32)).reshape(1, -1, 1, 1).to(device)
    fov = torch.from_numpy(rel.astype(np.float32)).reshape(1, 1, -1, 1, 1).to(device)
    return fd, fov


def unpack_stack(warp, size=None):
    """The aligned stack End_to_End.Network returns, (B,3,N,H,W) float32 CUDA in [-1,1] -> uint8 (B,N,h,w,3) slice images:
    `127.5 * (warp + 1.0)` truncated to uint8, cropped to size=(h, w), channel order kept (test_real_scenes.py:42-47)."""
    dev = _dev(warp, "warp")
    if warp.dim() != 5 or warp.shape[1] != 3 or warp.dtype != torch.float32:
        raise ValueError(f"warp must be float32 (B,3,N,H,W), got {warp.dtype} {tuple(warp.shape)}")
    x = warp.contiguous()
    B, _, N, H, W = x.shape
    h, w = (H, W) if size is None else size
    img = torch.empty((B, N, h, w, 3), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_unpack_stack(dev, c_void_p(x.data_ptr()), B, N, H, W, h, w, c_void_p(img.data_ptr()), _stream_ptr(dev)), "dffw_unpack_stack")
    return img


def colorize(depth, size=None, vrange=None, return_range=False):
    """depth (B,H,W) or (H,W) float32 CUDA -> uint8 (B,h,w,3) RGB through matplotlib's 'jet' semantics.
    vrange=(lo, hi): fixed normalisation range (test.py:130-132); None: each map's own min/max over the whole padded
    map (test_real_scenes.py:40).  size=(h, w): crop (test.py:124-126, test_real_scenes.py:52)."""
    dev = _dev(depth, "depth")
    squeeze = depth.dim() == 2
    d = depth.unsqueeze(0) if squeeze else depth
    if d.dim() != 3 or d.dtype != torch.float32:
        raise ValueError(f"depth must be float32 (B,H,W), got {d.dtype} {tuple(d.shape)}")
    d = d.contiguous()
    B, H, W = d.shape
    h, w = (H, W) if size is None else size
    rng = torch.empty((B, 2), dtype=torch.float32, device=d.device)
    rgb = torch.empty((B, h, w, 3), dtype=torch.uint8, device=d.device)
    lo, hi = (0.0, 0.0) if vrange is None else (float(vrange[0]), float(vrange[1]))
    with torch.cuda.device(dev):
        _check(lib.dffw_colorize(dev, c_void_p(d.data_ptr()), B, H, W, h, w, 1 if vrange is None else 0, lo, hi,
                                 c_void_p(rng.data_ptr()), c_void_p(rgb.data_ptr()), _stream_ptr(dev)), "dffw_colorize")
    rgb = rgb[0] if squeeze else rgb
    return (rgb, rng) if return_range else rgb


def masked_metrics(est, gt, mask, conf=None):
    """est (B,H,W) float32 (pred3, still padded), gt (B,h,w) float32, mask (B,h,w) bool/uint8, conf (B,h,w) float32 or
    None.  Returns a float64 CUDA tensor (B,12) in METRIC_NAMES order (metrics.py:90-127)."""
    dev = _dev(est, "est")
    for name, t in (("gt", gt), ("mask", mask)) + ((("conf", conf),) if conf is not None else ()):
        if _dev(t, name) != dev:
            raise ValueError(f"{name} is on another device")
    if est.dim() == 2:
        est, gt, mask = est.unsqueeze(0), gt.unsqueeze(0), mask.unsqueeze(0)
        conf = conf.unsqueeze(0) if conf is not None else None
    est, gt = est.contiguous(), gt.contiguous().float()
    mask = mask.contiguous().to(torch.uint8)
    B, H, W = est.shape
    h, w = gt.shape[-2:]
    if mask.shape != gt.shape or (conf is not None and conf.shape != gt.shape) or gt.shape[0] != B:
        raise ValueError("gt / mask / conf shapes differ")
    conf = conf.contiguous().float() if conf is not None else None
    out = torch.empty((B, len(METRIC_NAMES)), dtype=torch.float64, device=est.device)
    nbytes = lib.dffw_metrics_scratch_bytes(B)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=est.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_metrics(dev, c_void_p(est.data_ptr()), B, H, W, c_void_p(gt.data_ptr()), c_void_p(mask.data_ptr()),
                                c_void_p(conf.data_ptr()) if conf is not None else None, h, w, c_void_p(out.data_ptr()),
                                c_void_p(scratch.data_ptr()), nbytes, _stream_ptr(dev)), "dffw_metrics")
    return out


# ---- training loss and regression-head backward (first link) ---------------------------------------------
HEAD_WEIGHTS = (0.3, 0.5, 0.7, 1.0)   # mid_out, pred1, pred2, pred3: train_code_*.py


def _loss_mask(mask):
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise ValueError(f"mask must be bool or uint8, got {mask.dtype}")
    return mask


def training_loss(scores, focus_dists, gt, mask, conf=None, weights=HEAD_WEIGHTS, depth_range=None, grads=True):
    """The loss of the reference's training scripts on the four score volumes (conf, cost1, cost2, cost3 of the forward's taps), and its
    gradient with respect to them:

        Loss_k = sum(conf * ((d_k - gt)/r)^2 over mask) / sum(conf over mask),   total = sum_k weights[k] * Loss_k

    with d_k the k-th regression head's depth map, r = hi - lo of depth_range (FlyingThings (10, 100), Smartphone (1/3.91092, 1/0.10201))
    or 1, conf = 1 when None (then Loss_k is nn.MSELoss over est[mask]).  mask: bool or uint8.  An empty mask gives NaN losses and zero
    gradients, as torch does on an empty selection.  Returns (total, per_head, preds, grads): float64 scalar, float64 (len(scores),),
    list of (B,H,W) depth maps, list of gradients shaped like the scores (None with grads=False).  All device tensors; nothing syncs."""
    _dev(scores[0], "score volumes")
    losses, preds, g = engine.op_loss_heads(list(scores), focus_dists.float(), gt, _loss_mask(mask), conf, weights, depth_range, grads=grads)
    return losses[-1], losses[:-1], preds, g


class HeadsLoss(torch.autograd.Function):
    """total = HeadsLoss.apply(conf_score, cost1, cost2, cost3, focus_dists, gt, mask, conf, weights, depth_range): the total training loss
    (float32 scalar) as an autograd node, so that any PyTorch producer of the four score volumes trains against the HIP heads.  The gradients
    are computed in the forward launch and scaled by the incoming gradient in backward; the non-score arguments get None."""

    @staticmethod
    def forward(ctx, s0, s1, s2, s3, focus_dists, gt, mask, conf=None, weights=HEAD_WEIGHTS, depth_range=None):
        total, _, _, g = training_loss([s0.detach(), s1.detach(), s2.detach(), s3.detach()], focus_dists, gt, mask, conf, weights, depth_range)
        ctx.save_for_backward(*g)
        return total.float()

    @staticmethod
    def backward(ctx, grad_out):
        return tuple(g * grad_out for g in ctx.saved_tensors) + (None,) * 6


# ---- the regression heads as a differentiable node of their own ------------------------------------------------
def _head_scale(score, H, W):
    """s in (1, 2, 4, 8) with (H, W) = s * the score's size: the heads the backward serves; None for any other size."""
    h, w = score.shape[-2:]
    return next((s for s in (1, 2, 4, 8) if h * s == H and w * s == W), None)


class RegressHeads(torch.autograd.Function):
    """maps = RegressHeads.apply(focus_dists, (H, W), *scores): the depth maps of 1..4 regression heads (engine.op_regress_heads, the bits of the
    inference forward) as an autograd node; backward is engine.op_heads_backward for the heads that received a gradient.  focus_dists is
    data: it gets no gradient.  backward_kernels: engine.op_kernels() of the last backward, read on the thread that launched it (autograd
    runs the backward of GPU tensors on a thread of its own, and dffw_last_op_kernels is per thread, so the caller's op_kernels() cannot see it)."""

    backward_kernels = []

    @staticmethod
    def forward(ctx, focus_dists, size, *scores):
        _dev(scores[0], "score volumes")
        H, W = size
        if ctx.needs_input_grad[0]:
            raise ValueError("regress_heads: focus_dists is data, it has no gradient here (requires_grad is set)")
        for k, s in enumerate(scores):
            if ctx.needs_input_grad[2 + k] and _head_scale(s, H, W) is None:
                raise ValueError(f"regress_heads: scores[{k}] requires grad at {s.shape[-2]}x{s.shape[-1]}, which is not {H}x{W} divided by 1, 2, 4 "
                                 f"or 8: the backward does not serve it")
        ctx.set_materialize_grads(False)
        ctx.size = (H, W)
        ctx.save_for_backward(focus_dists, *scores)
        return tuple(engine.op_regress_heads([s.detach().float() for s in scores], focus_dists.float(), H, W))

    @staticmethod
    def backward(ctx, *grad_maps):
        focus_dists, *scores = ctx.saved_tensors
        H, W = ctx.size
        live = [k for k, (g, need) in enumerate(zip(grad_maps, ctx.needs_input_grad[2:])) if g is not None and need]
        grads, RegressHeads.backward_kernels = [None] * len(scores), []
        if live:   # only these heads go to the library: the others may have a size the backward does not serve
            got = engine.op_heads_backward([scores[k].detach().float() for k in live], focus_dists.float(),
                                           [grad_maps[k].contiguous().float() for k in live], H, W)
            RegressHeads.backward_kernels = engine.op_kernels()
            for k, g in zip(live, got):
                grads[k] = g
        return (None, None) + tuple(g.to(s.dtype) if g is not None else None for g, s in zip(grads, scores))


def regress_heads(scores, focus_dists, size=None):
    """The depth maps (B,H,W) of 1 to 4 score volumes (B,N,h_k,w_k) as a tuple that carries a gradient: bilinear upsample to `size` (default:
    the largest score's size), softplus + 1e-6, normalisation over the slices, sum of focus_dists * p.  Any loss written in PyTorch on the maps
    differentiates through the HIP backward down to the scores; heads the loss does not use are not launched.  The forward takes any
    score size; a score that requires grad must be (H,W) divided by 1, 2, 4 or 8.  focus_dists: broadcastable to (B,N,H,W), no gradient."""
    scores = tuple(scores)
    if not 1 <= len(scores) <= 4:
        raise ValueError(f"regress_heads: 1 to 4 score volumes, got {len(scores)}")
    if size is None:
        size = (max(s.shape[-2] for s in scores), max(s.shape[-1] for s in scores))
    return RegressHeads.apply(focus_dists, (int(size[0]), int(size[1])), *scores)


def _xw_backward(ctx, op, x, weight, grad, **kw):
    """(grad_x, grad_w) of a conv node whose first two inputs are x and the weight: ``op`` (an engine.op_*_backward) computes those autograd
    asks for, and the weight's gradient goes to the weight's device and dtype."""
    need = tuple(n for n, on in zip(("x", "w"), ctx.needs_input_grad[:2]) if on)
    gx, gw = op(x, weight, grad, need=need, **kw)
    return gx, gw.to(weight.device, weight.dtype) if gw is not None else None


# ---- conv backward: one plain conv of the aggregation network as an autograd node ----------------------------------------
class Conv3d(torch.autograd.Function):
    """y = Conv3d.apply(x, weight, stride, pad, transposed, precision): the plain conv (no BN, bias or ReLU) through engine.op_conv3d, its
    backward through engine.op_conv3d_backward (the adjoint conv on the forward's dispatch for x, the conv_wgrad kernels for the weight), or,
    for the kernels (3,1,1) and (1,1,1), through engine.op_conv_pw_backward (the conv_pw_wgrad kernels)."""

    @staticmethod
    def forward(ctx, x, weight, stride=1, pad=0, transposed=False, precision="bf16x3"):
        _dev(x, "x")
        ctx.save_for_backward(x, weight)
        ctx.geom = (stride, pad, transposed, precision)
        return engine.op_conv3d(x.detach().float(), weight, stride=stride, pad=pad, transposed=transposed, precision=precision)

    @staticmethod
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        stride, pad, transposed, precision = ctx.geom
        if tuple(weight.shape[2:]) in ((3, 1, 1), (1, 1, 1)):
            if transposed:
                raise ValueError(f"conv3d backward: a transposed {tuple(weight.shape[2:])} conv is not served")
            gx, gw = _xw_backward(ctx, engine.op_conv_pw_backward, x, weight, grad_y, pad=pad, stride=stride, precision=precision)
        else:
            gx, gw = _xw_backward(ctx, engine.op_conv3d_backward, x, weight, grad_y, stride=stride, pad=pad, transposed=transposed, precision=precision)
        return gx, gw, None, None, None, None


def conv3d(x, weight, *, stride=1, pad=0, transposed=False, precision="bf16x3"):
    """conv(x, weight) on the HIP kernels with gradients for both: x (B,Cin,N,H,W) float32 CUDA, weight in PyTorch layout (CPU or CUDA).  The
    geometries are those of engine.op_conv3d_backward (3x3x3 and 1x3x3 stride 1, 3x3x3 stride (1,2,2), the transposed 3x3x3) and of
    engine.op_conv_pw_backward (3x1x1 with pad (1,0,0) and 1x1x1, stride 1), channels multiples of 8 up to 128.  With training_loss / HeadsLoss behind it a score
    volume's gradient flows one layer further in the caller's autograd graph."""
    return Conv3d.apply(x, weight, stride, pad, transposed, precision)


# ---- a conv over a channel concatenation: dres2/3/4.conv0, SPP_module.combine1 / combine2 --------------------------------
class ConvCat3d(torch.autograd.Function):
    """y = ConvCat3d.apply(xa, xb, weight, precision): the 3x3x3 stride-1 pad-1 conv of cat([xa, xb], 1) through engine.op_conv3d; its backward
    through engine.op_conv_cat_backward, which reads the two tensors as they are: two adjoint convs for xa and xb, the conv_wgrad_cat kernels
    for the weight (up to 128 + 64 = 192 input channels, which Conv3d's backward refuses)."""

    @staticmethod
    def forward(ctx, xa, xb, weight, precision="bf16x3"):
        _dev(xa, "xa")
        _dev(xb, "xb")
        ctx.save_for_backward(xa, xb, weight)
        ctx.precision = precision
        return engine.op_conv3d(torch.cat([xa.detach().float(), xb.detach().float()], 1), weight, stride=1, pad=1, precision=precision)

    @staticmethod
    def backward(ctx, grad_y):
        xa, xb, weight = ctx.saved_tensors
        need = tuple(n for n, on in zip(("xa", "xb", "w"), ctx.needs_input_grad[:3]) if on)
        gxa, gxb, gw = engine.op_conv_cat_backward(xa, xb, weight, grad_y, precision=ctx.precision, need=need)
        return gxa, gxb, gw.to(weight.device, weight.dtype) if gw is not None else None, None


def conv3d_cat(xa, xb, weight, *, precision="bf16x3"):
    """conv(cat([xa, xb], 1), weight) on the HIP kernels with gradients for all three: xa (B,Ca,N,H,W) and xb (B,Cb,N,H,W) float32 CUDA, weight
    (Cout,Ca+Cb,3,3,3) in PyTorch layout (CPU or CUDA); stride 1, pad 1, no bias.  Ca, Cb and Cout multiples of 8 from 8 to 128, Ca + Cb <= 192:
    the hourglasses' conv0 and the pyramid's combine1 / combine2.  The forward is bit for bit conv3d on the concatenation."""
    if xa.dim() != 5 or xb.dim() != 5 or weight.dim() != 5:
        raise ValueError("conv3d_cat: xa, xb and weight must have 5 dimensions")
    if (xa.shape[0], *xa.shape[2:]) != (xb.shape[0], *xb.shape[2:]):
        raise ValueError(f"conv3d_cat: xa {tuple(xa.shape)} and xb {tuple(xb.shape)} differ outside the channel axis")
    if tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"conv3d_cat: the conv over a concatenation is 3x3x3 stride 1 pad 1, got a {tuple(weight.shape[2:])} kernel")
    if weight.shape[1] != xa.shape[1] + xb.shape[1]:
        raise ValueError(f"conv3d_cat: weight {tuple(weight.shape)} does not take {xa.shape[1]} + {xb.shape[1]} input channels")
    return ConvCat3d.apply(xa, xb, weight, precision)


# ---- the score convs: Cin -> 1, the convs whose outputs the loss heads read --------------------------------------------
class ScoreConv(torch.autograd.Function):
    """s = ScoreConv.apply(x, weight, pad, precision): a conv with ONE output channel (classif1.0 / classif2.0 / classif3.0: 1x1x1;
    confidence.2: 3x3x3 pad 1; no bias) through engine.op_conv3d, which returns the fp32 score volume (B,N,h,w); its backward through
    engine.op_score_conv_backward (the score_dgrad / score_wgrad kernels): the score gradient stays fp32 planar, as HeadsLoss hands it over."""

    @staticmethod
    def forward(ctx, x, weight, pad=0, precision="bf16x3"):
        _dev(x, "x")
        ctx.save_for_backward(x, weight)
        ctx.geom = (pad, precision)
        return engine.op_conv3d(x.detach().float(), weight, stride=1, pad=pad, precision=precision)

    @staticmethod
    def backward(ctx, grad_score):
        x, weight = ctx.saved_tensors
        pad, precision = ctx.geom
        return _xw_backward(ctx, engine.op_score_conv_backward, x, weight, grad_score, pad=pad, precision=precision) + (None, None)


def score_conv(x, weight, *, pad=0, precision="bf16x3"):
    """The score volume (B,N,h,w) of a conv with one output channel, with gradients for x and weight: x (B,Cin,N,h,w) float32 CUDA, weight
    (1,Cin,1,1,1) with pad 0 or (1,Cin,3,3,3) with pad 1 (CPU or CUDA), Cin a multiple of 8 up to 128.  With HeadsLoss behind it and conv3d /
    batch_norm3d in front, the real head chain trains."""
    if weight.dim() != 5 or weight.shape[0] != 1:
        raise ValueError(f"score_conv: weight {tuple(weight.shape)} is not a conv with one output channel")
    return ScoreConv.apply(x, weight, pad, precision)


# ---- the stem: the dilated 1x9x9 conv of the image stack, with a gradient for its weight ---------------------------------
class StemConv(torch.autograd.Function):
    """y = StemConv.apply(x, weight, precision): FM_measure.Focus_extraction.0.0, Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2)) without
    BN or ReLU, through engine.op_conv3d; the backward through engine.op_stem_backward (the stem_wgrad kernels) gives the weight's gradient.
    x is the image stack and receives none."""

    @staticmethod
    def forward(ctx, x, weight, precision="bf16x3"):
        _dev(x, "x")
        ctx.save_for_backward(x)
        ctx.cfg = (weight.device, weight.dtype, precision)
        return engine.op_conv3d(x.detach().float(), weight, precision=precision, **engine.STEM_GEOMETRY)

    @staticmethod
    def backward(ctx, grad_y):
        (x,) = ctx.saved_tensors
        device, dtype, precision = ctx.cfg
        gw = engine.op_stem_backward(x, grad_y, precision=precision).to(device, dtype) if ctx.needs_input_grad[1] else None
        return None, gw, None


def stem_conv(x, weight, *, precision="bf16x3"):
    """The stem's conv on the HIP kernels with a gradient for ``weight``: x (B,3,N,H,W) float32 CUDA, the image stack; weight (8,3,1,9,9) in
    PyTorch layout (CPU or CUDA).  pipeline.batch_norm3d follows it as it follows any other conv.  The data gradient of the stem is not built:
    an ``x`` that requires grad is refused here rather than left without one."""
    if x.requires_grad:
        raise ValueError("stem_conv: x requires grad, but the data gradient of the stem is not built (DESIGN.md section 17: only the weight's is)")
    if tuple(weight.shape) != engine.STEM_WEIGHT_SHAPE:
        raise ValueError(f"stem_conv: weight {tuple(weight.shape)} is not the stem's {engine.STEM_WEIGHT_SHAPE}")
    return StemConv.apply(x, weight, precision)


# ---- train-mode BatchNorm: BatchNorm3d with its residual add and ReLU as an autograd node -------------------------------
class BatchNorm3d(torch.autograd.Function):
    """y = BatchNorm3d.apply(x, gamma, beta, running_mean, running_var, residual, relu, eps, momentum, precision): nn.BatchNorm3d in training
    mode followed by the optional residual add and ReLU, through engine.op_bn_train; the backward through engine.op_bn_train_backward gives the
    gradients of x, gamma, beta and the residual.  The running statistics are updated in place by the forward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean=None, running_var=None, residual=None, relu=False, eps=engine.BN_EPS, momentum=0.1, precision="bf16x3"):
        _dev(x, "x")
        y, mean, invstd = engine.op_bn_train(x, gamma, beta, running_mean, running_var, residual=residual, relu=relu, eps=eps, momentum=momentum,
                                             precision=precision)
        ctx.save_for_backward(x, y, gamma, mean, invstd)
        ctx.cfg = (bool(relu), residual is not None, precision)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, y, gamma, mean, invstd = ctx.saved_tensors
        relu, has_res, precision = ctx.cfg
        need_x = ctx.needs_input_grad[0] or (has_res and ctx.needs_input_grad[5])
        gx, gres, gg, gb = engine.op_bn_train_backward(x, y, grad_y, gamma, mean, invstd, relu=relu, residual=has_res and ctx.needs_input_grad[5],
                                                       precision=precision, need=("x", "params") if need_x else ("params",))
        return (gx if ctx.needs_input_grad[0] else None, gg.to(gamma.dtype) if ctx.needs_input_grad[1] else None,
                gb.to(gamma.dtype) if ctx.needs_input_grad[2] else None, None, None, gres, None, None, None, None)


def batch_norm3d(x, gamma, beta, running_mean=None, running_var=None, *, residual=None, relu=False, eps=engine.BN_EPS, momentum=0.1,
                 precision="bf16x3"):
    """[relu](BatchNorm3d(x) [+ residual]) in training mode on the HIP kernels, with gradients for x, gamma, beta and the residual: x (B,C,N,H,W)
    float32 CUDA with 8, 16, 32, 64 or 128 channels, gamma / beta / the running statistics CUDA tensors of C values (the running statistics
    float32, updated in place).  Behind pipeline.conv3d this is one conv -> BN -> (+skip) -> ReLU layer of the aggregation network."""
    return BatchNorm3d.apply(x, gamma, beta, running_mean, running_var, residual, relu, eps, momentum, precision)


# ---- the attention tail: y = x + relu(conv111(relu(conv311(x)))) as ONE autograd node with one backward kernel -----------
class AttentionTail(torch.autograd.Function):
    """y = AttentionTail.apply(x, w3, w1, precision): engine.op_attention_tail (two forward convs and the skip add), keeping a and t; its backward
    through engine.op_attention_tail_backward, one kernel for grad_x and both weight gradients, the ReLU masks read from the stored a and t."""

    @staticmethod
    def forward(ctx, x, w3, w1, precision="bf16x3"):
        _dev(x, "x")
        y, a, t = engine.op_attention_tail(x.detach().float(), w3, w1, precision=precision)
        ctx.save_for_backward(x, a, t, w3, w1)
        ctx.precision = precision
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, a, t, w3, w1 = ctx.saved_tensors
        need = (("x",) if ctx.needs_input_grad[0] else ()) + (("w",) if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] else ())
        gx, gw3, gw1 = engine.op_attention_tail_backward(x, a, t, grad_y, w3, w1, precision=ctx.precision, need=need)
        return (gx, gw3.to(w3.device, w3.dtype) if ctx.needs_input_grad[1] else None, gw1.to(w1.device, w1.dtype) if ctx.needs_input_grad[2] else None,
                None)


def attention_tail(x, w3, w1, *, precision="bf16x3"):
    """x + relu(conv111(relu(conv311(x)))) on the HIP kernels with gradients for x, w3 and w1: x (B,C,N,H,W) float32 CUDA with C = 8, 16 or 32,
    w3 (C,C,3,1,1) and w1 (C,C,1,1,1) in PyTorch layout (CPU or CUDA), no bias.  The forward is bit for bit conv3d -> relu -> conv3d -> relu -> +."""
    C = x.shape[1] if x.dim() == 5 else -1
    if tuple(w3.shape) != (C, C, 3, 1, 1) or tuple(w1.shape) != (C, C, 1, 1, 1):
        raise ValueError(f"attention_tail: x {tuple(x.shape)}, w3 {tuple(w3.shape)} and w1 {tuple(w1.shape)} are not (B,C,N,H,W), (C,C,3,1,1) and (C,C,1,1,1)")
    return AttentionTail.apply(x, w3, w1, precision)


def feature_extraction(x, params, *, precision="bf16x3", momentum=0.1):
    """The Feature_Extraction block in training mode: conv 1x3x3 -> BN -> ReLU -> conv 1x3x3 -> BN -> + x -> ReLU -> attention tail, out of
    conv3d, batch_norm3d and attention_tail.  ``params``: a mapping under the block's own key names -- Focus_Measure.conv.0.0.weight,
    Focus_Measure.conv.0.1.{weight,bias,running_mean,running_var}, Focus_Measure.conv.2.0.weight, Focus_Measure.conv.2.1.*,
    N_ch_attention.0.weight, N_ch_attention.2.weight -- i.e. a slice of a checkpoint or of a state_dict as it is.  The running statistics are
    updated in place."""
    def bn(v, key, **kw):
        return batch_norm3d(v, params[key + ".weight"], params[key + ".bias"], params[key + ".running_mean"], params[key + ".running_var"],
                            momentum=momentum, precision=precision, **kw)
    h = bn(conv3d(x, params["Focus_Measure.conv.0.0.weight"], pad=(0, 1, 1), precision=precision), "Focus_Measure.conv.0.1", relu=True)
    h = bn(conv3d(h, params["Focus_Measure.conv.2.0.weight"], pad=(0, 1, 1), precision=precision), "Focus_Measure.conv.2.1", residual=x, relu=True)
    return attention_tail(h, params["N_ch_attention.0.weight"], params["N_ch_attention.2.weight"], precision=precision)


# ---- the pools: MaxPool3d((1,2,2)), AvgPool3d((1,k,k)) and the pyramid's three average pools as autograd nodes -----------
class MaxPool3d(torch.autograd.Function):
    """y = MaxPool3d.apply(x, precision): the (1,2,2) max pool through engine.op_pool; the backward through engine.op_pool_backward sends each
    gradient to its window's first maximum among the stored values of x, as torch does."""

    @staticmethod
    def forward(ctx, x, precision="bf16x3"):
        _dev(x, "x")
        x = x.detach().float()
        ctx.save_for_backward(x)
        ctx.precision = precision
        return engine.op_pool(x, 2, "max", precision)

    @staticmethod
    def backward(ctx, grad_y):
        x, = ctx.saved_tensors
        return engine.op_pool_backward(grad_y, x=x, k=2, mode="max", precision=ctx.precision), None


class AvgPool3d(torch.autograd.Function):
    """y = AvgPool3d.apply(x, k, precision): the (1,k,k) average pool, k = 2, 4 or 8, through engine.op_pool and engine.op_pool_backward."""

    @staticmethod
    def forward(ctx, x, k, precision="bf16x3"):
        _dev(x, "x")
        ctx.cfg = (int(k), precision)
        return engine.op_pool(x.detach().float(), int(k), "avg", precision)

    @staticmethod
    def backward(ctx, grad_y):
        k, precision = ctx.cfg
        return engine.op_pool_backward(grad_y, k=k, mode="avg", precision=precision), None, None


class AvgPoolPyramid(torch.autograd.Function):
    """p2, p4, p8 = AvgPoolPyramid.apply(x, precision): the average pools (1,2,2), (1,4,4), (1,8,8) of one volume (one engine.op_pool3, the
    forward's single pass, bit-identical to three engine.op_pool calls); the backward is ONE engine.op_pool3_backward, an output without a gradient counting as zeros."""

    @staticmethod
    def forward(ctx, x, precision="bf16x3"):
        _dev(x, "x")
        x = x.detach().float()
        ctx.precision = precision
        ctx.set_materialize_grads(False)     # backward fills in the zeros itself, at the shapes it derives
        return engine.op_pool3(x, precision)

    @staticmethod
    def backward(ctx, g2, g4, g8):
        return engine.op_pool3_backward(*_pyramid_grads(g2, g4, g8), precision=ctx.precision), None


def _pyramid_grads(g2, g4, g8):
    """The three gradients of the pyramid's outputs, zeros for one autograd did not give."""
    given, f = next((g, f) for g, f in ((g2, 4), (g4, 2), (g8, 1)) if g is not None)
    B, C, N, h, w = given.shape
    H8, W8 = h // f, w // f
    return tuple(g if g is not None else given.new_zeros((B, C, N, m * H8, m * W8)) for g, m in ((g2, 4), (g4, 2), (g8, 1)))


def max_pool3d(x, *, precision="bf16x3"):
    """MaxPool3d((1,2,2)) of x (B,C,N,H,W) float32 CUDA on the HIP kernels, with the gradient of x: C a multiple of 8 up to 128, H and W even."""
    return MaxPool3d.apply(x, precision)


def avg_pool3d(x, k, *, precision="bf16x3"):
    """AvgPool3d((1,k,k)), k = 2, 4 or 8, of x (B,C,N,H,W) float32 CUDA on the HIP kernels, with the gradient of x."""
    return AvgPool3d.apply(x, k, precision)


def avg_pool_pyramid(x, *, precision="bf16x3"):
    """(p2, p4, p8): the average pools (1,2,2), (1,4,4), (1,8,8) that hourglassup takes of one volume x (B,C,N,H,W), H and W multiples of 8,
    with the gradient of x from one kernel launch."""
    return AvgPoolPyramid.apply(x, precision)


# ---- the optimiser: the reference's torch.optim.Adam(lr, betas=(0.9, 0.99)) on one multi-tensor HIP kernel ----------------
class Adam(torch.optim.Optimizer):
    """optimizer = Adam(model.parameters(), lr, betas=(0.9, 0.99), eps=1e-8); loss.backward(); optimizer.step(): what the reference's training
    scripts do, with every parameter of a group and device updated by ONE engine.op_adam_step call (ceil(n / engine.ADAM_TENSORS_PER_LAUNCH)
    launches, enqueue-only).  Parameters are float32 contiguous CUDA tensors.  The per-parameter state has torch.optim.Adam's keys and types
    (capturable=False): ``step`` a float32 CPU scalar, ``exp_avg`` and ``exp_avg_sq`` zeros_like(param); the groups carry its options.  A
    state_dict therefore loads into torch.optim.Adam and back.  weight_decay, amsgrad and maximize are not built: a value that asks for one is
    refused, here and when a loaded checkpoint brings it."""

    _NOT_BUILT = (("weight_decay", 0), ("amsgrad", False), ("maximize", False))

    def __init__(self, params, lr, betas=(0.9, 0.99), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if not 0.0 <= lr:
            raise ValueError(f"Adam: invalid learning rate {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Adam: invalid eps {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Adam: invalid betas {betas}")
        # the option keys of torch.optim.Adam's groups, so that a checkpoint of one class loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=False)
        self._refuse_not_built(defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._refuse_not_built(group)

    @classmethod
    def _refuse_not_built(cls, group):
        for name, off in cls._NOT_BUILT:
            if group.get(name, off) != off:
                raise ValueError(f"Adam: {name}={group[name]!r} is not built (DESIGN.md section 20: plain Adam only)")

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("Adam.step: closures are not supported")
        for gi, group in enumerate(self.param_groups):
            self._refuse_not_built(group)
            rows = []   # (p, grad, exp_avg, exp_avg_sq, step) of every parameter that has a gradient
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise ValueError("Adam: sparse gradients are not supported")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                rows.append((p, g if g.is_contiguous() else g.contiguous(), state["exp_avg"], state["exp_avg_sq"], state["step"]))
            if not rows:
                continue
            counts, bump = self._step_counts(gi, rows)
            # one call per device -- and per step count, which differs inside a group only after a partial load
            devs = [r[0].device for r in rows]
            if counts.count(counts[0]) == len(counts) and devs.count(devs[0]) == len(devs):
                calls = {(devs[0], int(counts[0]) + 1): rows}
            else:
                calls = {}
                for r, d, t in zip(rows, devs, counts):
                    calls.setdefault((d, int(t) + 1), []).append(r)
            for (_, t), rs in calls.items():
                ps, gs, ms, vs, _ = zip(*rs)
                engine.op_adam_step(ps, gs, ms, vs, step=t, lr=group["lr"], betas=group["betas"], eps=group["eps"])
                # the kernel wrote through raw pointers: count the in-place change as torch.optim.Adam's own updates do, so that whoever
                # watches the parameters' versions (Network's packed-weight cache) sees the step
                torch.autograd.graph.increment_version(ps)
            bump()   # counted once the updates are enqueued: a refused call leaves the counts as they were
        return None

    def _step_counts(self, gi, rows):
        """(the step counts of ``rows``' parameters before this step, a callable that adds 1 to each).  The ``step`` tensors of the parameters
        that step together are kept as the elements of ONE float32 CPU vector -- each state["step"] a 0-dim view of it, so that nothing changes
        for a reader of the state -- which is read and incremented whole: 200 separate CPU scalars cost more host time than the update's
        launches.  Whatever replaced the views since (load_state_dict, a first step) is packed again here."""
        steps = [r[4] for r in rows]
        cache = self.__dict__.setdefault("_packed_steps", {})   # per param group
        packed = cache.get(gi)
        if packed is None or len(packed[1]) != len(steps) or any(a is not b for a, b in zip(packed[1], steps)):
            base = torch.stack([s.detach().to("cpu", torch.float32).reshape(()) for s in steps])
            views = list(base.unbind(0))
            for r, v in zip(rows, views):
                self.state[r[0]]["step"] = v
            packed = cache[gi] = (base, views)
        return packed[0].tolist(), lambda: packed[0].add_(1)

