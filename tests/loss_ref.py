"""Reference for the training loss and the regression-head backward, shared by tests/test_loss.py (CPU) and
tests/test_gpu_loss.py (GPU).

    v_n = bilinear(score_k, align_corners=False)   p_n = softplus(v_n) + 1e-6   d_k = sum_n f_n p_n / sum_n p_n
    Loss_k = sum_i c_i m_i ((d_k - gt)/r)^2 / Z,  Z = sum_i c_i m_i      Total = sum_k w_k Loss_k

`reference` restates this in torch autograd (float64: the reference; float32: the calibration of the gates).  `manual_grads` is the same
gradient in the kernel's formulation (explicit adjoint of the upsample), in which faults can be planted.  `bound` is the per-element
error bound, in the idiom of oracle/error_bounds.py:

    |g - g64| <= ALPHA * G,   G = upsample^T(E),   E_n = [2 w c m (|d| + |gt|) / (r^2 Z)] * (|f_n| + |d|)/S * (sigmoid(v_n) + 1e-30) * (1 + |v_n|)

all of G in float64; (1 + |v|) carries the interpolation error of v into sigmoid, 1e-30 absorbs the float32 underflow of exp(v) near -88.

ALPHA and LOSS_RTOL are calibrated, not fitted to the kernel: the float32 CPU autograd of this file over CASES (the GPU test's own list)
has a worst err/G of 5.81 * 2^-24 (n16_conf, full-resolution head) and a worst relative loss error of 1.68e-6 (mask_single: one pixel, no averaging) (test_loss.py::test_calibration re-measures both); times 4
(hardware exp2 / log / rcp at ~1 ulp each, another fixed summation order), rounded up to a power of two."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHTS = (0.3, 0.5, 0.7, 1.0)
EPS32 = 2.0 ** -24
CAL_GRAD = 5.81 * EPS32     # worst err/G of the float32 CPU autograd over CASES
CAL_LOSS = 1.68e-6          # its worst relative loss error
ALPHA = 32 * EPS32          # 4 * CAL_GRAD = 23.2 * 2^-24, rounded up to a power of two
LOSS_RTOL = 2.0 ** -17      # 4 * CAL_LOSS = 6.7e-6, rounded up to a power of two (7.6e-6)

# the GPU test's cases: the smallest shapes at which each mechanism can fail.  32x32: the 1/8 head is 4x4, every element on a border;
# 96x64 / 64x96: non-square, interior and border elements, several tiles in both directions for every head; N on either side of the slice
# chunk (10) and of the forward's unroll boundaries; scores scaled to +-1 (plain), +-30 (threshold branch), +-100 (underflow of exp)
CASES = [
    dict(id="n1_32x32", B=1, N=1, H=32, W=32, scale=1.0, dense=False, rng=None, conf=False, mask="full", sentinel=0.0),
    dict(id="n2_b3_ranged_nan", B=3, N=2, H=32, W=32, scale=30.0, dense=False, rng=(10.0, 100.0), conf=False, mask="random", sentinel=float("nan")),
    dict(id="n5_conf_dense", B=1, N=5, H=96, W=64, scale=1.0, dense=True, rng=(1 / 3.91092, 1 / 0.10201), conf=True, mask="random", sentinel=-3.0),
    dict(id="n10_b3_dense", B=3, N=10, H=96, W=64, scale=30.0, dense=True, rng=None, conf=False, mask="random", sentinel=float("nan")),
    dict(id="n11_underflow", B=1, N=11, H=64, W=96, scale=100.0, dense=False, rng=(10.0, 100.0), conf=False, mask="random", sentinel=-3.0),
    dict(id="n16_conf", B=1, N=16, H=96, W=64, scale=30.0, dense=False, rng=None, conf=True, mask="random", sentinel=float("nan")),
    dict(id="n17_dense", B=1, N=17, H=64, W=64, scale=100.0, dense=True, rng=None, conf=False, mask="random", sentinel=-3.0),
    dict(id="mask_empty", B=1, N=5, H=32, W=64, scale=30.0, dense=False, rng=None, conf=True, mask="empty", sentinel=float("nan")),
    dict(id="mask_single", B=1, N=5, H=32, W=64, scale=30.0, dense=False, rng=None, conf=False, mask="single", sentinel=float("nan")),
    dict(id="mask_full_b3", B=3, N=5, H=64, W=32, scale=1.0, dense=False, rng=None, conf=True, mask="full", sentinel=0.0),
    dict(id="one_head", B=1, N=10, H=96, W=64, scale=30.0, dense=False, rng=None, conf=False, mask="random", sentinel=float("nan"), heads=(1,)),
]


def make_case(spec, seed=0):
    """CPU tensors of one case: scores (4 or the listed heads), fd, gt, mask (bool), conf or None, weights, rng."""
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, spec["id"])))
    B, N, H, W = spec["B"], spec["N"], spec["H"], spec["W"]
    heads = spec.get("heads", (0, 1, 2, 3))
    scores = [(torch.rand(B, N, H >> (3 - k), W >> (3 - k), generator=g) * 2 - 1) * spec["scale"] for k in heads]
    lo, hi = spec["rng"] if spec["rng"] else (0.1, 1.5)
    fd = lo + (hi - lo) * torch.rand((B, N, H, W) if spec["dense"] else (B, N, 1, 1), generator=g)
    gt = lo + (hi - lo) * torch.rand(B, H, W, generator=g)
    if spec["mask"] == "random":
        mask = torch.rand(B, H, W, generator=g) < 0.6
    elif spec["mask"] == "full":
        mask = torch.ones(B, H, W, dtype=torch.bool)
    else:
        mask = torch.zeros(B, H, W, dtype=torch.bool)
        if spec["mask"] == "single":
            mask[B - 1, H // 3, W - 1] = True
    gt[~mask] = spec["sentinel"]
    conf = torch.rand(B, H, W, generator=g) + 0.05 if spec["conf"] else None
    return dict(scores=scores, fd=fd, gt=gt, mask=mask, conf=conf, weights=[WEIGHTS[k] for k in heads], rng=spec["rng"])


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, "loss_%s.npz" % name))
    t = lambda k: torch.from_numpy(z[k])
    case = dict(scores=[t("score%d" % k) for k in range(4)], fd=t("focus_dists"), gt=t("gt"), mask=t("mask"),
                conf=t("conf") if z["conf"].size else None, weights=[float(x) for x in z["weights"]],
                rng=tuple(float(x) for x in z["range"]) if z["range"].size else None)
    want = dict(losses=t("losses"), preds=[t("pred%d" % k) for k in range(4)], grads=[t("grad%d" % k) for k in range(4)])
    return case, want


def _range(case, dtype):
    if not case["rng"]:
        return torch.tensor(1.0, dtype=dtype)
    lo, hi = (torch.tensor(x, dtype=torch.float32).to(dtype) for x in case["rng"])   # the C ABI takes the range as two floats
    return hi - lo


def _upsample(s, H, W):
    return s if s.shape[-2:] == (H, W) else F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False)


def _head(score, fd, H, W):
    v = _upsample(score, H, W)
    p = F.softplus(v) + 1e-6
    S = p.sum(1)
    return v, p, S, (fd * p).sum(1) / S


def reference(case, dtype=torch.float64, grads=True):
    """dict(total, per_head (n,), preds, grads) by torch autograd in `dtype`."""
    B, H, W = case["gt"].shape
    scores = [s.to(dtype).requires_grad_(grads) for s in case["scores"]]
    fd, gt, mask = case["fd"].to(dtype), case["gt"].to(dtype), case["mask"]
    c = case["conf"].to(dtype)[mask] if case["conf"] is not None else torch.ones(int(mask.sum()), dtype=dtype)
    r, Z = _range(case, dtype), c.sum()
    per, preds, total = [], [], 0
    for s, w in zip(scores, case["weights"]):
        d = _head(s, fd, H, W)[3]
        preds.append(d.detach())
        per.append((c * ((d[mask] - gt[mask]) / r) ** 2).sum() / Z)   # an empty selection: 0/0 = NaN, as torch's MSELoss gives
        total = total + w * per[-1]
    g = None
    if grads:
        g = [torch.zeros_like(s) for s in scores] if Z == 0 else list(torch.autograd.grad(total, scores))
    return dict(total=total.detach(), per_head=torch.stack(per).detach(), preds=preds, grads=g)


def bound(case):
    """G per head (float64): the scale of the admissible error of every gradient element."""
    dt = torch.float64
    B, H, W = case["gt"].shape
    fd, mask = case["fd"].to(dt).expand(B, -1, H, W), case["mask"]
    gt = torch.where(mask, case["gt"].to(dt), torch.zeros((), dtype=dt))
    c = case["conf"].to(dt) if case["conf"] is not None else torch.ones(B, H, W, dtype=dt)
    cm = torch.where(mask, c, torch.zeros((), dtype=dt))
    r, Z = _range(case, dt), cm.sum()
    out = []
    for s, w in zip(case["scores"], case["weights"]):
        x = s.to(dt).requires_grad_(True)
        v, p, S, d = _head(x, fd, H, W)
        if Z == 0:
            out.append(torch.zeros_like(x).detach())
            continue
        E = (2 * w * cm * (d.abs() + gt.abs()) / (r * r * Z)).unsqueeze(1) * ((fd.abs() + d.abs().unsqueeze(1)) / S.unsqueeze(1)) \
            * (torch.sigmoid(v) + 1e-30) * (1 + v.abs())
        out.append(torch.autograd.grad((_upsample(x, H, W) * E.detach()).sum(), x)[0])   # upsample^T(E)
    return out


def _axis_taps(n_out, n_in, dtype):
    """PyTorch's align_corners=False index rule along one axis: i0, i1 (clamped), l (weight of i1)."""
    s = ((torch.arange(n_out, dtype=dtype) + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
    i0 = s.floor().long()
    return i0, i0 + 1, s - i0.to(dtype)


def manual_grads(case, dtype=torch.float32, fault=None):
    """The gradients in the kernel's formulation, every step in `dtype`; `fault` plants one defect:
    no_clamp (the adjoint drops the taps past the far border instead of clamping them), missed_pixel (one contributor of every
    low-resolution element is left out), no_threshold (sigmoid as e/(1+e) without the v > 20 branch), mask_mul (the mask multiplies
    instead of selecting), z_no_conf (Z counts pixels although conf is given)."""
    B, H, W = case["gt"].shape
    fd, gt, mask = case["fd"].to(dtype).expand(B, -1, H, W), case["gt"].to(dtype), case["mask"]
    c = case["conf"].to(dtype) if case["conf"] is not None else torch.ones(B, H, W, dtype=dtype)
    Z = mask.sum().to(dtype) if fault == "z_no_conf" else torch.where(mask, c, torch.zeros((), dtype=dtype)).sum()
    r = _range(case, dtype)
    out = []
    for s, w in zip(case["scores"], case["weights"]):
        s = s.to(dtype)
        N, h, wd = s.shape[1:]
        y0, y1, ly = _axis_taps(H, h, dtype)
        x0, x1, lx = _axis_taps(W, wd, dtype)
        y1c, x1c = y1.clamp(max=h - 1), x1.clamp(max=wd - 1)
        wy = [(y0, 1 - ly), (y1c, ly)]
        wx = [(x0, 1 - lx), (x1c, lx)]
        v = sum(s[:, :, yi][:, :, :, xi] * (a[:, None] * b[None, :]) for yi, a in wy for xi, b in wx) if h != H else s
        p = F.softplus(v) + 1e-6
        S = p.sum(1)
        d = (fd * p).sum(1) / S
        if fault == "no_threshold":
            e = torch.exp(v)
            sig = e / (1 + e)
        else:
            sig = torch.where(v > 20, torch.ones((), dtype=dtype), torch.sigmoid(v))
        k = 2 * w * c * (d - gt) / (r * r * Z)
        gd = k * mask.to(dtype) if fault == "mask_mul" else torch.where(mask, k, torch.zeros((), dtype=dtype))
        a = (gd / S).unsqueeze(1) * (fd - d.unsqueeze(1)) * sig if N > 1 else torch.zeros_like(v)
        if h == H:
            out.append(a)
            continue
        S_ = H // h
        g = torch.zeros(B, N, h + 1, wd + 1, dtype=dtype)   # one spare row / column takes the unclamped taps of no_clamp
        for ti, (yi, wa) in enumerate(((y0, 1 - ly), (y1 if fault == "no_clamp" else y1c, ly))):
            for tk, (xi, wb) in enumerate(((x0, 1 - lx), (x1 if fault == "no_clamp" else x1c, lx))):
                t = a * (wa[:, None] * wb[None, :])
                if fault == "missed_pixel" and ti == 0 and tk == 0:
                    t = t.clone()
                    t[:, :, S_ // 2::S_, S_ // 2::S_] = 0   # the pixel nearest to each element's centre
                idx = (yi[:, None] * (wd + 1) + xi[None, :]).reshape(-1)
                g.view(B, N, -1).index_add_(2, idx, t.reshape(B, N, -1))
        out.append(g[:, :, :h, :wd].contiguous())
    return out


def worst_ratio(got, ref, G):
    """max over elements of |got - ref| / G per head (inf where got is not finite or G is 0 and got differs)."""
    out = []
    for a, b, g in zip(got, ref, G):
        err = (a.double() - b.double()).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        ratio = torch.where(err == 0, torch.zeros_like(err), err / g)
        out.append(float(ratio.detach().max()) if ratio.numel() else 0.0)
    return out
