"""Reference for the backward of the regression heads under any upstream gradient, shared by tests/test_heads_grad.py (CPU)
and tests/test_gpu_heads_grad.py (GPU).

    v_n = bilinear(score_k, align_corners=False)   p_n = softplus(v_n) + 1e-6   S = sum_n p_n   d_k = sum_n f_n p_n / S
    dL/dv_n(i) = gp(i) * (f_n - d_k)/S * sigmoid(v_n)      dL/dscore_k = upsample^T(dL/dv)          gp = dL/dd_k, given

`reference` is torch autograd of sum(d * gp) on loss_ref._head (float64: the reference; float32: the calibration of the gate).
`manual_grads` is the same gradient in the kernel's formulation (explicit adjoint of the upsample), in which faults can be planted.
`bound` is the per-element error bound, in the idiom of loss_ref.bound with the loss bracket replaced by |gp|:

    |g - g64| <= ALPHA * G,   G = upsample^T(E),   E_n = |gp| * (|f_n| + |d|)/S * (sigmoid(v_n) + 1e-30) * (1 + |v_n|)

all of G in float64; no element is left out, and where G == 0 the result must be 0.

The cases are loss_ref.CASES (the smallest shapes at which a border, a chunk of 10 slices or a tile edge can go wrong) and an 8x8 stack whose
1/8 head is 1x1, so that every tap is clamped on both axes; each is crossed with four upstream gradients (KINDS) from a fixed seed.

ALPHA is calibrated, not fitted to the kernel: the float32 CPU autograd of this file over SPECS x KINDS has a worst err/G of
CAL_GRAD (test_heads_grad.py::test_calibration re-measures it); times 4 (hardware exp2 / log / rcp at ~1 ulp each, another fixed summation
order), rounded up to a power of two."""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as L  # noqa: E402

EPS32 = L.EPS32
CAL_GRAD = 8.97 * EPS32     # worst err/G of the float32 CPU autograd over SPECS x KINDS (n11_underflow, sparse, the 1/2 head)
ALPHA = 64 * EPS32          # 4 * CAL_GRAD = 35.9 * 2^-24, rounded up to a power of two

SPECS = L.CASES + [
    dict(id="n3_b2_8x8", B=2, N=3, H=8, W=8, scale=30.0, dense=False, rng=None, conf=False, mask="full", sentinel=0.0),
]
KINDS = ("dense", "sparse", "pixel", "big")   # randn; about 10 % non-zero; one pixel at (B-1, H//3, W-1); randn * 1e4


def alpha_rule(cal):
    """4 x the calibration figure, rounded up to a power of two"""
    return 2.0 ** math.ceil(math.log2(4 * cal))


def spec_of(cid):
    return next(s for s in SPECS if s["id"] == cid)


def make_gps(spec, case, kind):
    """the upstream gradients dL/dd_k, float32 (B,H,W), one per head of the case"""
    g = torch.Generator().manual_seed(7000 + KINDS.index(kind) + sum(map(ord, spec["id"])))
    B, H, W = case["gt"].shape
    out = []
    for _ in case["scores"]:
        r = torch.randn(B, H, W, generator=g)
        if kind == "sparse":
            r = r * (torch.rand(B, H, W, generator=g) < 0.1)
        elif kind == "pixel":
            one = torch.zeros(B, H, W)
            one[B - 1, H // 3, W - 1] = r[B - 1, H // 3, W - 1]
            r = one
        elif kind == "big":
            r = r * 1e4
        out.append(r.contiguous())
    return out


def reference(case, gps, dtype=torch.float64):
    """the gradients of sum_k sum(d_k * gp_k) with respect to the scores, by torch autograd in `dtype`"""
    B, H, W = case["gt"].shape
    fd = case["fd"].to(dtype)
    out = []
    for s, gp in zip(case["scores"], gps):
        x = s.to(dtype).requires_grad_(True)
        d = L._head(x, fd, H, W)[3]
        out.append(torch.autograd.grad((d * gp.to(dtype)).sum(), x)[0])
    return out


def bound(case, gps):
    """G per head (float64): the scale of the admissible error of every gradient element."""
    dt = torch.float64
    B, H, W = case["gt"].shape
    fd = case["fd"].to(dt).expand(B, -1, H, W)
    out = []
    for s, gp in zip(case["scores"], gps):
        x = s.to(dt).requires_grad_(True)
        v, p, S, d = L._head(x, fd, H, W)
        E = gp.to(dt).abs().unsqueeze(1) * ((fd.abs() + d.abs().unsqueeze(1)) / S.unsqueeze(1)) * (torch.sigmoid(v) + 1e-30) * (1 + v.abs())
        out.append(torch.autograd.grad((L._upsample(x, H, W) * E.detach()).sum(), x)[0])   # upsample^T(E)
    return out


FAULTS = ("no_clamp", "missed_pixel", "no_threshold", "f_not_centred", "no_S")


def manual_grads(case, gps, dtype=torch.float32, fault=None):
    """The gradients in the kernel's formulation, every step in `dtype`; `fault` plants one defect:
    no_clamp (the adjoint drops the taps past the far border instead of clamping them), missed_pixel (one contributor of every
    low-resolution element is left out), no_threshold (sigmoid as e/(1+e) without the v > 20 branch), f_not_centred (f_n in place of
    f_n - d), no_S (the division by S dropped)."""
    B, H, W = case["gt"].shape
    fd = case["fd"].to(dtype).expand(B, -1, H, W)
    out = []
    for s, gp in zip(case["scores"], gps):
        s, gp = s.to(dtype), gp.to(dtype)
        N, h, wd = s.shape[1:]
        y0, y1, ly = L._axis_taps(H, h, dtype)
        x0, x1, lx = L._axis_taps(W, wd, dtype)
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
        gS = gp if fault == "no_S" else gp / S
        fm = fd if fault == "f_not_centred" else fd - d.unsqueeze(1)
        a = gS.unsqueeze(1) * fm * sig if N > 1 else torch.zeros_like(v)
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


_cache = {}


def evaluated(cid, kind):
    """(case, gps, float64 reference, bound) of one case x gradient kind: computed once, shared, never modified"""
    key = (cid, kind)
    if key not in _cache:
        spec = spec_of(cid)
        if cid not in _cache:
            _cache[cid] = L.make_case(spec)
        case = _cache[cid]
        gps = make_gps(spec, case, kind)
        _cache[key] = (case, gps, reference(case, gps), bound(case, gps))
    return _cache[key]


worst_ratio = L.worst_ratio
