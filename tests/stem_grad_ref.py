"""Reference, bound and a CPU emulation for the weight gradient of the stem; shared by tests/test_stem_grad.py and
tests/test_gpu_stem_grad.py.

The stem is FM_measure.Focus_extraction.0.0: Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2), bias=False) on the image stack.

Reference: float64 ``torch.autograd.grad`` of ``F.conv3d`` on the CPU.

Bound: section 13's, unchanged.  Every grad_w element is one dot product over the pixels, both operands rounded to the parts of the precision
exactly like a forward conv's, so

    |dW - dW64| <= ALPHA[prec] * G,        G = sum |grad_y| * |x| over the same contraction

plus, for fp16, ``FP16_SUB * (sum |grad_y| + sum |x|)``.  ``ALPHA`` is ``oracle.error_bounds``'.  ``emulate`` runs the kernel's arithmetic: the
fp32 accumulation over at most PARTIAL_PIXELS pixels is the one term the derivation does not cover, and tests/test_stem_grad.py holds it well
inside the bound.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_grad_ref as cg  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402

PRECISIONS = cg.PRECISIONS
CO, CI, K, DIL, PAD = 8, 3, 9, 2, 8
WEIGHT_SHAPE = (CO, CI, 1, K, K)
GEOMETRY = dict(stride=1, pad=(0, PAD, PAD), dilation=(1, DIL, DIL))
# what dffw_stem_wgrad.h fixes: a unit is TY x TX pixels, 16 chunks of 32 (2 rows x 16 columns); the fp32 accumulators are flushed after FLUSH_UNITS units
TY, TX, FLUSH_UNITS, DEFAULT_WGS = 16, 32, 32, 512
PARTIAL_PIXELS = TY * TX * FLUSH_UNITS   # 16 384
assert PARTIAL_PIXELS == cg.PARTIAL_PIXELS
REGIMES = ("zero_mean", "post_relu", "offset")
FAULTS = ("dilation1", "swap_kykx", "swap_planes", "pad7", "wrap_row", "drop_product", "missing_partial")


def conv64(x, w):
    return F.conv3d(x, w, None, 1, (0, PAD, PAD), (1, DIL, DIL))


def _wgrad_of(x, gy):
    w = torch.zeros(WEIGHT_SHAPE, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(conv64(x, w), w, gy)[0]


def wgrad64(x, gy):
    """grad_w of <gy, stem(x, w)> by float64 autograd."""
    return _wgrad_of(x.detach().cpu().double(), gy.detach().cpu().double())


def wgrad_ref64(x, gy):
    """Ref64 of grad_w: reference, G = sum |gy| |x| as D, and the fp16 subnormal term."""
    x, gy = x.detach().cpu().double(), gy.detach().cpu().double()
    ref = _wgrad_of(x, gy)
    G = _wgrad_of(x.abs(), gy.abs())
    sub = eb.FP16_SUB * (_wgrad_of(torch.ones_like(x), gy.abs()) + _wgrad_of(x.abs(), torch.ones_like(gy)))
    return eb.Ref64(ref, ref, G, sub)


def rounded(t, prec):
    """The value a record of ``prec`` holds for ``t``: hi + lo for split-bf16."""
    parts = cg.round_parts(t, prec)
    return parts[0] + parts[1] if len(parts) == 2 else parts[0]


def total_units(B, N, H, W):
    return B * N * -(-H // TY) * -(-W // TX)


def grid_x_of(B, N, H, W, wgs=0):
    """persistent_grid (dffw_persist.h) of the launch: ``wgs`` is DFFW_WGRAD_WGS (0: the default)."""
    want = max(8, wgs if wgs > 0 else DEFAULT_WGS)
    return 8 * min(-(-total_units(B, N, H, W) // 8), max(1, want // 8))


def units_per_workgroup(B, N, H, W, wgs=0):
    """How many units every workgroup of the launch sums.  More than FLUSH_UNITS: it flushes a full-length fp32 partial and starts another."""
    return [len(u) for u in cg.persistent_units(total_units(B, N, H, W), grid_x_of(B, N, H, W, wgs))]


def _chunks(t, H, W):
    """(B*N, C, H, W) -> (units, 16 chunks, 32 pixels, C): units numbered x fastest, then y, slice, sample; chunk (cr, ch) is rows 2cr, 2cr + 1
    and columns 16 ch .. 16 ch + 15 of the unit, cr outer."""
    BN, C = t.shape[:2]
    ty, tx = -(-H // TY), -(-W // TX)
    t = F.pad(t, (0, tx * TX - W, 0, ty * TY - H))
    t = t.reshape(BN, C, ty, TY // 2, 2, tx, TX // 16, 16).permute(0, 2, 5, 3, 6, 4, 7, 1)
    return t.reshape(BN * ty * tx, TY // 2 * (TX // 16), 32, C)


def _columns(t, H, W, fault):
    """(B*N, 3, H, W) -> (B*N, 243, H, W): column (ci, ky, kx) holds x[ci, y + 2 ky - 8, x + 2 kx - 8], zero outside the image."""
    BN = t.shape[0]
    if fault == "wrap_row":   # a column beyond the row's end read from the neighbouring row, as flat addressing without a column check would
        flat = F.pad(t, (0, 0, PAD + 1, PAD + 1)).reshape(BN, CI, -1)
        cols = [torch.roll(flat, -((DIL * ky - PAD) * W + DIL * kx - PAD), 2).reshape(BN, CI, H + 2 * PAD + 2, W)[:, :, PAD + 1:PAD + 1 + H]
                for ky in range(K) for kx in range(K)]
        return torch.stack(cols, 2).reshape(BN, CI * K * K, H, W)
    dil, pad = (1, PAD) if fault == "dilation1" else (DIL, PAD - 1) if fault == "pad7" else (DIL, PAD)
    big = F.pad(t, (pad, 2 * PAD, pad, 2 * PAD))       # the taps start `pad` before the pixel; the far side is long enough for every variant
    cols = F.unfold(big, K, dilation=dil).reshape(BN, CI * K * K, H + pad + 2 * PAD - dil * (K - 1), -1)[:, :, :H, :W]
    if fault == "swap_planes":
        cols = cols.reshape(BN, CI, K * K, H, W)[:, [1, 0, 2]].reshape(BN, CI * K * K, H, W)
    if fault == "swap_kykx":
        cols = cols.reshape(BN, CI, K, K, H, W).transpose(2, 3).reshape(BN, CI * K * K, H, W)
    return cols


def emulate(x, gy, prec, *, wgs=0, flush_units=FLUSH_UNITS, fault=None):
    """grad_w in the kernel's arithmetic: both operands rounded to the parts of ``prec``; per 32-pixel chunk one fp32 MFMA step per product (for
    bf16x3 lo*hi, hi*lo, hi*hi, in that order) added to an fp32 accumulator; the accumulator added to a float64 sum every ``flush_units`` units
    and at the end; the workgroups' sums added in float64 in workgroup order, over the unit ranges of the real launch (``wgs`` = DFFW_WGRAD_WGS).
    ``fault`` plants one of FAULTS."""
    B, _, N, H, W = x.shape
    x, gy = x.detach().cpu().float(), gy.detach().cpu().float()
    flat = lambda t: t.permute(0, 2, 1, 3, 4).reshape(B * N, t.shape[1], H, W)
    gp = [_chunks(flat(t), H, W) for t in cg.round_parts(gy, prec)]                      # (units, 16, 32, 8)
    xp = [_chunks(_columns(flat(t), H, W, fault), H, W) for t in cg.round_parts(x, prec)]   # (units, 16, 32, 243)
    nparts, nu = len(gp), gp[0].shape[0]
    assert nu == total_units(B, N, H, W)
    upw = cg.persistent_units(nu, grid_x_of(B, N, H, W, wgs))
    longest = max(len(u) for u in upw)
    idx = torch.tensor([u + [nu] * (longest - len(u)) for u in upw], dtype=torch.long)   # short workgroups end on a unit of zeros: + 0 exactly
    gp = [torch.cat([t, torch.zeros_like(t[:1])]) for t in gp]
    xp = [torch.cat([t, torch.zeros_like(t[:1])]) for t in xp]
    order = ((1, 0), (0, 1), (0, 0)) if nparts == 2 else ((0, 0),)
    if fault == "drop_product" and nparts == 2:
        order = order[1:]
    total = torch.zeros(len(upw), CO, CI * K * K, dtype=torch.float64)
    acc = torch.zeros(len(upw), CO, CI * K * K, dtype=torch.float32)
    since = 0
    for i in range(longest):
        A = [t[idx[:, i]].transpose(2, 3) for t in gp]     # (wg, 16, 8, 32)
        Bm = [t[idx[:, i]] for t in xp]                    # (wg, 16, 32, 243)
        for c in range(A[0].shape[1]):
            for ia, ib in order:
                acc = acc + torch.bmm(A[ia][:, c], Bm[ib][:, c])
        since += 1
        if since >= flush_units:
            total, acc, since = total + acc.double(), torch.zeros_like(acc), 0
    total = total + acc.double()
    if fault == "missing_partial":
        total[max(range(len(upw)), key=lambda w: len(upw[w]))] = 0
    dw = torch.zeros(CO, CI * K * K, dtype=torch.float64)
    for blk in total:                                      # workgroup order
        dw = dw + blk
    return dw.float().reshape(WEIGHT_SHAPE)


def make_case(regime, B, N, H, W, seed):
    """(x, gy) float32 CPU tensors of a regime: zero_mean (both uniform in [-1, 1]); post_relu (half of gy zero, as behind a ReLU); offset (both
    1 + 0.25 U: no cancellation, the regime where the fp32 partials grow fastest)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda c: torch.rand(B, c, N, H, W, generator=g) * 2 - 1
    x, gy = u(CI), u(CO)
    if regime == "post_relu":
        gy = F.relu(gy)
    elif regime == "offset":
        x, gy = 1 + 0.25 * x, 1 + 0.25 * gy
    else:
        assert regime == "zero_mean", regime
    return x, gy


def int_case(B, N, H, W, seed):
    """Small integers: exact in every format, every product and every sum, in any order."""
    g = torch.Generator().manual_seed(seed)
    r = lambda c: torch.randint(-3, 4, (B, c, N, H, W), generator=g).float()
    return r(CI), r(CO)
