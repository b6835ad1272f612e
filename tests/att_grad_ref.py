"""Reference, bounds and a CPU emulation for the fused backward of the attention tail; shared by tests/test_att_grad.py
and tests/test_gpu_att_grad.py.  The record helpers and persistent_units are those of tests/conv_grad_ref.py, ``rounded`` and ``U`` those of
tests/pw_grad_ref.py.

Reference.  The five formulas of the section in float64, formed from the record-rounded x, a, t, grad_y, the fp32 filters and the masks of the
STORED a and t (``formulas64``; ``ref64`` rounds the operands first).

Bounds, stage by stage, with oracle.error_bounds.ALPHA unchanged (alpha), the record's unit roundoff U (u) and |.| taken elementwise:

    gt  = [t > 0] gy                          exact: a record or +0
    ga  = [a > 0] W1^T gt                     E_ga  = [a > 0] (alpha sum |w1| |gt| + u |W1^T gt|)         the contraction, then ga's rounding to the record format
    gx  = gy + adj311(ga, W3)                 E_gx  = alpha adj311(|ga|, |W3|) + adj311(E_ga, |W3|) + u |gx|     own contraction, ga's error carried, gx stored
    dW1 = sum gt a                            E_dW1 = alpha sum |gt| |a|                                  both operands are records: section 13's bound
    dW3 = sum ga x                            E_dW3 = alpha sum |ga| |x| + sum E_ga |x|                   own contraction, ga's error carried

fp16 adds the subnormal terms (FP16_SUB = 2^-25 per rounded weight or stored value): to E_ga ``[a > 0] FP16_SUB (sum_co |gt| + 1)``, to E_gx
``FP16_SUB (adj311(|ga|, 1) + 1)``, and both are carried like E_ga.  The masks are exact (stored values), so nothing passes a closed ReLU.
"""
import torch
import torch.nn.functional as F

import conv_grad_ref as cg
import pw_grad_ref as pw
from oracle import error_bounds as eb

PRECISIONS = cg.PRECISIONS
# what dffw_att_grad.h fixes
P, WAVE_PIX, WAVES, FLUSH_STEPS, DEFAULT_WGS = 128, 32, 4, 512, 512
SHAPES = ((1, 1, 8, 8), (2, 2, 12, 20), (2, 3, 8, 8), (1, 5, 16, 24), (2, 10, 32, 32))   # (B, N, H, W) of the GPU tests


def adj311(v, w):
    """sum_kz sum_co w[co][ci][kz] v[n - kz + 1][co]: the adjoint of the 3x1x1 pad (1,0,0) conv."""
    return F.conv_transpose3d(v, w, None, 1, (1, 0, 0))


def forward64(x, w3, w1):
    """(y, a, t) of the tail in the dtype of its arguments."""
    a = F.relu(F.conv3d(x, w3, None, 1, (1, 0, 0)))
    t = F.relu(F.conv3d(a, w1))
    return x + t, a, t


def formulas64(x, a, t, gy, w3, w1):
    """(gx, dW3, dW1, ga, gt) by the section's five formulas, float64 in and out, the masks from the given a and t."""
    gt = (t > 0).double() * gy
    ga = (a > 0).double() * torch.einsum("oi,bonhw->binhw", w1[:, :, 0, 0, 0], gt)
    gx = gy + adj311(ga, w3)
    dw1 = torch.einsum("bonhw,binhw->oi", gt, a)[..., None, None, None]
    dw3 = pw._wgrad_of(x, ga, "k311")
    return gx, dw3, dw1, ga, gt


class Ref:
    """Float64 references and per-element bounds of the three gradients for one arithmetic."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def ref64(x, a, t, gy, w3, w1, prec):
    X, A, T, G = (pw.rounded(v.detach().cpu(), prec).double() for v in (x, a, t, gy))
    W3, W1 = w3.detach().cpu().double(), w1.detach().cpu().double()
    gx, dw3, dw1, ga, gt = formulas64(X, A, T, G, W3, W1)
    al, u = eb.ALPHA[prec], pw.U[prec]
    sub = eb.FP16_SUB if prec == "fp16" else 0.0
    ma = (A > 0).double()
    w1m = W1[:, :, 0, 0, 0]
    ga_pre = torch.einsum("oi,bonhw->binhw", w1m, gt)
    e_ga = ma * (al * torch.einsum("oi,bonhw->binhw", w1m.abs(), gt.abs()) + u * ga_pre.abs() + sub * (gt.abs().sum(1, keepdim=True) + 1.0))
    e_gx = al * adj311(ga.abs(), W3.abs()) + adj311(e_ga, W3.abs()) + u * gx.abs() + sub * (adj311(ga.abs(), torch.ones_like(W3)) + 1.0)
    e_dw1 = al * torch.einsum("bonhw,binhw->oi", gt.abs(), A.abs())[..., None, None, None]
    e_dw3 = al * pw._wgrad_of(X.abs(), ga.abs(), "k311") + pw._wgrad_of(X.abs(), e_ga, "k311")
    return Ref(gx=gx, dw3=dw3, dw1=dw1, e_gx=e_gx, e_dw3=e_dw3, e_dw1=e_dw1, ga=ga, gt=gt, mask_a=ma, mask_t=(T > 0))


def ratios(got, r):
    """Worst err / bound of (gx, dW3, dW1) against a Ref; an entry of ``got`` may be None."""
    out = []
    for g, ref, e in zip(got, (r.gx, r.dw3, r.dw1), (r.e_gx, r.e_dw3, r.e_dw1)):
        out.append(float(eb._ratio((g.detach().cpu().double() - ref).abs(), e).max()) if g is not None else 0.0)
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def filters(C, g, scale=1.7):
    u = lambda shape: torch.rand(*shape, generator=g) * 2 - 1
    return u((C, C, 3, 1, 1)) * (2.0 / (3 * C)) ** 0.5 * scale, u((C, C, 1, 1, 1)) * (2.0 / C) ** 0.5 * scale


def make_case(regime, B, C, N, H, W, seed):
    """(x, w3, w1, gy) float32 CPU tensors: zero_mean, post_relu (x) and offset (x and gy), as conv_grad_ref.make_case's regimes.  The filters
    are zero-mean at He scale, so both ReLUs open about half of their elements in every regime."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape: torch.rand(*shape, generator=g) * 2 - 1
    x, gy = u((B, C, N, H, W)), u((B, C, N, H, W))
    if regime == "post_relu":
        x = F.relu(x)
    elif regime == "offset":
        x, gy = 3 + 0.5 * x, 1 + 0.25 * gy
    else:
        assert regime == "zero_mean", regime
    w3, w1 = filters(C, g)
    return x, w3, w1, gy


def int_case(B, C, N, H, W, seed):
    """Small integers with sparse filters: every intermediate and every result is an integer a record holds exactly (the tests assert it)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()
    x, gy = r((B, C, N, H, W), -2, 2), r((B, C, N, H, W), -2, 2)
    keep = lambda shape: (torch.rand(*shape, generator=g) < 2.0 / C).float()
    w3 = r((C, C, 3, 1, 1), -1, 1) * keep((C, C, 3, 1, 1))
    w1 = r((C, C, 1, 1, 1), -1, 1) * keep((C, C, 1, 1, 1))
    return x, w3, w1, gy


def exact_in_record(v, prec):
    return bool((pw.rounded(v.float(), prec).double() == v.double()).all())


# ---- the kernel's decomposition ---------------------------------------------------------------------------------------------------------------
def chunks_of(H, W):
    return -(-(H * W) // P)


def grid_x_of(B, H, W, wgs=DEFAULT_WGS):
    """att_tail_bwd_grid_x: ``wgs`` workgroups, at least 8, a multiple of 8, never more per XCD than it has units."""
    total = B * chunks_of(H, W)
    return 8 * min(-(-total // 8), max(1, max(8, wgs) // 8))


def steps_per_workgroup(B, N, H, W, grid_x):
    return [len(units) * N for units in cg.persistent_units(B * chunks_of(H, W), grid_x)]


def _cols(t, runs_on=False):
    """(B, C, N, H, W) -> (B, N, chunks * P, C): the flat plane, zero-filled to whole chunks (or, the planted fault, running on in memory)."""
    c = (pw._columns_running_on if runs_on else pw._columns)(t)
    return c.permute(0, 2, 3, 1).contiguous()


def _mm3(acc, A, Bm, order):
    """acc + the products of the parts in the family's order, each one fp32 matrix product (an MFMA step's worth of contraction)."""
    for ia, ib in order:
        acc = acc + torch.matmul(A[ia], Bm[ib])
    return acc


def emulate(x, a, t, gy, w3, w1, prec, *, grid_x=8, flush_steps=FLUSH_STEPS, fault=None):
    """(gx, dW3, dW1) in the kernel's arithmetic.  Operands rounded to records and split into parts; per step (one slice of one 128-pixel column)
    ga = mask_a (W1^T gt) in fp32 from the three products (lo*hi, hi*lo, hi*hi), rounded to the record format and split again; gx through the
    P / Q recurrence of the kernel, rounded to a record; per wave (32 pixels) fp32 accumulators of dW1 and the three taps of dW3, added in
    float64 into the workgroup's block wave after wave every ``flush_steps`` steps and at the end; the blocks summed per lane (blocks l, l + 64, ...)
    and the 64 lane sums in a butterfly.  ``fault`` plants one of the errors tests/test_att_grad.py names."""
    B, C, N, H, W = x.shape
    HW, chunks = H * W, chunks_of(H, W)
    order = ((1, 0), (0, 1), (0, 0)) if prec == "bf16x3" else ((0, 0),)
    on = fault == "ragged_runs_on"
    xp, ap, gp = ([_cols(v, on) for v in cg.round_parts(s, prec)] for s in (x, a, gy))
    tm = _cols(pw.rounded(t, prec), on) > 0
    am = _cols(pw.rounded(t if fault == "mask_a_from_t" else a, prec), on) > 0
    if fault == "t_mask_dropped":
        tm = torch.ones_like(tm)
    w1m = w1[:, :, 0, 0, 0]                                               # [co][ci]
    w1p = [(v if fault == "w1_not_transposed" else v.t()).contiguous() for v in cg.round_parts(w1m, prec)]      # [ci][co]: row operand
    w3k = w3[:, :, :, 0, 0].flip(2) if fault == "taps_reversed" else w3[:, :, :, 0, 0]
    w3p = [[v[:, :, kz].t().contiguous() for v in cg.round_parts(w3k, prec)] for kz in range(3)]                # [kz][part][ci][co]
    gx = torch.zeros(B, N, chunks * P, C)
    blocks = []
    for units in cg.persistent_units(B * chunks, grid_x):
        total = torch.zeros(4, C, C, dtype=torch.float64)
        acc = torch.zeros(WAVES, 4, C, C)
        since, flushed = 0, False
        for uidx in units:
            b, c = divmod(uidx, chunks)
            px = slice(c * P, (c + 1) * P)
            Pn = Qn = ga_prev = x_prev = None
            for n in range(N):
                gtp = [v[b, n, px] * tm[b, n, px] for v in gp]                                                   # (128, C) per part
                d = _mm3(torch.zeros(C, P), w1p, [v.t() for v in gtp], order)                                    # (ci, pixel)
                ga_parts = cg.round_parts(d.t() * am[b, n, px], prec)
                gap_t = [v.t() for v in ga_parts]
                if n > 0:
                    gx[b, n - 1, px] = _mm3(Pn, w3p[0], gap_t, order).t()
                init = sum(v[b, n, px] for v in gp).t()
                if fault == "skip_missing":
                    init = torch.zeros_like(init)
                if n > 0:
                    init = init + Qn
                Pn = _mm3(init, w3p[1], gap_t, order)
                Qn = _mm3(torch.zeros(C, P), w3p[2], gap_t, order)
                wv = lambda v: v.reshape(WAVES, WAVE_PIX, C)
                GT, AA, GA, XX = ([wv(v).transpose(1, 2) for v in gtp], [wv(v[b, n, px]) for v in ap], [wv(v).transpose(1, 2) for v in ga_parts],
                                  [wv(v[b, n, px]) for v in xp])
                acc[:, 3] = _mm3(acc[:, 3], GT, AA, order)
                acc[:, 1] = _mm3(acc[:, 1], GA, XX, order)
                if n > 0:
                    acc[:, 0] = _mm3(acc[:, 0], GA, x_prev, order)
                    acc[:, 2] = _mm3(acc[:, 2], ga_prev, XX, order)
                ga_prev, x_prev = GA, XX
                since += 1
                if since >= flush_steps:
                    for w in range(WAVES):
                        total = total + acc[w].double()
                    acc, since = torch.zeros_like(acc), 0
            last = Pn
            if fault == "next_sample" and b + 1 < B:     # the tap past the sample's last slice reads the next sample's first slice
                gt2 = [v[b + 1, 0, px] * tm[b + 1, 0, px] for v in gp]
                d2 = _mm3(torch.zeros(C, P), w1p, [v.t() for v in gt2], order)
                last = _mm3(Pn, w3p[0], [v.t() for v in cg.round_parts(d2.t() * am[b + 1, 0, px], prec)], order)
            gx[b, N - 1, px] = last.t()
        for w in range(WAVES):
            total = total + acc[w].double()
        blocks.append(total)
    if fault == "missing_partial":
        blocks[max(range(len(blocks)), key=lambda i: float(blocks[i].abs().sum()))] *= 0
    nb = len(blocks)
    lanes = [sum((blocks[i] for i in range(l, nb, 64)), torch.zeros(4, C, C, dtype=torch.float64)) for l in range(64)]
    off = 32
    while off:
        lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
        off >>= 1
    s = lanes[0]
    dw3 = s[:3].permute(1, 2, 0).contiguous().float()[..., None, None]
    dw1 = s[3].float()[..., None, None, None]
    if fault == "dw3_taps_swapped":
        dw3 = dw3.flip(2)
    gx = pw.rounded(gx[:, :, :HW].reshape(B, N, H, W, C).permute(0, 4, 1, 2, 3).contiguous(), prec)
    return gx, dw3, dw1


FAULTS = ("mask_a_from_t", "t_mask_dropped", "w1_not_transposed", "taps_reversed", "next_sample", "ragged_runs_on", "skip_missing", "missing_partial",
          "dw3_taps_swapped")
