"""Reference, bounds and a CPU emulation for the backward of the pools: max (1,2,2), average (1,k,k) and the pyramid's three
average pools in one pass, each optionally added to a second gradient b; shared by tests/test_pool_grad.py and tests/test_gpu_pool_grad.py.

Reference: float64 ``torch.autograd.grad`` of ``F.max_pool3d`` / ``F.avg_pool3d`` on the CPU, on the RECORD-ROUNDED operands: the kernels read
stored records, so a tie is a tie of stored values, and torch's CPU max pool sends a tied window's gradient to the first maximum in row-major
window order (test_pool_grad.py asserts it).

Bounds, derived from the arithmetic (u = section 14's unit roundoff of one stored record, pw_grad_ref.U):

    max without b     exact: the bits of rounded(g) at the argmax, +0 elsewhere
    avg without b     exact for bf16x3 and bf16 (g * k^-2 is a record value again); fp16: |err| <= FP16_SUB, g * k^-2 may fall below the normal range
    either with b     (u + 2^-23) |ref64|: one fp32 addition of two exact values, one split (section 15's bound); + FP16_SUB for fp16 avg
    pyramid           (u + 2^-22) S, S = |g8| / 64 + |g4| / 16 + |g2| / 4 + |b|: three fp32 additions of at most 2^-24 each relative to partial
                      sums of at most S, then one split of a value of at most (1 + 3 * 2^-24) S; + FP16_SUB for fp16
"""
import torch
import torch.nn.functional as F

from conv_grad_ref import round_parts  # noqa: F401
from oracle import error_bounds as eb
from pw_grad_ref import U, rounded

PRECISIONS = ("bf16x3", "fp16", "bf16")
FP16_SUB = eb.FP16_SUB
FAULTS = ("tie_last", "tie_all", "argmax_unrounded", "window_transposed", "levels_swapped", "b_dropped")

# (B, N, H, W) of the pools' input and the channel counts, per form, of tests/test_gpu_pool_grad.py: one window / one block; B > 1, N > 1,
# H != W, an odd count of pooled columns (10 at k = 2, 5 at k = 4) or of blocks per row (3), a ragged last unit (1 440 = 2.8 and 2 304 = 4.5
# units of 512 pixels), at 8, 24 (three octets) and 128 channels; a volume whose 40 units every workgroup of a grid of 8 walks several of
SMALL_GRID = ((2, 10, 32, 32), 32)
_MID2 = [((2, 3, 12, 20), C) for C in (8, 24, 128)]
_MID8 = [((2, 3, 16, 24), C) for C in (8, 24, 128)]
CASES = {
    ("max", 2): [((1, 1, 2, 2), 8)] + _MID2 + [SMALL_GRID],
    ("avg", 2): [((1, 1, 2, 2), 8)] + _MID2 + [SMALL_GRID],
    ("avg", 4): _MID2 + [SMALL_GRID],
    ("avg", 8): [((1, 1, 8, 8), 8)] + _MID8 + [SMALL_GRID],
    ("pyramid", 8): [((1, 1, 8, 8), 8)] + _MID8 + [SMALL_GRID],
}
X_REGIMES = ("zero_mean", "post_relu", "plateau", "rounding_ties")
G_REGIMES = ("zero_mean", "offset")


def make_x(regime, shape, C, seed):
    """The max pool's input (B, C, N, H, W) float32: U(-1, 1); relu of it (whole windows of stored zeros); integers in {0, 1, 2} (plateaus);
    1 + 2^-12 U(0, 1): distinct fp32 values that share one bf16 record, so that under bf16 every window is a tie the first element must win."""
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if regime == "plateau":
        return torch.randint(0, 3, (B, C, N, H, W), generator=g).float()
    u = torch.rand(B, C, N, H, W, generator=g)
    if regime == "rounding_ties":
        return 1 + 2.0 ** -12 * u
    x = 2 * u - 1
    if regime == "post_relu":
        return F.relu(x)
    assert regime == "zero_mean", regime
    return x


def make_g(regime, shape, C, k, seed):
    """A gradient at the pooled resolution (B, C, N, H / k, W / k) (k = 1: at the input's, a `b`): U(-1, 1), or 1 + 0.25 U(-1, 1)."""
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    v = 2 * torch.rand(B, C, N, H // k, W // k, generator=g) - 1
    if regime == "offset":
        return 1 + 0.25 * v
    assert regime == "zero_mean", regime
    return v


def int_g(shape, C, k, seed):
    """Small integers times 64: the pyramid's three scales and every sum of them stay exact in every format."""
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (B, C, N, H // k, W // k), generator=g).float() * (1.0 if k == 1 else 64.0)


def tie_share(x, prec):
    """Share of the 2x2 windows of x whose stored maximum is held by more than one element."""
    xr = rounded(x, prec)
    B, C, N, H, W = xr.shape
    w = xr.reshape(B, C, N, H // 2, 2, W // 2, 2)
    m = w.amax(dim=(4, 6), keepdim=True)
    return float(((w == m).sum(dim=(4, 6)) > 1).double().mean())


def up(t, k):
    return t.repeat_interleave(k, 3).repeat_interleave(k, 4)


# ---- float64 autograd ---------------------------------------------------------------------------------------------------------------------------
def pool_ref64(g, x, b, k, mode, prec):
    """(ref64, bound) of the (1,k,k) pool's input gradient (+ b), from the record-rounded operands."""
    gr = rounded(g, prec).double()
    if mode == "max":
        assert k == 2
        xr = rounded(x, prec).double().requires_grad_(True)
        ref, = torch.autograd.grad(F.max_pool3d(xr, (1, 2, 2)), xr, gr)
    else:
        B, C, N, Ho, Wo = g.shape
        z = torch.zeros(B, C, N, Ho * k, Wo * k, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(F.avg_pool3d(z, (1, k, k)), z, gr)
    sub = FP16_SUB if (prec == "fp16" and mode == "avg") else 0.0
    if b is None:
        return ref, torch.full_like(ref, sub)
    ref = ref + rounded(b, prec).double()
    return ref, (U[prec] + 2.0 ** -23) * ref.abs() + sub


def pool3_ref64(g2, g4, g8, b, prec):
    """(ref64, bound) of the pyramid's input gradient (+ b)."""
    r2, r4, r8 = (rounded(t, prec).double() for t in (g2, g4, g8))
    B, C, N, H8, W8 = g8.shape
    z = torch.zeros(B, C, N, 8 * H8, 8 * W8, dtype=torch.float64, requires_grad=True)
    y = (F.avg_pool3d(z, (1, 2, 2)) * r2).sum() + (F.avg_pool3d(z, (1, 4, 4)) * r4).sum() + (F.avg_pool3d(z, (1, 8, 8)) * r8).sum()
    ref, = torch.autograd.grad(y, z)
    S = up(r8.abs(), 8) / 64 + up(r4.abs(), 4) / 16 + up(r2.abs(), 2) / 4
    if b is not None:
        br = rounded(b, prec).double()
        ref, S = ref + br, S + br.abs()
    return ref, (U[prec] + 2.0 ** -22) * S + (FP16_SUB if prec == "fp16" else 0.0)


# ---- the kernels' arithmetic --------------------------------------------------------------------------------------------------------------------
def emulate(mode, prec, *, k=2, g=None, x=None, b=None, g2=None, g4=None, g8=None, fault=None):
    """dffw::pool_bwd_kernel (mode "max" / "avg") and dffw::pool3_bwd_kernel (mode "pyramid") in fp32, in the kernels' order: the argmax is the
    first element, in row-major window order, that no later one exceeds, among the STORED values of x; without b a max gradient is g's record or
    +0; every other result is formed in fp32 -- g * k^-2, ((g8 / 64 + g4 / 16) + g2 / 4), then + b -- and split once.  ``fault`` plants one of
    FAULTS."""
    assert fault in (None,) + FAULTS, fault
    br = None if (b is None or fault == "b_dropped") else rounded(b, prec)
    if mode == "pyramid":
        s8, s4 = (2.0 ** -4, 2.0 ** -6) if fault == "levels_swapped" else (2.0 ** -6, 2.0 ** -4)
        v = (up(rounded(g8, prec), 8) * s8 + up(rounded(g4, prec), 4) * s4) + up(rounded(g2, prec), 2) * 0.25
        return rounded(v if br is None else v + br, prec)
    gr = rounded(g, prec)
    if mode == "avg":
        v = up(gr, k) * (1.0 / (k * k))
        return rounded(v if br is None else v + br, prec)
    assert mode == "max" and k == 2
    xs = x.float() if fault == "argmax_unrounded" else rounded(x, prec)
    B, C, N, H, W = xs.shape
    w = xs.reshape(B, C, N, H // 2, 2, W // 2, 2).permute(0, 1, 2, 3, 5, 4, 6).reshape(B, C, N, H // 2, W // 2, 4)   # q = 2 dy + dx
    best, first = w[..., 0], torch.zeros(w.shape[:-1], dtype=torch.long)
    for q in range(1, 4):
        wins = w[..., q] >= best if fault == "tie_last" else w[..., q] > best
        best, first = torch.where(wins, w[..., q], best), torch.where(wins, torch.full_like(first, q), first)
    if fault == "window_transposed":
        first = torch.tensor([0, 2, 1, 3])[first]
    sel = w == best[..., None] if fault == "tie_all" else first[..., None] == torch.arange(4)
    out = torch.where(sel, gr[..., None], torch.zeros(()))
    out = out.reshape(B, C, N, H // 2, W // 2, 2, 2).permute(0, 1, 2, 3, 5, 4, 6).reshape(B, C, N, H, W)
    return out if br is None else rounded(out + br, prec)


def check(got, ref, bound, what=""):
    """max err / bound over every element (0 / 0 = 0); asserts that none exceeds 1.  NaN fails."""
    err = (got.detach().cpu().double() - ref).abs()
    ratio = eb._ratio(err, bound)
    worst = float(ratio.max())
    assert worst <= 1.0, "%s: %d of %d elements over the bound, worst err/bound %.3g" % (what, int((ratio > 1).sum()), ratio.numel(), worst)
    return worst


def same_bits(a, b):
    """fp32 tensors equal bit for bit (so +0 and -0 differ)."""
    return torch.equal(a.detach().cpu().float().contiguous().view(torch.int32), b.detach().cpu().float().contiguous().view(torch.int32))
