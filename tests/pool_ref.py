"""Reference, CPU emulation, input regimes and planted faults for the FORWARD pools on activation records (dffw::pool_kernel, dffw::pool3_kernel,
csrc/dffw_kernels.hip): max (1,2,2), average (1,k,k) for k = 2, 4, 8, and the pyramid's three average pools of one volume in one pass; shared by
tests/test_pool.py (CPU) and tests/test_gpu_pool.py.

The kernels' arithmetic, as read from their code.  A lane takes one row of a k x k window; k adjacent lanes hold one window.
    operands   the stored records: rounded(x, prec), hi + lo joined exactly in fp32 (``stored``: the same value with the sign of a zero kept)
    max        fmaxf over the stored values (exact: the result is one of them)
    avg        every window row summed left to right from 0.f; the k row sums combined by the xor-shuffle tree (offsets 1, 2, 4, each lane adding
               its partner's sum to its own: ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) on the lane that stores); the sum times 1 / k^2, a
               power of two, split into a record
    pyramid    each level by the same rule from the same registers (pool3_kernel), so each level equals the single pool bit for bit
Every step is one IEEE fp32 addition or maximum and the split is ``round_parts``, so ``emulate`` is the kernels' result BIT FOR BIT, and the GPU
tests compare bits.  ``ref64`` is the float64 pool of the unrounded input with ``oracle.error_bounds.pool_ref64``'s bound, which holds the
emulation itself to the project's per-element bound (tests/test_pool.py).

What a bit comparison can see.  A power-of-two scale commutes with every fp32 addition, and for inputs of one magnitude an fp32 sum of k^2 <= 64
record values (8, 11 or 16 significant bits each) is exact or nearly so in any order: on U(-1, 1) the tree order and a flat row-major sum differ in
under 4 % of the windows in bf16x3 and in none in fp16 and bf16.  ``cancelling_pair`` makes the order visible: one +b and one -b per window,
b in [2^14, 2^15], exact in all three formats, so a partial sum that holds b has lost the low bits of the small values added before it.  Order faults
are then observable in most bf16x3 windows (tests/test_pool.py asserts at least 25 %), and in about 5-35 % of the fp16 and bf16 ones.
"""
import torch
import torch.nn.functional as F

from conv_grad_ref import round_parts
from oracle import error_bounds as eb
from pool_grad_ref import same_bits  # noqa: F401
from pw_grad_ref import rounded

PRECISIONS = ("bf16x3", "fp16", "bf16")
FP16_SUB = eb.FP16_SUB
MODES = (("max", 2), ("avg", 2), ("avg", 4), ("avg", 8))
REGIMES = ("zero_mean", "post_relu", "plateau", "rounding_ties", "fp16_small", "cancelling_pair")
# order of the sum; arithmetic; which elements are read; what is stored; the pyramid's levels
FAULTS = ("rows_sequential", "flat_sequential", "tree_truncated", "scale_before_sum", "window_transposed", "window_one_row_down", "lo_dropped",
          "levels_swapped")

# (B, C, N, H, W) of tests/test_gpu_pool.py's pool_kernel cases: one window; B > 1, N > 1, H != W, an odd count of pooled columns (5 at k = 4,
# 3 at k = 8) at one, three and sixteen channel octets; a second slice with five windows per row at k = 8
_MID = {2: (12, 20), 4: (12, 20), 8: (16, 24)}
CASES = {k: [(1, 8, 1, k, k)] + [(2, C, 3) + _MID[k] for C in (8, 24, 128)] + [(1, 8, 2, 8, 40)] for k in (2, 4, 8)}
# 1 179 648 work items at k = 2 against the launch cap of 4096 x 256 threads: 131 072 lanes walk a second item
GRID_STRIDE_CASE = (2, 128, 2, 192, 192)
LAUNCH_CAP = 4096 * 256
# the pyramid's cases: one 8 x 8 block; three octets and an odd count of blocks per row; sixteen octets, five blocks per row; one block per row
PYRAMID_CASES = [(1, 8, 1, 8, 8), (2, 24, 3, 16, 24), (1, 128, 2, 8, 40), (2, 32, 2, 24, 8)]


def work_items(shape, k):
    B, C, N, H, W = shape
    return B * N * (H // k) * (W // k) * (C // 8) * k


def windows(t, k):
    """(B, C, N, H, W) -> (B, C, N, H / k, W / k, k, k): [..., dy, dx]."""
    B, C, N, H, W = t.shape
    return t.reshape(B, C, N, H // k, k, W // k, k).permute(0, 1, 2, 3, 5, 4, 6)


def make_x(regime, shape, k, seed):
    """An input (B, C, N, H, W) float32.  zero_mean: U(-1, 1); post_relu: relu of it (whole windows of stored zeros); plateau: integers in
    {0, 1, 2}; rounding_ties: 1 + 2^-12 U(0, 1), fp32 values that share one bf16 record; fp16_small: the fp16 values nearest +-2^-e (1 + U), e
    uniform in 14 .. 22: fp16 subnormals and the first normal binade, whose averages are fp16 subnormals; being fp16 values (multiples of 2^-24)
    they are their own fp16 and bf16x3 records, so the fp16 error is the result's rounding alone, within FP16_SUB (off that grid every operand
    adds up to FP16_SUB of its own, which pool_ref64's absolute term does not hold: tests/test_pool.py::test_subnormal_inputs_off_the_fp16_grid);
    cancelling_pair: U(-1, 1) plus +b at one and -b at another random position of every k x k window, b = bf16((1 + U) 2^14): at most 2^15, 8 significant bits, so b is exact in all three formats."""
    B, C, N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if regime == "plateau":
        return torch.randint(0, 3, shape, generator=g).float()
    u = torch.rand(shape, generator=g)
    if regime == "rounding_ties":
        return 1 + 2.0 ** -12 * u
    x = 2 * u - 1
    if regime == "zero_mean":
        return x
    if regime == "post_relu":
        return F.relu(x)
    if regime == "fp16_small":
        e = torch.randint(14, 23, shape, generator=g).float()
        return (torch.sign(x) * torch.exp2(-e) * (1 + torch.rand(shape, generator=g))).half().float()
    assert regime == "cancelling_pair", regime
    Ho, Wo = H // k, W // k
    b = rounded((1 + torch.rand(B, C, N, Ho, Wo, generator=g)) * 2.0 ** 14, "bf16")
    assert float(b.max()) <= 2.0 ** 15 and all(torch.equal(rounded(b, p), b) for p in PRECISIONS)
    pos = torch.rand(B, C, N, Ho, Wo, k * k, generator=g).argsort(dim=-1)[..., :2]       # two distinct positions q = k dy + dx
    add = torch.zeros(B, C, N, Ho, Wo, k * k).scatter_(-1, pos, torch.stack((b, -b), dim=-1))
    add = add.reshape(B, C, N, Ho, Wo, k, k).permute(0, 1, 2, 3, 5, 4, 6).reshape(shape)
    return x + add


def stored(t, prec):
    """The value of t's activation record as the kernels join it, with the sign of a zero: ``rounded`` (Python's sum() starts from +0, so its -0
    comes out +0) without that start value.  One part: the part itself; bf16x3: the fp32 sum hi + lo, whose (-0) + (+0) is +0 on the device as well."""
    parts = round_parts(t, prec)
    return parts[0] if len(parts) == 1 else parts[0] + parts[1]


def ref64(x, k, mode):
    """The float64 pool of the UNROUNDED input with the project's per-element bound: a Ref64, ``.ref`` and ``.bound(prec)``."""
    return eb.pool_ref64(x, k, mode)


def _tree(rows, k, steps=None):
    """The xor-shuffle tree over the k row sums ``rows`` [..., k]: every lane adds its partner's value to its own; lane 0 stores."""
    lanes = torch.arange(k)
    off, n = 1, 0
    while off < k and (steps is None or n < steps):
        rows = rows + rows[..., lanes ^ off]
        off, n = off << 1, n + 1
    return rows[..., 0]


def emulate(mode, k, x, prec, fault=None, scale=None):
    """dffw::pool_kernel's result for the fp32 tensor x, in fp32 in the kernel's order (see the module docstring).  ``fault`` plants one of FAULTS:
    rows_sequential     the row sums added in order, ((r0 + r1) + r2) + ..., instead of by the tree (k = 2: the same sum)
    flat_sequential     all k^2 values added in row-major order to one accumulator
    tree_truncated      the last shuffle step missing: the result covers the upper half of the window's rows only
    scale_before_sum    every operand scaled by 1 / k^2 AS A RECORD before the sum.  (In fp32 the scale is a power of two and commutes with every
                        addition: scaling first is then no fault at all.  Folded into the record, it shows where x / k^2 leaves the format's
                        normal range: fp16 on fp16_small.)
    window_transposed   element (dy, dx) read at (dx, dy)
    window_one_row_down every window one input row lower (the last one wraps)
    lo_dropped          a bf16x3 result whose lo plane is zero
    ``scale``: the factor in place of 1 / k^2 (pyramid(): levels_swapped)."""
    assert fault in (None,) + FAULTS and fault != "levels_swapped", fault
    inv = 1.0 / (k * k) if scale is None else scale
    xr = stored(x, prec)
    if fault == "scale_before_sum" and mode == "avg":
        xr = stored(xr * inv, prec)
    if fault == "window_one_row_down":
        xr = torch.roll(xr, -1, dims=3)
    w = windows(xr, k)
    if fault == "window_transposed":
        w = w.transpose(-1, -2)
    if mode == "max":
        assert k == 2
        v = w.amax(dim=(-1, -2)) if fault != "tree_truncated" else w[..., 0, :].amax(dim=-1)
    else:
        assert mode == "avg", mode
        if fault == "flat_sequential":
            v = torch.zeros(w.shape[:-2])
            for dy in range(k):
                for dx in range(k):
                    v = v + w[..., dy, dx]
        else:
            rows = torch.zeros(w.shape[:-1])
            for dx in range(k):
                rows = rows + w[..., dx]
            if fault == "rows_sequential":
                v = rows[..., 0]
                for dy in range(1, k):
                    v = v + rows[..., dy]
            else:
                v = _tree(rows, k, steps=(k.bit_length() - 2) if fault == "tree_truncated" else None)
        if fault != "scale_before_sum":
            v = v * inv
    if fault == "lo_dropped" and prec == "bf16x3":
        return round_parts(v, prec)[0]
    return stored(v, prec)


def pyramid(x, prec, fault=None):
    """dffw::pool3_kernel's (p2, p4, p8): each level by emulate's rule.  levels_swapped: levels 4 and 8 with each other's scale."""
    if fault == "levels_swapped":
        return emulate("avg", 2, x, prec), emulate("avg", 4, x, prec, scale=1.0 / 64), emulate("avg", 8, x, prec, scale=1.0 / 16)
    return tuple(emulate("avg", k, x, prec, fault) for k in (2, 4, 8))


def differing_share(a, b):
    """Share of the elements of two fp32 tensors whose bits differ."""
    return float((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).double().mean())


# ---- the record sweeps of tests/test_gpu_pool.py ---------------------------------------------------------------------------------------------------
SWEEP_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def sweep_values(prec):
    """(v, keep): all 65 536 high halves of an fp32 crossed with SWEEP_LOW_HALVES (every bf16 tie, on both sides of it, toward even and toward
    odd), 393 216 fp32 patterns; ``keep`` is False at NaN and Inf and, for bf16x3, at |v| >= 2^127 (hi overflows and lo is -inf: outside the
    documented domain), where v holds 0 instead."""
    hi = torch.arange(65536, dtype=torch.int64)[:, None]
    bits = ((hi << 16) | torch.tensor(SWEEP_LOW_HALVES, dtype=torch.int64)[None, :]).reshape(-1)
    exp = (bits >> 23) & 0xFF
    keep = exp < (254 if prec == "bf16x3" else 255)
    bits = torch.where(keep, bits, torch.zeros_like(bits))
    v = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
    return v, keep


_FORMAT = {"fp16": (torch.float16, 10, -14), "bf16": (torch.bfloat16, 7, -126)}   # dtype, mantissa bits, least normal exponent


def tie_operands(prec):
    """(a, b) float32, for fp16 / bf16: a = every finite value t of the format, b = c ulp(t) for c in +-1/4, +-1/2, +-3/4 wherever that is a
    value of the format too.  a + b is exact in fp32 and sits below, on and above the midpoint of t and its neighbour."""
    dtype, mant, emin = _FORMAT[prec]
    t = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    t = t[torch.isfinite(t.float())].double()
    e = torch.where(t == 0, torch.full_like(t, emin), (torch.frexp(t.abs())[1] - 1).double().clamp_min(emin))
    ulp = torch.exp2(e - mant)
    a, b = [], []
    for c in (0.25, -0.25, 0.5, -0.5, 0.75, -0.75):
        bc = c * ulp
        ok = bc.to(dtype).double() == bc
        a.append(t[ok])
        b.append(bc[ok])
    a, b = torch.cat(a), torch.cat(b)
    assert torch.equal((a + b).float().double(), a + b)
    return a.float(), b.float()
