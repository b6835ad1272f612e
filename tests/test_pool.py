"""CPU tests of tests/pool_ref.py, the reference and emulation behind tests/test_gpu_pool.py (forward pools on activation records).

The emulation against float64.  At every pool_kernel case of the GPU test, in every regime, precision and k, ``emulate`` stays within
``oracle.error_bounds.pool_ref64``'s bound of the float64 pool of the unrounded input.  Worst err / bound per regime (bf16x3 / fp16 / bf16):
    zero_mean 0.499 / 0.498 / 0.497    post_relu 0.499 / 0.498 / 0.497    plateau 0 / 0 / 0    rounding_ties 0.031 / 0.250 / 0.031
    fp16_small 0 / 0.987 / 0.498       cancelling_pair 0.015 / 0.062 / 0.008
(fp16_small in fp16 is the result's subnormal rounding against FP16_SUB alone: its inputs are fp16 values.  With inputs OFF the fp16 grid the
emulation reaches 1.72 x that bound: every operand's own subnormal rounding, up to FP16_SUB each and so up to FP16_SUB in the mean, is not in
pool_ref64's absolute term, which holds the output's only.  test_subnormal_inputs_off_the_fp16_grid holds that case to alpha D + 2 FP16_SUB.)

Which planted fault changes bits where, at the GPU test's case (2, 8, 3, 12, 20) (k = 8: (2, 8, 3, 16, 24)); the share of differing elements:
    fault                 mode, k          regime            bf16x3   fp16    bf16
    rows_sequential       avg 4 / 8        cancelling_pair   38/71 %  17/32 % 4/8 %     (k = 2: the same sum by construction)
    flat_sequential       avg 2 / 4 / 8    cancelling_pair   52-98 %  37-67 % 4-14 %
    tree_truncated        max 2, avg *     every regime      28-100 % (rounding_ties under max: bf16x3 only, the other records are all equal)
    scale_before_sum      avg 2 / 4 / 8    fp16_small        -        43-84 % -         (a power-of-two scale commutes with fp32 addition: the
                                                                                         fault exists only as a scale folded into the record)
    window_transposed     avg 2 / 4 / 8    cancelling_pair   67-91 %  48-72 % 6-19 %    (the same elements in another order: never under max)
    window_one_row_down   max 2, avg *     every regime      22-100 % (rounding_ties: bf16x3 only)
    lo_dropped            max 2, avg *     all but plateau   39-100 % -       -
    levels_swapped        pyramid          every regime      p4 and p8 differ wherever they are not zero
Order faults (rows_sequential, flat_sequential, window_transposed) are observable under ``cancelling_pair`` only, and reliably in bf16x3 only: on
U(-1, 1) the tree and the flat order differ in about 4 % of the bf16x3 windows at k = 8 (under 1 % at k = 4, none at k = 2) and in NO fp16 or
bf16 window; under cancelling_pair in 50 / 90 / 98 % of the bf16x3 windows at k = 2 / 4 / 8 (40 / 71 % against rows_sequential at k = 4 / 8),
and in about 5-35 % (rows) and 3-67 % (flat) of the 16-bit formats'.  test_order_faults_are_visible asserts the 25 % the GPU test relies on.
"""
import ctypes
import functools

import pytest
import torch

import pool_ref as pr
from oracle import error_bounds as eb

PRECS = pr.PRECISIONS
MID = {2: (2, 8, 3, 12, 20), 4: (2, 8, 3, 12, 20), 8: (2, 8, 3, 16, 24)}
ALL_K = tuple(k for _, k in pr.MODES if _ == "avg")
# fault -> the (mode, k, regime, precision) at which the GPU test's data must show it
CAUGHT = {
    "rows_sequential": [("avg", k, "cancelling_pair", p) for k in (4, 8) for p in PRECS],
    "flat_sequential": [("avg", k, "cancelling_pair", p) for k in ALL_K for p in PRECS],
    "tree_truncated": [(m, k, r, p) for m, k in pr.MODES for r in pr.REGIMES for p in PRECS if not (m == "max" and r == "rounding_ties" and p != "bf16x3")],
    "scale_before_sum": [("avg", k, "fp16_small", "fp16") for k in ALL_K],
    "window_transposed": [("avg", k, "cancelling_pair", p) for k in ALL_K for p in PRECS],
    "window_one_row_down": [(m, k, r, p) for m, k in pr.MODES for r in pr.REGIMES for p in PRECS if not (r == "rounding_ties" and p != "bf16x3")],
    "lo_dropped": [(m, k, r, "bf16x3") for m, k in pr.MODES for r in pr.REGIMES if r != "plateau"],
}


@functools.lru_cache(maxsize=None)
def _x(regime, shape, k):
    return pr.make_x(regime, shape, k, 7 + sum(shape) + k)


def test_the_regimes_are_what_they_claim():
    shape = MID[2]
    assert float((pr.windows(pr.rounded(_x("post_relu", shape, 2), "bf16x3"), 2).abs().amax(dim=(-1, -2)) == 0).double().mean()) > 0.03
    ties = _x("rounding_ties", shape, 2)
    assert ties.unique().numel() > 1000 and pr.rounded(ties, "bf16").unique().numel() == 1
    small = _x("fp16_small", shape, 2)
    assert torch.equal(small.half().float(), small) and float(small.abs().max()) <= 2.0 ** -13 and float(small.abs().min()) >= 2.0 ** -23
    for k in ALL_K:
        avg = pr.emulate("avg", k, _x("fp16_small", MID[k], k), "fp16")
        assert float((avg.abs() < 2.0 ** -14).double().mean()) > 0.9       # nearly every average is an fp16 subnormal
        x = _x("cancelling_pair", MID[k], k)
        big = pr.windows(x, k).reshape(x.shape[0], x.shape[1], x.shape[2], MID[k][3] // k, MID[k][4] // k, k * k)
        assert bool(((big > 2.0 ** 13).sum(-1) == 1).all()) and bool(((big < -2.0 ** 13).sum(-1) == 1).all()) and float(x.abs().max()) < 65504
        for prec in PRECS:      # +b and -b are stored exactly: the window's stored sum has no trace of them
            xr = pr.windows(pr.rounded(x, prec), k).reshape(big.shape).double()
            assert float(xr.sum(-1).abs().max()) <= k * k


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_emulation_holds_the_float64_bound(regime, prec):
    """|emulate - float64 pool of the unrounded input| <= pool_ref64's bound, per element, at every pool_kernel case of the GPU test."""
    worst = 0.0
    for mode, k in pr.MODES:
        for shape in pr.CASES[k]:
            x = _x(regime, shape, k)
            worst = max(worst, eb.check_elementwise(pr.emulate(mode, k, x, prec), pr.ref64(x, k, mode), prec, "%s k=%d %s %s" % (mode, k, shape, regime)))
    print("pool emulation %s %s: worst err/bound %.3f" % (regime, prec, worst))
    for shape in pr.PYRAMID_CASES:
        x = _x(regime, shape, 8)
        for k, p in zip((2, 4, 8), pr.pyramid(x, prec)):
            assert pr.same_bits(p, pr.emulate("avg", k, x, prec))
            eb.check_elementwise(p, pr.ref64(x, k, "avg"), prec, "pyramid level %d %s %s" % (k, shape, regime))


def test_subnormal_inputs_off_the_fp16_grid():
    """Why fp16_small draws fp16 values: off that grid each operand's subnormal rounding (up to FP16_SUB) enters the mean beside the result's own,
    and pool_ref64's absolute term holds one FP16_SUB.  The emulation exceeds that bound there and stays within alpha D + 2 FP16_SUB."""
    g = torch.Generator().manual_seed(3)
    over = 0.0
    for k in ALL_K:
        shape = MID[k]
        x = torch.exp2(-torch.randint(14, 23, shape, generator=g).float()) * (1 + torch.rand(shape, generator=g)) * torch.sign(torch.rand(shape, generator=g) - 0.5)
        r = pr.ref64(x, k, "avg")
        err = (pr.emulate("avg", k, x, "fp16").double() - r.ref).abs()
        assert bool((err <= r.bound("fp16") + eb.FP16_SUB).all())
        over = max(over, float((err / r.bound("fp16")).max()))
    assert over > 1.0


@pytest.mark.parametrize("fault", [f for f in pr.FAULTS if f != "levels_swapped"])
def test_planted_faults_change_bits(fault):
    """Each fault changes the bits of at least one element at every (mode, k, regime, precision) the table above names, on the GPU test's data."""
    for mode, k, regime, prec in CAUGHT[fault]:
        x = _x(regime, MID[k], k)
        assert not pr.same_bits(pr.emulate(mode, k, x, prec), pr.emulate(mode, k, x, prec, fault)), (fault, mode, k, regime, prec)
    if fault == "rows_sequential":      # at k = 2 the two orders are one sum
        x = _x("cancelling_pair", MID[2], 2)
        assert pr.same_bits(pr.emulate("avg", 2, x, "bf16x3"), pr.emulate("avg", 2, x, "bf16x3", fault))
    if fault == "scale_before_sum":     # no fault in the bf16 formats, whose exponent range the scale stays inside
        for regime in pr.REGIMES:
            x = _x(regime, MID[8], 8)
            assert all(pr.same_bits(pr.emulate("avg", 8, x, p), pr.emulate("avg", 8, x, p, fault)) for p in ("bf16x3", "bf16"))


@pytest.mark.parametrize("prec", PRECS)
def test_pyramid_faults_change_bits(prec):
    for shape in pr.PYRAMID_CASES:
        for regime in pr.REGIMES:
            x = _x(regime, shape, 8)
            p2, p4, p8 = pr.pyramid(x, prec)
            q2, q4, q8 = pr.pyramid(x, prec, "levels_swapped")
            assert pr.same_bits(p2, q2) and not pr.same_bits(p4, q4) and not pr.same_bits(p8, q8), (shape, regime)
    x = _x("cancelling_pair", pr.PYRAMID_CASES[1], 8)
    for fault in ("flat_sequential", "rows_sequential", "tree_truncated", "window_one_row_down"):
        assert not any(pr.same_bits(a, b) for a, b in list(zip(pr.pyramid(x, prec), pr.pyramid(x, prec, fault)))[1:]), fault


def test_order_faults_are_visible():
    """What keeps the GPU comparison from being blind to the order of the sum: under cancelling_pair at bf16x3 at least 25 % of the windows differ
    between the tree order and flat_sequential at k = 2, 4, 8, and between it and rows_sequential at k = 4, 8; on U(-1, 1) under 5 % do in
    bf16x3 and none in fp16 and bf16."""
    shape = (2, 8, 2, 32, 48)
    for k in ALL_K:
        x = pr.make_x("cancelling_pair", shape, k, 5)
        share = {(p, f): pr.differing_share(pr.emulate("avg", k, x, p), pr.emulate("avg", k, x, p, f)) for p in PRECS for f in ("flat_sequential", "rows_sequential")}
        print("cancelling_pair k=%d: " % k + "  ".join("%s %s %.1f %%" % (p, f[:4], 100 * s) for (p, f), s in share.items()))
        assert share[("bf16x3", "flat_sequential")] >= 0.25
        if k > 2:
            assert share[("bf16x3", "rows_sequential")] >= 0.25
        else:
            assert all(share[(p, "rows_sequential")] == 0.0 for p in PRECS)
        u = pr.make_x("zero_mean", shape, k, 5)
        for f in ("flat_sequential", "rows_sequential"):
            assert pr.differing_share(pr.emulate("avg", k, u, "bf16x3"), pr.emulate("avg", k, u, "bf16x3", f)) < 0.05
            assert all(pr.differing_share(pr.emulate("avg", k, u, p), pr.emulate("avg", k, u, p, f)) == 0.0 for p in ("fp16", "bf16"))


def test_the_grid_stride_case_walks_a_second_item():
    items = pr.work_items(pr.GRID_STRIDE_CASE, 2)
    assert items == 1179648 and pr.LAUNCH_CAP < items < 2 * pr.LAUNCH_CAP and pr.LAUNCH_CAP % 64 == 0
    assert all(pr.work_items(s, k) < pr.LAUNCH_CAP for k in ALL_K for s in pr.CASES[k])


def test_the_sweeps_cover_what_they_claim():
    """Sweep (a): 393 216 fp32 patterns, NaN / Inf left out (1 536) and, for bf16x3, |v| >= 2^127 (1 536 more).  Sweep (b): every finite value of
    the 16-bit format with the quarter-ulp offsets that are values of the format; each sum exact in fp32."""
    for prec, kept in (("bf16x3", 390144), ("fp16", 391680), ("bf16", 391680)):
        v, keep = pr.sweep_values(prec)
        assert v.numel() == 393216 and int(keep.sum()) == kept and bool(torch.isfinite(v).all())
        assert bool((v[~keep] == 0).all()) and float(v[keep].abs().max()) < (2.0 ** 127 if prec == "bf16x3" else float("inf"))
        lows = (v.view(torch.int32) & 0xFFFF).reshape(65536, 6)[256]
        assert lows.tolist() == list(pr.SWEEP_LOW_HALVES)
    for prec, n in (("fp16", 348160), ("bf16", 387584)):
        a, b = pr.tie_operands(prec)
        assert a.numel() == b.numel() == n and torch.equal(pr.rounded(a, prec), a) and torch.equal(pr.rounded(b, prec), b)
        s = a + b
        on_tie = pr.rounded(s, prec) != s
        assert int(on_tie.sum()) > n // 2 and int((~on_tie).sum()) > 0      # between two values of the format, and some on one (at a binade's edge)


def test_op_pool3_abi_and_refusals_without_gpu(lib_built):
    """dffw_op_pool3 is exported, declared and bound; C, H or W no multiple of 8, a bad precision, a bad shape or a null tensor is DFFW_EINVAL
    (-1) with a message before the GPU is touched (dummy addresses stand for the tensors)."""
    import os
    from dffinthewild_amd import engine
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dffw.h")).read()
    assert "int dffw_op_pool3(" in header and "dffw_op_pool3" in engine.ABI_SYMBOLS and callable(engine.op_pool3)
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dffw_op_pool3.argtypes = [ci, ci, vp] + [ci] * 5 + [vp] * 4
    P = 4096

    def call(prec=0, x=P, shape=(1, 8, 2, 8, 8), p2=P, p4=P, p8=P):
        return lib.dffw_op_pool3(0, prec, x, *shape, p2, p4, p8, None)

    for what, kw in (("C % 8", dict(shape=(1, 12, 2, 8, 8))), ("H % 8", dict(shape=(1, 8, 2, 12, 8))), ("W % 8", dict(shape=(1, 8, 2, 8, 20))),
                     ("C = 0", dict(shape=(1, 0, 2, 8, 8))), ("B = 0", dict(shape=(0, 8, 2, 8, 8))), ("H = -8", dict(shape=(1, 8, 2, -8, 8))),
                     ("precision 3", dict(prec=3)), ("precision -1", dict(prec=-1)),
                     ("null x", dict(x=None)), ("null p2", dict(p2=None)), ("null p4", dict(p4=None)), ("null p8", dict(p8=None))):
        assert call(**kw) == -1 and lib.dffw_last_error(), what
