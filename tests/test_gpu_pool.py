"""The forward pools and the activation records themselves on the GPU, BIT FOR BIT (tests/pool_ref.py; its CPU tests are tests/test_pool.py).

No tolerance anywhere: every step of dffw::pool_kernel / pool3_kernel is one IEEE fp32 addition or maximum, the scale is a power of two and the
split is ``round_parts``, so the kernels must give the bits of the CPU emulation.

(a) record sweep through the software split (Fmt::split: from_ncdhw_kernel's and pool_kernel's): op_pool(max, 2) of windows of four equal values,
    all 65 536 high halves of an fp32 x six low halves around the bf16 tie = 393 216 patterns; NaN / Inf left out (1 536) and for bf16x3
    |v| >= 2^127 (1 536 more, outside the documented domain).  Expected: the bits of rounded(v), the sign of zero included (pool_ref.stored, applied twice as the op does).
(b) record sweep through the hardware pack (Fmt::split2 in store8): op_grad_combine(a, b=b) = store8(load8(a) + load8(b)).  bf16x3: a = bf16(v),
    b = v - a, both exact records from 2^-110 up, so the sum is sweep (a)'s arbitrary fp32 v (390 144 compared).  fp16 / bf16: a = every finite value t of the
    format, b = +-1/4, +-1/2, +-3/4 ulp(t) where that is a value of the format (348 160 / 387 584 sums, exact in fp32, below, on and above a tie).
    (a) and (b) together: Fmt::split, Fmt::split2 and the CPU's round_parts are one function on every finite value.
(c) pool_kernel against pool_ref.emulate: max k = 2, avg k = 2, 4, 8, every regime and precision, at pool_ref.CASES and one grid-stride case.
(d) dffw_op_pool3 (pool3_kernel) against op_pool(avg, k) and pool_ref.pyramid at pool_ref.PYRAMID_CASES; its kernel name; its refusals.
The pooled copies of the SRD block are held to max_pool(y) bit for bit in tests/test_gpu_blocks.py."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP_SHAPE = (1, 8, 1, 192, 256)     # 393 216 elements


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def bits(t):
    return t.detach().cpu().float().contiguous().view(torch.int32)


def assert_same_bits(got, want, what, keep=None):
    """Every element (where ``keep``) equal bit for bit: +0 and -0 differ, a NaN left by the poisoned workspace differs from every expected value."""
    g, w = bits(got), bits(want)
    bad = g != w
    if keep is not None:
        bad &= keep.reshape(bad.shape)
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: %d of %d elements differ; first at flat index %d: got 0x%08x, expected 0x%08x" % (
            what, n, bad.numel(), i, int(g.reshape(-1)[i]) & 0xFFFFFFFF, int(w.reshape(-1)[i]) & 0xFFFFFFFF))


@functools.lru_cache(maxsize=None)
def case_x(regime, shape, k):
    return pr.make_x(regime, shape, k, 7 + sum(shape) + k)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", pr.PRECISIONS)
def test_record_sweep_software_split(eng, prec):
    v, keep = pr.sweep_values(prec)
    assert int(keep.sum()) == (390144 if prec == "bf16x3" else 391680)
    x = v.reshape(SWEEP_SHAPE).repeat_interleave(2, 3).repeat_interleave(2, 4)       # (1, 8, 1, 384, 512): every window four equal values
    got = eng.op_pool(x.cuda(), 2, "max", prec)
    # the op splits twice, staging in and storing the maximum: the same VALUE as one split, rounded(v); in bf16x3 the second split of a -0 gives
    # (hi, lo) = (-0, (-0) - (-0) = +0), so the three negative fp32 subnormals whose record is (-0, -0) come back as +0, as round_parts has it
    once = pr.stored(v, prec)
    want = pr.stored(once, prec)
    assert torch.equal(want, pr.rounded(v, prec)) and int((bits(want) != bits(once)).sum()) == (3 if prec == "bf16x3" else 0)
    want = want.reshape(SWEEP_SHAPE)
    assert_same_bits(got, want, "software split %s" % prec, keep)
    print("record sweep (a) %s: %d patterns compared, %d left out" % (prec, int(keep.sum()), int((~keep).sum())))


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", pr.PRECISIONS)
def test_record_sweep_hardware_pack(eng, prec):
    if prec == "bf16x3":
        v, keep = pr.sweep_values(prec)
        a = pr.rounded(v, "bf16")
        b = v - a
        # a and b are exact records and a + b is v, except below 2^-110, where v - a has bits under bf16's least subnormal 2^-133: there b is
        # rounded to its record first, as the formula below has it
        inexact = pr.rounded(b, prec) != b
        assert torch.equal(a.double() + b.double(), v.double()) and torch.equal(pr.rounded(a, prec), a) and not bool(inexact[v.abs() >= 2.0 ** -110].any())
        print("record sweep (b) bf16x3: b is no exact record for %d patterns below 2^-110" % int(inexact.sum()))
    else:
        a, b = pr.tie_operands(prec)
        keep = torch.ones(a.numel(), dtype=torch.bool)
    n = a.numel()
    numel = SWEEP_SHAPE[1] * SWEEP_SHAPE[3] * SWEEP_SHAPE[4]
    assert n <= numel
    pad = lambda t: torch.cat((t, torch.zeros(numel - n))).reshape(SWEEP_SHAPE)
    a, b, keep = pad(a), pad(b), torch.cat((keep, torch.zeros(numel - n, dtype=torch.bool)))
    got = eng.op_grad_combine(a.cuda(), b=b.cuda(), precision=prec)
    want = pr.stored((pr.stored(a, prec) + pr.stored(b, prec)).float(), prec)
    assert torch.equal(want, pr.rounded((pr.rounded(a, prec) + pr.rounded(b, prec)).float(), prec))
    assert_same_bits(got, want, "hardware pack %s" % prec, keep)
    print("record sweep (b) %s: %d sums compared" % (prec, int(keep.sum())))


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", pr.PRECISIONS)
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_pool_kernel_equals_the_emulation(eng, regime, prec):
    for mode, k in pr.MODES:
        for shape in pr.CASES[k]:
            x = case_x(regime, shape, k)
            got = eng.op_pool(x.cuda(), k, mode, prec)
            assert_same_bits(got, pr.emulate(mode, k, x, prec), "pool_kernel %s k=%d %s %s %s" % (mode, k, shape, regime, prec))


@functools.lru_cache(maxsize=None)
def grid_stride_x():
    return pr.make_x("cancelling_pair", pr.GRID_STRIDE_CASE, 2, 41)


@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_pool_kernel_grid_stride(eng, prec):
    """1 179 648 work items on 4096 x 256 threads: 131 072 lanes take a second item, whose rows meet in the shuffle of the second iteration."""
    assert pr.work_items(pr.GRID_STRIDE_CASE, 2) > pr.LAUNCH_CAP
    x = grid_stride_x()
    xd = x.cuda()
    for mode in ("max", "avg"):
        assert_same_bits(eng.op_pool(xd, 2, mode, prec), pr.emulate(mode, 2, x, prec), "pool_kernel grid stride %s %s" % (mode, prec))


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", pr.PRECISIONS)
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_pool3_equals_three_pools(eng, regime, prec):
    """dffw_op_pool3's three outputs: the bits of op_pool(avg, k) and of the emulation, every element finite (the op's workspace is poisoned), by
    the kernel the forward's pyramid launches."""
    for shape in pr.PYRAMID_CASES:
        x = case_x(regime, shape, 8)
        xd = x.cuda()
        ps = eng.op_pool3(xd, prec)
        assert eng.op_kernels() == ["dffw::pool3_kernel<%d>" % eng.PRECISIONS[prec]]
        B, C, N, H, W = shape
        for k, p, e in zip((2, 4, 8), ps, pr.pyramid(x, prec)):
            what = "pool3 level %d %s %s %s" % (k, shape, regime, prec)
            assert tuple(p.shape) == (B, C, N, H // k, W // k) and bool(torch.isfinite(p).all()), what
            assert_same_bits(p, eng.op_pool(xd, k, "avg", prec), what + " vs op_pool")
            assert_same_bits(p, e, what + " vs emulation")


def test_pool3_refusals(eng):
    x = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    for bad in ((1, 12, 2, 8, 8), (1, 8, 2, 12, 8), (1, 8, 2, 8, 20), (1, 8, 2, 4, 8)):
        with pytest.raises(ValueError):
            eng.op_pool3(torch.zeros(bad, device="cuda"))
        assert eng.op_kernels() == []
    with pytest.raises(KeyError):
        eng.op_pool3(x, "fp8")
    assert all(bool((p == 0).all()) for p in eng.op_pool3(x))


def test_pipeline_pyramid_is_one_pass(eng):
    """pipeline.avg_pool_pyramid's forward is the one pool3_kernel launch, with op_pool's bits."""
    from dffinthewild_amd import pipeline
    x = case_x("cancelling_pair", pr.PYRAMID_CASES[1], 8).cuda()
    ps = pipeline.avg_pool_pyramid(x, precision="bf16x3")
    assert eng.op_kernels() == ["dffw::pool3_kernel<0>"]
    for k, p in zip((2, 4, 8), ps):
        assert_same_bits(p, eng.op_pool(x, k, "avg", "bf16x3"), "pipeline pyramid level %d" % k)
