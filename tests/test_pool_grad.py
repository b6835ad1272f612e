"""CPU tests of the reference, the bounds and the emulation of tests/pool_grad_ref.py (backward of the pools): the kernels'
arithmetic stays under its bounds at every shape of tests/test_gpu_pool_grad.py (bit-equal where the bound is zero, and on small-integer data
throughout); every planted fault breaks its check; the built library refuses what it does not serve without touching a GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pool_grad_ref as pg

PRECS = pg.PRECISIONS


def _seed(shape, C):
    return 11 + C + sum(shape)


def test_torch_sends_a_tie_to_the_first_maximum():
    """What the reference rests on: float64 CPU max_pool3d gives a tied window's gradient to its first maximum in row-major order."""
    for vals, want in (([0, 0, 0, 0], 0), ([1, 2, 2, 0], 1), ([0, 1, 1, 1], 1), ([0, 0, 3, 3], 2), ([-0.0, 0.0, 0.0, -0.0], 0)):
        x = torch.tensor(vals, dtype=torch.float64).reshape(1, 1, 1, 2, 2).requires_grad_(True)
        g, = torch.autograd.grad(F.max_pool3d(x, (1, 2, 2)), x, torch.ones(1, 1, 1, 1, 1, dtype=torch.float64))
        assert g.reshape(-1).tolist() == [float(i == want) for i in range(4)], (vals, g.reshape(-1).tolist())


@pytest.mark.parametrize("prec", PRECS)
def test_max_emulation_is_exact(prec):
    """Without b: the bits of rounded(g) at the argmax, +0 with the sign bit clear elsewhere, in every regime of x (rounding-born ties under
    bf16, where they arise).  With b: under (u + 2^-23) |ref64|."""
    for shape, C in pg.CASES[("max", 2)]:
        g = pg.make_g("zero_mean", shape, C, 2, _seed(shape, C))
        for regime in pg.X_REGIMES:
            if regime == "rounding_ties" and prec != "bf16":
                continue
            x = pg.make_x(regime, shape, C, _seed(shape, C) + 1)
            ref, bound = pg.pool_ref64(g, x, None, 2, "max", prec)
            got = pg.emulate("max", prec, g=g, x=x)
            assert float(bound.abs().max()) == 0.0 and pg.same_bits(got, ref.float()) and torch.equal(got.double(), ref), (shape, C, regime)
            # exactly one element of every window carries the gradient
            assert int((got != 0).sum()) <= g.numel()
        x = pg.make_x("post_relu", shape, C, _seed(shape, C) + 1)
        for gregime in pg.G_REGIMES:
            g, b = pg.make_g(gregime, shape, C, 2, 3), pg.make_g(gregime, shape, C, 1, 4)
            ref, bound = pg.pool_ref64(g, x, b, 2, "max", prec)
            pg.check(pg.emulate("max", prec, g=g, x=x, b=b), ref, bound, "max + b %s %s" % (shape, gregime))


def test_post_relu_windows_tie():
    """The regime the tie rule is for: at least 5 % of the windows of relu(U(-1, 1)) hold a tie (1 / 16 of them are all zero)."""
    x = pg.make_x("post_relu", (2, 3, 8, 12), 8, 5)
    assert pg.tie_share(x, "bf16x3") >= 0.05
    assert pg.tie_share(pg.make_x("rounding_ties", (2, 3, 8, 12), 8, 5), "bf16") == 1.0
    assert pg.tie_share(pg.make_x("rounding_ties", (2, 3, 8, 12), 8, 5), "bf16x3") < 0.05


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k", [2, 4, 8])
def test_avg_emulation_holds_its_bounds(k, prec):
    worst = 0.0
    for shape, C in pg.CASES[("avg", k)]:
        for gregime in pg.G_REGIMES:
            g, b = pg.make_g(gregime, shape, C, k, _seed(shape, C)), pg.make_g(gregime, shape, C, 1, _seed(shape, C) + 1)
            ref, bound = pg.pool_ref64(g, None, None, k, "avg", prec)
            got = pg.emulate("avg", prec, k=k, g=g)
            if prec != "fp16":
                assert torch.equal(got.double(), ref), (shape, C, gregime)
            pg.check(got, ref, bound, "avg %d %s" % (k, shape))
            ref, bound = pg.pool_ref64(g, None, b, k, "avg", prec)
            worst = max(worst, pg.check(pg.emulate("avg", prec, k=k, g=g, b=b), ref, bound, "avg %d + b %s" % (k, shape)))
    print("pool_grad emulation avg k=%d %s with b: err/bound %.3f" % (k, prec, worst))


@pytest.mark.parametrize("prec", PRECS)
def test_pyramid_emulation_holds_its_bound(prec):
    worst = 0.0
    for shape, C in pg.CASES[("pyramid", 8)]:
        for gregime in pg.G_REGIMES:
            g2, g4, g8, b = (pg.make_g(gregime, shape, C, k, _seed(shape, C) + k) for k in (2, 4, 8, 1))
            for bb in (None, b):
                ref, bound = pg.pool3_ref64(g2, g4, g8, bb, prec)
                worst = max(worst, pg.check(pg.emulate("pyramid", prec, g2=g2, g4=g4, g8=g8, b=bb), ref, bound, "pyramid %s" % (shape,)))
    print("pool_grad emulation pyramid %s: err/bound %.3f" % (prec, worst))


@pytest.mark.parametrize("prec", PRECS)
def test_small_integers_are_exact_throughout(prec):
    """Small-integer data is exact in every format and at every step: every form, with and without b, equals float64 autograd bit for bit."""
    for (mode, k), cases in pg.CASES.items():
        for shape, C in cases:
            b = pg.int_g(shape, C, 1, 9)
            for bb in (None, b):
                if mode == "pyramid":
                    g2, g4, g8 = (pg.int_g(shape, C, kk, 9 + kk) for kk in (2, 4, 8))
                    ref, _ = pg.pool3_ref64(g2, g4, g8, bb, prec)
                    got = pg.emulate("pyramid", prec, g2=g2, g4=g4, g8=g8, b=bb)
                else:
                    g, x = pg.int_g(shape, C, k, 9 + k), pg.make_x("plateau", shape, C, 10)
                    ref, _ = pg.pool_ref64(g, x, bb, k, mode, prec)
                    got = pg.emulate(mode, prec, k=k, g=g, x=x, b=bb)
                assert torch.equal(got.double(), ref), (mode, k, shape, C, bb is not None)


def _breaks(got, ref, bound):
    """A planted fault shows: an element fails equality where the bound is zero, or exceeds 4x the bound elsewhere."""
    err = (got.double() - ref).abs()
    return bool(((bound == 0) & (err > 0)).any()) or bool(((bound > 0) & (err > 4 * bound)).any())


@pytest.mark.parametrize("prec", PRECS)
def test_planted_faults_break_their_checks(prec):
    shape, C = (2, 3, 12, 20), 8
    g, b = pg.make_g("offset", shape, C, 2, 1), pg.make_g("offset", shape, C, 1, 2)
    # the tie rule, in the regimes that hold ties of stored values; with and without b
    for regime in ("post_relu", "plateau"):
        x = pg.make_x(regime, shape, C, 3)
        for bb in (None, b):
            ref, bound = pg.pool_ref64(g, x, bb, 2, "max", prec)
            assert not _breaks(pg.emulate("max", prec, g=g, x=x, b=bb), ref, bound)
            for fault in ("tie_last", "tie_all"):
                assert _breaks(pg.emulate("max", prec, g=g, x=x, b=bb, fault=fault), ref, bound), (regime, fault, bb is not None)
    # a tie born of the rounding: the argmax of the unrounded input is another element
    if prec == "bf16":
        x = pg.make_x("rounding_ties", shape, C, 3)
        ref, bound = pg.pool_ref64(g, x, None, 2, "max", prec)
        assert not _breaks(pg.emulate("max", prec, g=g, x=x), ref, bound)
        assert _breaks(pg.emulate("max", prec, g=g, x=x, fault="argmax_unrounded"), ref, bound)
    # the window read transposed: no tie needed
    x = pg.make_x("zero_mean", shape, C, 3)
    for bb in (None, b):
        ref, bound = pg.pool_ref64(g, x, bb, 2, "max", prec)
        assert _breaks(pg.emulate("max", prec, g=g, x=x, b=bb, fault="window_transposed"), ref, bound)
    # b dropped, in every form
    ref, bound = pg.pool_ref64(g, x, b, 2, "max", prec)
    assert _breaks(pg.emulate("max", prec, g=g, x=x, b=b, fault="b_dropped"), ref, bound)
    for gregime in pg.G_REGIMES:
        for k in (2, 4):
            gk, bk = pg.make_g(gregime, shape, C, k, 4), pg.make_g(gregime, shape, C, 1, 5)
            ref, bound = pg.pool_ref64(gk, None, bk, k, "avg", prec)
            assert _breaks(pg.emulate("avg", prec, k=k, g=gk, b=bk, fault="b_dropped"), ref, bound)
        # the pyramid: g4 and g8 with each other's scale, and b dropped
        shape8 = (2, 3, 16, 24)
        g2, g4, g8, b8 = (pg.make_g(gregime, shape8, C, k, 6 + k) for k in (2, 4, 8, 1))
        for bb in (None, b8):
            ref, bound = pg.pool3_ref64(g2, g4, g8, bb, prec)
            assert not _breaks(pg.emulate("pyramid", prec, g2=g2, g4=g4, g8=g8, b=bb), ref, bound)
            assert _breaks(pg.emulate("pyramid", prec, g2=g2, g4=g4, g8=g8, b=bb, fault="levels_swapped"), ref, bound)
        ref, bound = pg.pool3_ref64(g2, g4, g8, b8, prec)
        assert _breaks(pg.emulate("pyramid", prec, g2=g2, g4=g4, g8=g8, b=b8, fault="b_dropped"), ref, bound)


def test_refusals_without_gpu(lib_built):
    """Everything the pool backward does not serve is DFFW_EINVAL (-1) with a message, from the built library, before any launch and before the
    GPU is touched: this runs on a machine without one (dummy non-null, 16-byte-aligned addresses stand for the operands)."""
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name in ("dffw_pool_backward", "dffw_op_pool_backward"):
        getattr(lib, name).argtypes = [ci] * 4 + [vp] * 3 + [ci] * 5 + [vp] * 2
    for name in ("dffw_pool3_backward", "dffw_op_pool3_backward"):
        getattr(lib, name).argtypes = [ci, ci] + [vp] * 4 + [ci] * 5 + [vp] * 2
    P = 4096   # never dereferenced: every call below is refused first
    MAX, AVG = 0, 1

    def pool(fn, prec=0, mode=MAX, k=2, g=P, x=P, b=None, shape=(1, 8, 2, 8, 8), out=P):
        return fn(0, prec, mode, k, g, x, b, *shape, out, None)

    def pool3(fn, prec=0, g2=P, g4=P, g8=P, b=None, shape=(1, 8, 2, 8, 8), out=P):
        return fn(0, prec, g2, g4, g8, b, *shape, out, None)

    def refused(rc, what):
        assert rc == -1 and lib.dffw_last_error(), (what, rc)

    for fn in (lib.dffw_pool_backward, lib.dffw_op_pool_backward):
        for C in (0, 4, 12, 136):
            refused(pool(fn, shape=(1, C, 2, 8, 8)), "C = %d" % C)
        for bad in ((0, 8, 2, 8, 8), (1, 8, 0, 8, 8), (1, 8, 2, 0, 8), (1, 8, 2, 8, -2)):
            refused(pool(fn, shape=bad), bad)
        refused(pool(fn, shape=(1, 8, 2, 7, 8)), "H % 2")
        refused(pool(fn, mode=AVG, k=4, shape=(1, 8, 2, 8, 6)), "W % 4")
        refused(pool(fn, mode=AVG, k=8, shape=(1, 8, 2, 12, 8)), "H % 8")
        for k in (0, 1, 3, 4, 8):
            refused(pool(fn, mode=MAX, k=k), "max k = %d" % k)
        for k in (0, 1, 3, 6, 16):
            refused(pool(fn, mode=AVG, k=k, shape=(1, 8, 2, 48, 48)), "avg k = %d" % k)
        for mode in (-1, 2):
            refused(pool(fn, mode=mode), "mode %d" % mode)
        for prec in (-1, 3):
            refused(pool(fn, prec=prec), "precision %d" % prec)
        refused(pool(fn, x=None), "max without x")
        refused(pool(fn, g=None), "null g")
        refused(pool(fn, out=None), "null out")
        refused(pool(fn, shape=(32768, 8, 1, 256, 256)), "2^31 pixels")
    for fn in (lib.dffw_pool3_backward, lib.dffw_op_pool3_backward):
        for C in (0, 4, 12, 136):
            refused(pool3(fn, shape=(1, C, 2, 8, 8)), "C = %d" % C)
        for bad in ((0, 8, 2, 8, 8), (1, 8, 0, 8, 8), (1, 8, 2, 0, 8), (1, 8, 2, 8, -8)):
            refused(pool3(fn, shape=bad), bad)
        refused(pool3(fn, shape=(1, 8, 2, 12, 8)), "H % 8")
        refused(pool3(fn, shape=(1, 8, 2, 8, 20)), "W % 8")
        for prec in (-1, 3):
            refused(pool3(fn, prec=prec), "precision %d" % prec)
        for missing in ("g2", "g4", "g8", "out"):
            refused(pool3(fn, **{missing: None}), "null " + missing)
        refused(pool3(fn, shape=(32768, 8, 1, 256, 256)), "2^31 pixels")
