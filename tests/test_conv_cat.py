"""The forward conv over a virtual concatenation (dffw_op_conv3d_cat), the part that needs no GPU: the entry point's ABI and
refusals, the Python wrapper's argument errors, and what the per-element bound of oracle/error_bounds.py can see of a two-source fill gone wrong --
the op's split-bf16 arithmetic emulated on cat([xa, xb]) (emulate / split of tests/test_error_bounds.py) stays under half the bound at the
contraction depths of the network's five two-source layers, and the faults such a fill can make exceed it."""
import ctypes
import os

import pytest
import torch

from oracle import error_bounds as eb
from test_error_bounds import _conv32, emulate, fold, geo, split, store

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dffw.h")


# ---- ABI and refusals --------------------------------------------------------------------------------------------------------------------------
def test_op_conv3d_cat_abi_and_refusals_without_gpu(lib_built):
    """dffw_op_conv3d_cat is exported, declared and bound; a null tensor, a bad precision, a volume below 1, Ca or Cb below 8 or no multiple of 8,
    Ca + Cb > 192, Cout no multiple of 8 or above 128 is DFFW_EINVAL (-1) with a message before the GPU is touched (dummy addresses stand for the
    tensors)."""
    from dffinthewild_amd import engine
    header = open(HEADER).read()
    assert "int dffw_op_conv3d_cat(" in header and "dffw_op_conv3d_cat" in engine.ABI_SYMBOLS and callable(engine.op_conv3d_cat)
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dffw_op_conv3d_cat.argtypes = [ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, ci, vp, vp]
    P = 4096

    def call(prec=0, xa=P, ca=8, xb=P, cb=8, shape=(1, 2, 8, 16), w=P, cout=8, y=P):
        return lib.dffw_op_conv3d_cat(0, prec, xa, ca, xb, cb, *shape, w, cout, None, None, None, 1, y, None)

    for what, kw in (("null xa", dict(xa=None)), ("null xb", dict(xb=None)), ("null weight", dict(w=None)), ("null y", dict(y=None)),
                     ("precision 3", dict(prec=3)), ("precision -1", dict(prec=-1)),
                     ("Ca = 4", dict(ca=4)), ("Ca = 12", dict(ca=12)), ("Ca = 0", dict(ca=0)), ("Ca = -8", dict(ca=-8)),
                     ("Cb = 4", dict(cb=4)), ("Cb = 20", dict(cb=20)), ("Cb = 0", dict(cb=0)),
                     ("Ca + Cb = 200", dict(ca=128, cb=72)), ("Ca + Cb = 200, mirrored", dict(ca=72, cb=128)), ("Ca = 192", dict(ca=192, cb=8)),
                     ("Cout = 12", dict(cout=12)), ("Cout = 136", dict(cout=136)), ("Cout = 4", dict(cout=4)), ("Cout = 0", dict(cout=0)),
                     ("B = 0", dict(shape=(0, 2, 8, 16))), ("N = 0", dict(shape=(1, 0, 8, 16))), ("H = 0", dict(shape=(1, 2, 0, 16))),
                     ("W = -16", dict(shape=(1, 2, 8, -16)))):
        assert call(**kw) == -1 and lib.dffw_last_error(), what
    # a refusal names what it refuses
    assert call(ca=128, cb=72) == -1 and b"128 and 72" in lib.dffw_last_error()
    assert call(cout=136) == -1 and b"136" in lib.dffw_last_error()


def test_wrapper_refuses_cpu_tensors_and_mismatched_shapes(lib_built):
    from dffinthewild_amd import engine
    xa, xb, w = torch.zeros(1, 8, 2, 8, 16), torch.zeros(1, 16, 2, 8, 16), torch.zeros(8, 24, 3, 3, 3)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        engine.op_conv3d_cat(xa, xb, w)
    for what, args, kw in (("volumes differ", (xa, torch.zeros(1, 16, 2, 8, 8), w), {}), ("batches differ", (xa, torch.zeros(2, 16, 2, 8, 16), w), {}),
                           ("slice counts differ", (xa, torch.zeros(1, 16, 3, 8, 16), w), {}),
                           ("weight takes 16, not 8 + 16", (xa, xb, torch.zeros(8, 16, 3, 3, 3)), {}),
                           ("1x3x3 kernel", (xa, xb, torch.zeros(8, 24, 1, 3, 3)), {}), ("four dimensions", (xa[0], xb[0], w), {}),
                           ("residual of another shape", (xa, xb, w), dict(residual=torch.zeros(1, 16, 2, 8, 16)))):
        with pytest.raises(ValueError, match="op_conv3d_cat"):
            engine.op_conv3d_cat(*args, **kw)


# ---- what the bound can see on a concatenation ---------------------------------------------------------------------------------------------------
# (Ca, Cb): K = 16 * 27, 64 * 27 and 192 * 27 -- dres4.conv0, dres2.conv0 and the pyramid's combine2
DEPTHS = [(8, 8), (32, 32), (128, 64)]
COUT = 16
SHAPE = (1, 3, 16, 32)          # (B, N, H, W): two 8 x 16 columns side by side and two rows of them, a slice with both neighbours
COLUMN = (1, slice(8, 16), slice(16, 32))   # the 8 x 16 column of fault 3: slice 1, rows 8-15, columns 16-31
PREC = "bf16x3"
G = geo(1, 1)
RATIOS = {}


@pytest.fixture(scope="module", params=DEPTHS, ids=lambda p: "%d+%d" % p)
def case(request):
    ca, cb = request.param
    B, N, H, W = SHAPE
    gen = torch.Generator().manual_seed(31 + ca)
    xa = torch.rand(B, ca, N, H, W, generator=gen) * 2 - 1
    xb = torch.rand(B, cb, N, H, W, generator=gen) * 2 - 1
    w = (torch.rand(COUT, ca + cb, 3, 3, 3, generator=gen) * 2 - 1) * (2.0 / ((ca + cb) * 27)) ** 0.5 * 1.7
    bn = eb.bn_regime("plain", COUT, 32)
    r = eb.conv_ref64(torch.cat([xa, xb], 1), w, stride=1, pad=1, bn=bn, relu=0)
    return ca, cb, xa, xb, w, bn, r


def ratio(name, case, got):
    worst, _ = eb.elementwise_ratio(got, case[6], PREC)
    RATIOS[(name, case[0], case[1])] = worst
    print("conv over cat, K = %d (%d + %d), %s: err/bound %.3g" % ((case[0] + case[1]) * 27, case[0], case[1], name, worst))
    return worst


def test_clean_emulation_within_half_the_bound(case):
    ca, cb, xa, xb, w, bn, r = case
    got = emulate(torch.cat([xa, xb], 1), w, G, bn, None, 0, PREC)
    assert torch.isfinite(got).all()
    assert ratio("clean", case, got) <= 0.5


def test_fault_sources_swapped(case):
    """The fill reads xb where xa belongs and the other way round (at 128 + 64: the concatenation in the mirror order)."""
    ca, cb, xa, xb, w, bn, r = case
    assert ratio("sources swapped", case, emulate(torch.cat([xb, xa], 1), w, G, bn, None, 0, PREC)) > 1.0


def test_fault_octets_of_xb_rotated(case):
    """xb's 8-channel octets rotated by one (a piece of the fill that starts one octet on).  A tensor of one octet has no rotation: 8 + 8 is left
    out, not weakened."""
    ca, cb, xa, xb, w, bn, r = case
    if cb == 8:
        assert torch.equal(xb.roll(8, 1), xb)   # the identity: nothing to plant
        return
    assert ratio("xb's octets rotated", case, emulate(torch.cat([xa, xb.roll(8, 1)], 1), w, G, bn, None, 0, PREC)) > 1.0


def cross_dropped_ratio(case):
    """xb's cross products (hi * lo, lo * hi) dropped on one 8 x 16 column, all output channels: the second source read from hi halves only there."""
    ca, cb, xa, xb, w, bn, r = case
    x = torch.cat([xa, xb], 1)
    ws, t = fold(w, bn, False)
    xh, xl = split(x, PREC)
    wh, wl = split(ws, PREC)
    only_b = torch.zeros(1, ca + cb, 1, 1, 1)
    only_b[:, ca:] = 1.0
    cross_b = _conv32(xh * only_b, wl, G) + _conv32(xl * only_b, wh, G)
    mask = torch.zeros_like(cross_b)
    mask[(0, slice(None)) + COLUMN] = 1.0
    acc = _conv32(xh, wh, G) + _conv32(xh, wl, G) + _conv32(xl, wh, G) - cross_b * mask
    return ratio("xb's cross products dropped on one column", case, store(acc + t.reshape(1, -1, 1, 1, 1), PREC))


def test_fault_cross_products_of_xb_dropped_on_one_column(case):
    assert cross_dropped_ratio(case) > 1.0


def test_fault_one_tap_of_xb_missed_at_a_corner(case):
    """The corner pixel of a slice loses xb's channels of one filter position (1, 1, 2)."""
    ca, cb, xa, xb, w, bn, r = case
    s, _ = eb.fold_bn(bn, COUT)
    bad = emulate(torch.cat([xa, xb], 1), w, G, bn, None, 0, PREC).clone()
    tap = (xb[0, :, 1, 0, 1].double()[None, :] * w[:, ca:, 1, 1, 2].double()).sum(1) * s
    bad[0, :, 1, 0, 0] -= tap.float()
    assert ratio("one tap of xb missed at a corner", case, bad) > 1.0
