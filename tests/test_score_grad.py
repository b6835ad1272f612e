"""Backward of the score convs, Cin -> 1, without a GPU: the two formulas against float64 autograd; the CPU emulation of
the kernels' arithmetic (tests/score_grad_ref.py) inside the derived bounds at every shape of the GPU test, exact on integer data, and breaking
the bounds by the project's factor 4 under each planted fault; the refusals of the built library, before the GPU is touched.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 19 is where they go."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_grad_ref as sg  # noqa: E402

FACTOR = 4.0   # what a planted fault must exceed its bound by


@pytest.mark.parametrize("geom", sorted(sg.GEOMETRIES))
def test_formulas_equal_autograd(geom):
    """dgrad_of / wgrad_of in float64 against float64 autograd of F.conv3d, to 1e-12 of the largest element."""
    for shape, C in ((sg.SHAPES[geom][2], 8), (sg.SHAPES[geom][3], 24)):
        x, w, g, _ = sg.make_case(geom, shape, C, 3)
        gx, gw = sg.grads64(x, w, g, geom)
        mine_x, mine_w = sg.dgrad_of(w.double(), g.double(), None, geom), sg.wgrad_of(x.double(), g.double(), geom)
        assert float((mine_x - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
        assert float((mine_w - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


@pytest.mark.parametrize("prec", sg.PRECISIONS)
@pytest.mark.parametrize("geom", sorted(sg.GEOMETRIES))
def test_emulation_inside_the_bounds(geom, prec):
    """The clean emulation at every (shape, C, grid) of tests/test_gpu_score_grad.py: the bounds are rigorous, so its worst err / bound is <= 1."""
    worst = {"x": 0.0, "x + b": 0.0, "w": 0.0}
    for shape in sg.SHAPES[geom]:
        for C in sg.CHANNELS[geom]:
            x, w, g, b = sg.make_case(geom, shape, C, 11 + C + sum(shape), aligned_b=(geom == "k111" and prec == "fp16"))
            for bb, key in ((None, "x"), (b, "x + b")):
                ref, bound = sg.dgrad_ref64(w, g, bb, geom, prec)
                worst[key] = max(worst[key], sg.check(sg.emulate_dgrad(w, g, bb, geom, prec), ref, bound, "grad_x %s %s C=%d" % (geom, shape, C)))
            for wgs in sg.grids_of(geom, shape):
                ref, bound = sg.wgrad_ref64(x, g, geom, prec, sg.wgrad_chain(geom, shape, C, wgs))
                worst["w"] = max(worst["w"], sg.check(sg.emulate_wgrad(x, g, geom, prec, wgs=wgs), ref, bound,
                                                      "grad_w %s %s C=%d wgs=%d" % (geom, shape, C, wgs)))
    print("score_grad emulation %s %s: err/bound " % (geom, prec) + " ".join("%s %.3f" % kv for kv in worst.items()))


@pytest.mark.parametrize("geom", sorted(sg.GEOMETRIES))
def test_integer_data_is_exact(geom):
    """Integer data: every product and every sum is exact, so the emulation equals float64 autograd bit for bit, on both grids."""
    shape, C = sg.SHAPES[geom][-1], 24 if geom == "k111" else 40
    x, w, g, b = sg.int_case(geom, shape, C, 5)
    gx, gw = sg.grads64(x, w, g, geom)
    for prec in sg.PRECISIONS:
        assert torch.equal(sg.emulate_dgrad(w, g, b, geom, prec).double(), gx + b.double()), prec
        assert torch.equal(sg.emulate_dgrad(w, g, None, geom, prec).double(), gx), prec
        for wgs in (sg.DEFAULT_WGS, sg.SMALL_WGS):
            assert sg.same_bits(sg.emulate_wgrad(x, g, geom, prec, wgs=wgs), gw.float()) and torch.equal(gw.float().double(), gw), (prec, wgs)


def test_fma32_is_correctly_rounded():
    """The emulation's fmaf against exact rational arithmetic, on cases whose float64 sum is a tie of the fp32 grid (the double rounding it avoids)."""
    from fractions import Fraction
    import numpy as np
    a = np.array([1 + 2.0 ** -23, 3.0, 1.0, -1.5], dtype=np.float32)
    b = np.array([1 + 2.0 ** -23, 2.0 ** -25, 2.0 ** -24, 2.0 ** -24], dtype=np.float32)
    c = np.array([2.0 ** -24 + 2.0 ** -60, 1.0, 1.0 + 2.0 ** -23, 1.0], dtype=np.float32)
    got = sg.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    gen = np.random.default_rng(0)
    a, b, c = (gen.standard_normal(4096).astype(np.float32) for _ in range(3))
    got = sg.fma32(a, b, c)
    for i in range(0, 4096, 64):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert abs(Fraction(float(got[i])) - exact) <= abs(exact) * Fraction(1, 2 ** 24), i


def _breaks(got, ref, bound):
    return sg.worst_ratio(got, ref, bound) >= FACTOR


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_planted_faults_k111(prec):
    """Each fault exceeds its bound by the factor 4; the clean emulation of the same case does not exceed it at all."""
    shape, C = (1, 2, 23, 23), 24        # three octets; two units and a ragged third
    x, w, g, b = sg.make_case("k111", shape, C, 17, aligned_b=(prec == "fp16"))
    L = sg.wgrad_chain("k111", shape, C)
    wref, wbound = sg.wgrad_ref64(x, g, "k111", prec, L)
    assert not sg.worst_ratio(sg.emulate_wgrad(x, g, "k111", prec), wref, wbound) > 1
    for fault in ("octets_swapped", "g_neighbour", "ragged_dropped", "slot_missing") + (("hi_only",) if prec == "bf16x3" else ()):
        assert _breaks(sg.emulate_wgrad(x, g, "k111", prec, fault=fault), wref, wbound), fault
    for bb in (None, b):
        ref, bound = sg.dgrad_ref64(w, g, bb, "k111", prec)
        assert not sg.worst_ratio(sg.emulate_dgrad(w, g, bb, "k111", prec), ref, bound) > 1
        for fault in ("octets_swapped", "g_neighbour", "ragged_dropped"):
            assert _breaks(sg.emulate_dgrad(w, g, bb, "k111", prec, fault=fault), ref, bound), fault


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_planted_faults_k333(prec):
    shape, C = (2, 3, 9, 11), 8          # two samples, ragged tiles in both directions
    x, w, g, b = sg.make_case("k333", shape, C, 19)
    L = sg.wgrad_chain("k333", shape, C)
    wref, wbound = sg.wgrad_ref64(x, g, "k333", prec, L)
    assert not sg.worst_ratio(sg.emulate_wgrad(x, g, "k333", prec), wref, wbound) > 1
    for fault in ("next_sample", "row_wrap", "kykx_swapped", "ragged_summed"):
        assert _breaks(sg.emulate_wgrad(x, g, "k333", prec, fault=fault), wref, wbound), fault
    for bb in (None, b):
        ref, bound = sg.dgrad_ref64(w, g, bb, "k333", prec)
        assert not sg.worst_ratio(sg.emulate_dgrad(w, g, bb, "k333", prec), ref, bound) > 1
        for fault in ("not_flipped", "next_sample", "row_wrap"):
            assert _breaks(sg.emulate_dgrad(w, g, bb, "k333", prec, fault=fault), ref, bound), fault


def test_refusals_without_gpu(lib_built):
    """Everything the score conv backward does not serve is DFFW_EINVAL (-1) with a message, and a short workspace DFFW_ENOMEM (-3), from the
    built library, before any launch and before the GPU is touched: this runs on a machine without one (dummy non-null, 16-byte-aligned
    addresses stand for the operands)."""
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci, i3 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    lib.dffw_score_conv_dgrad.argtypes = [ci, ci, vp] + [ci] * 5 + [vp, i3, i3] + [vp] * 3
    lib.dffw_score_conv_wgrad_workspace_bytes.argtypes = [ci] * 5 + [i3, i3]
    lib.dffw_score_conv_wgrad_workspace_bytes.restype = ctypes.c_int64
    lib.dffw_score_conv_wgrad.argtypes = [ci, ci, vp, vp] + [ci] * 5 + [i3, i3, vp, vp, ctypes.c_int64, vp]
    lib.dffw_op_score_conv_backward.argtypes = [ci, ci, vp] + [ci] * 5 + [vp, i3, i3] + [vp] * 5
    P = 4096   # never dereferenced: every call below is refused first
    v3 = lambda v: (ctypes.c_int * 3)(*v)
    K1, K3 = ((1, 1, 1), (0, 0, 0)), ((3, 3, 3), (1, 1, 1))

    def dgrad(prec=0, g=P, shape=(1, 8, 2, 8, 8), w=P, geom=K1, b=None, out=P):
        return lib.dffw_score_conv_dgrad(0, prec, g, *shape, w, v3(geom[0]), v3(geom[1]), b, out, None)

    def wgrad(prec=0, x=P, g=P, shape=(1, 8, 2, 8, 8), geom=K1, gw=P, ws=P, wsb=1 << 40):
        return lib.dffw_score_conv_wgrad(0, prec, x, g, *shape, v3(geom[0]), v3(geom[1]), gw, ws, wsb, None)

    def op(prec=0, x=P, shape=(1, 8, 2, 8, 8), w=P, geom=K1, g=P, b=None, gx=P, gw=P):
        return lib.dffw_op_score_conv_backward(0, prec, x, *shape, w, v3(geom[0]), v3(geom[1]), g, b, gx, gw, None)

    def bytes_of(shape=(1, 8, 2, 8, 8), geom=K1):
        return lib.dffw_score_conv_wgrad_workspace_bytes(*shape, v3(geom[0]), v3(geom[1]))

    def refused(rc, what):
        assert rc == -1 and lib.dffw_last_error(), (what, rc)

    bad_geoms = [((1, 3, 3), (0, 1, 1)), ((3, 1, 1), (1, 0, 0)), ((3, 3, 3), (0, 0, 0)), ((1, 1, 1), (1, 1, 1)), ((3, 3, 3), (1, 1, 0)),
                 ((5, 5, 5), (2, 2, 2)), ((3, 3, 1), (1, 1, 0)), ((0, 0, 0), (0, 0, 0))]
    bad_shapes = [(0, 8, 2, 8, 8), (1, 8, 0, 8, 8), (1, 8, 2, 0, 8), (1, 8, 2, 8, -2), (32768, 8, 1, 256, 256)]
    for fn in (dgrad, wgrad, op):
        for geom in bad_geoms:
            refused(fn(geom=geom), geom)
        for C in (0, 4, 12, 136, -8):
            refused(fn(shape=(1, C, 2, 8, 8)), "C = %d" % C)
        for shape in bad_shapes:
            refused(fn(shape=shape), shape)
        for prec in (-1, 3):
            refused(fn(prec=prec), "precision %d" % prec)
        refused(fn(g=None), "null grad_score")
    for geom in bad_geoms:
        assert bytes_of(geom=geom) == 0, geom
    for shape in bad_shapes + [(1, 4, 2, 8, 8), (1, 136, 2, 8, 8)]:
        assert bytes_of(shape=shape) == 0, shape
    # null and misaligned operands of the record forms
    refused(dgrad(w=None), "null weight")
    refused(dgrad(out=None), "null out")
    refused(dgrad(out=P + 8), "out misaligned")
    refused(dgrad(b=P + 8), "b misaligned")
    refused(dgrad(g=P + 2), "grad_score misaligned")
    refused(wgrad(x=None), "null x")
    refused(wgrad(gw=None), "null grad_w")
    refused(wgrad(ws=None), "null workspace")
    refused(wgrad(x=P + 8), "x misaligned")
    refused(wgrad(ws=P + 4), "workspace misaligned")
    # ... of the op form: b without grad_x, grad_x without a weight, grad_w without x; and a call with no output is only its refusals
    refused(op(b=P, gx=None), "b without grad_x")
    refused(op(w=None), "grad_x without weight")
    refused(op(x=None), "grad_w without x")
    assert op(gx=None, gw=None) == 0
    # the workspace: grid * Cin * taps float64, nothing that scales with the pixel count beyond the grid
    for geom, taps in ((K1, 1), (K3, 27)):
        for shape, C in (((1, 8, 2, 8, 8), 8), ((2, 40, 3, 16, 24), 40), ((8, 8, 10, 256, 256), 8), ((32, 32, 10, 32, 32), 32)):
            B, _, N, H, W = shape
            name = "k111" if taps == 1 else "k333"
            want = sg.grid_of(name, (B, N, H, W)) * C * taps * 8
            assert bytes_of(shape=shape, geom=geom) == want, (shape, geom)
            rc = wgrad(shape=shape, geom=geom, wsb=want - 1)
            assert rc == -3 and lib.dffw_last_error(), (shape, geom, rc)
    assert bytes_of(shape=(8, 8, 10, 256, 256)) == 512 * 8 * 8
