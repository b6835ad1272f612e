"""Backward of a conv over a channel concatenation, the part that needs no GPU: the refusals of the two record-form symbols
in their order, the workspace sizes, the CPU emulation of dffw::conv_wgrad_cat_kernel (cg.emulate_wgrad behind the restated two-source fill)
against the bound, the planted faults of the fill against the same bound, and the Python layer's argument errors."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cat_grad_ref as cc  # noqa: E402
import conv_grad_ref as cg  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402

PAIRS = [(8, 8), (24, 40), (128, 64), (64, 128)]   # the switch inside a 16-wide tile at both parities of its octet, on a 32-group boundary, past 128
COUT = 16
SHAPE = (2, 3, 12, 20)      # (B, N, H, W): both slice paddings, ragged tile edges, B > 1
FAULT_SHAPE = (1, 2, 6, 20)
I3 = ctypes.c_int * 3
K333 = (I3(3, 3, 3), I3(1, 1, 1), I3(1, 1, 1), 0)


@pytest.fixture(scope="module")
def lib(lib_built):
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    lib.dffw_conv_cat_wgrad_workspace_bytes.restype = ctypes.c_int64
    lib.dffw_conv_cat_wgrad_workspace_bytes.argtypes = [ctypes.c_int] * 7
    lib.dffw_conv_wgrad_workspace_bytes.restype = ctypes.c_int64
    lib.dffw_conv_wgrad_workspace_bytes.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.c_int]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dffw_conv_cat_wgrad.argtypes = [ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, ctypes.c_int64, vp]
    return lib


def test_the_symbols_are_exported_and_declared(lib):
    from dffinthewild_amd import engine
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dffw.h")).read()
    for name in ("dffw_conv_cat_wgrad_workspace_bytes", "dffw_conv_cat_wgrad", "dffw_op_conv_cat_backward"):
        assert hasattr(lib, name) and name in engine.ABI_SYMBOLS and name + "(" in header, name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def wgrad(lib, prec=0, xa=0x1000, ca=128, xb=0x2000, cb=64, B=2, N=3, H=12, W=20, gy=0x3000, cout=128, gw=0x4000, ws=0x5000, wsb=0):
    """dffw_conv_cat_wgrad with pointers that are no device memory: every call here must be refused before one is read.  -> (rc, message)"""
    rc = lib.dffw_conv_cat_wgrad(0, prec, xa, ca, xb, cb, B, N, H, W, gy, cout, gw, ws, wsb, None)
    return rc, lib.dffw_last_error().decode()


def test_refusals_in_the_familys_order(lib):
    """Shape (precision, volume, Cout, the unit limit, then this entry point's own rule for Ca and Cb), null, alignment, workspace: each refusal
    is reached only when everything before it is in order, so a call wrong in two ways names the earlier one."""
    bad = dict(prec=3), dict(B=0), dict(cout=136), dict(B=2 ** 15, N=2 ** 15, H=8, W=16), dict(ca=136), dict(xa=0), dict(xb=0x2008), dict()
    words = ("precision", "shape", "136", "31 bits", "Ca=136 Cb=64", "null", "16-byte", "workspace too small")
    codes = (-1,) * 7 + (-3,)
    for i, (kw, word, code) in enumerate(zip(bad, words, codes)):
        rc, msg = wgrad(lib, **kw)
        assert rc == code and word in msg, (kw, rc, msg)
        for later in bad[i + 1:-1]:     # ... and with any later fault added, still this one
            rc2, msg2 = wgrad(lib, **{**later, **kw})
            assert rc2 == code and word in msg2, (kw, later, rc2, msg2)
    # the rule of the two sources names both, whichever breaks it
    for ca, cb in ((0, 64), (8, 4), (64, 136), (128, 72), (120, 80), (12, 8), (-8, 8)):
        rc, msg = wgrad(lib, ca=ca, cb=cb)
        assert rc == -1 and "Ca=%d Cb=%d" % (ca, cb) in msg, (ca, cb, msg)
    for name, kw in (("xa", dict(xa=0)), ("xb", dict(xb=0)), ("grad_y", dict(gy=0)), ("grad_w", dict(gw=0)), ("workspace", dict(ws=0))):
        assert wgrad(lib, **kw) == (-1, "null argument"), name
    for name, kw in (("xa", dict(xa=0x1008)), ("xb", dict(xb=0x2004)), ("grad_y", dict(gy=0x3002)), ("workspace", dict(ws=0x5004))):
        rc, msg = wgrad(lib, **kw)
        assert rc == -1 and "aligned" in msg, (name, msg)
    need = lib.dffw_conv_cat_wgrad_workspace_bytes(2, 128, 64, 3, 12, 20, 128)
    rc, msg = wgrad(lib, wsb=need - 1)
    assert rc == -3 and str(need) in msg and str(need - 1) in msg, msg
    # every served pair of channel counts passes the shape's refusals: with no workspace the call ends at the last one
    for ca in range(8, 129, 8):
        for cb in range(8, min(128, 192 - ca) + 1, 8):
            assert wgrad(lib, ca=ca, cb=cb)[0] == -3, (ca, cb)


def test_workspace_bytes(lib):
    """The plain conv's size on the concatenation wherever that one is served (every sum up to 128), 0 for refused arguments, positive at 128 + 64."""
    B, N, H, W = SHAPE
    for cout in (8, 24, 128):
        for ca in range(8, 121, 8):
            for cb in range(8, 128 - ca + 1, 8):
                plain = lib.dffw_conv_wgrad_workspace_bytes(B, ca + cb, N, H, W, cout, *K333)
                assert plain > 0 and lib.dffw_conv_cat_wgrad_workspace_bytes(B, ca, cb, N, H, W, cout) == plain, (ca, cb, cout)
    assert lib.dffw_conv_cat_wgrad_workspace_bytes(B, 128, 64, N, H, W, 128) > 0
    assert lib.dffw_conv_wgrad_workspace_bytes(B, 192, N, H, W, 128, *K333) == 0      # (the plain entry point still refuses 192)
    for args in ((B, 128, 72, N, H, W, 128), (B, 136, 8, N, H, W, 8), (B, 8, 0, N, H, W, 8), (B, 8, 8, N, H, W, 136), (0, 8, 8, N, H, W, 8),
                 (B, 8, 8, N, H, 0, 8), (B, 12, 8, N, H, W, 8), (2 ** 15, 8, 8, 2 ** 15, 8, 16, 8)):
        assert lib.dffw_conv_cat_wgrad_workspace_bytes(*args) == 0, args


# ---- emulation -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d+%d" % p)
def test_emulation_stays_under_half_the_bound(pair, prec):
    xa, xb, w, gy, _, _, rw = cc.case("zero_mean", pair[0], pair[1], COUT, SHAPE)
    worst, _ = eb.elementwise_ratio(cc.emulate_cat_wgrad(xa, xb, gy, prec), rw, prec)
    print("emulated grad_w %d+%d -> %d %s %s: err/bound %.3f" % (pair + (COUT, SHAPE, prec, worst)))
    assert worst <= 0.5


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d+%d" % p)
def test_emulation_is_autograd_bit_for_bit_on_integers(pair):
    """Small integers are exact in every record format and every sum here is exact in fp32: the emulation must equal autograd in all three."""
    g = torch.Generator().manual_seed(5 + pair[0])
    B, N, H, W = FAULT_SHAPE
    xa, xb = (torch.randint(-3, 4, (B, c, N, H, W), generator=g).float() for c in pair)
    gy = torch.randint(-2, 3, (B, COUT, N, H, W), generator=g).float()
    w = torch.zeros(COUT, sum(pair), 3, 3, 3, requires_grad=True)
    want = torch.autograd.grad(F.conv3d(torch.cat([xa, xb], 1), w, None, 1, 1), w, gy)[0]
    assert float(want.abs().max()) > 0
    for prec in cg.PRECISIONS:
        assert torch.equal(cc.emulate_cat_wgrad(xa, xb, gy, prec), want), prec


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d+%d" % p)
@pytest.mark.parametrize("fault", cc.FAULTS)
def test_planted_faults_exceed_the_bound(fault, pair):
    """Each fault of the two-source fill puts at least one element of grad_w at 4 times its bound or more, in every precision: the bound the GPU
    test holds the kernel to would catch it.  One combination cannot: with Ca == Cb the two row pitches are one number, reading b with a's pitch
    is no fault there, and the fill must then read the unfaulted records."""
    xa, xb, w, gy, _, _, rw = cc.case("zero_mean", pair[0], pair[1], COUT, FAULT_SHAPE)
    for prec in cg.PRECISIONS:
        if fault == "b_pitch" and pair[0] == pair[1]:
            ra, rb = cg.to_records(xa, prec), cg.to_records(xb, prec)
            assert torch.equal(cc.cat_fill(ra, rb, fault), cc.cat_fill(ra, rb))
            continue
        got = cc.emulate_cat_wgrad(xa, xb, gy, prec, fault=fault)
        worst, _ = eb.elementwise_ratio(got, rw, prec)
        print("fault %s %d+%d %s: err/bound %.1f" % (fault, pair[0], pair[1], prec, worst))
        assert worst >= 4.0, (fault, pair, prec, worst)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors(lib_built):
    from dffinthewild_amd import engine, pipeline
    z = torch.zeros
    xa, xb, w, gy = z(1, 8, 2, 4, 4), z(1, 16, 2, 4, 4), z(8, 24, 3, 3, 3), z(1, 8, 2, 4, 4)
    wrong = (
        (dict(xb=z(1, 16, 2, 4, 5)), "differ outside the channel axis"),
        (dict(xb=z(2, 16, 2, 4, 4)), "differ outside the channel axis"),
        (dict(w=z(8, 16, 3, 3, 3)), "does not take 8 \\+ 16 input channels"),
        (dict(w=z(8, 24, 1, 3, 3)), "3x3x3 stride 1 pad 1"),
        (dict(xa=z(8, 2, 4, 4)), "5 dimensions"),
    )
    for kw, match in wrong:
        a = {**dict(xa=xa, xb=xb, w=w, gy=gy), **kw}
        with pytest.raises(ValueError, match=match):
            engine.op_conv_cat_backward(a["xa"], a["xb"], a["w"], a["gy"])
        with pytest.raises(ValueError, match=match):
            pipeline.conv3d_cat(a["xa"], a["xb"], a["w"])
    with pytest.raises(ValueError, match="not the conv's output shape"):
        engine.op_conv_cat_backward(xa, xb, w, z(1, 8, 2, 4, 5))
    with pytest.raises(ValueError, match="need"):
        engine.op_conv_cat_backward(xa, xb, w, gy, need=("x",))
    with pytest.raises(engine.DffwError, match="no CPU fallback"):
        engine.op_conv_cat_backward(xa, xb, w, gy)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipeline.conv3d_cat(xa, xb, w)
