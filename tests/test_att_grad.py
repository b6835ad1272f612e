"""The fused backward of the attention tail without a GPU: the five formulas against float64 autograd; the bounds of
tests/att_grad_ref.py calibrated on a CPU emulation of the kernel's arithmetic at the GPU tests' shapes; integer data bit for bit; every planted
fault over its bound by the project's factor; the C ABI's refusals."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import att_grad_ref as ag  # noqa: E402
import pw_grad_ref as pw  # noqa: E402

FAULT_FACTOR = 4.0


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def stored(x, w3, w1, prec):
    """a and t as the forward stores them: record values."""
    _, a, t = ag.forward64(pw.rounded(x, prec).double(), w3.double(), w1.double())
    return pw.rounded(a.float(), prec), pw.rounded(t.float(), prec)


def test_identities_match_autograd():
    B, C, N, H, W = 2, 8, 3, 5, 7
    g = torch.Generator().manual_seed(1)
    # x positive and w3's first row positive: a[0] is open everywhere, so no pixel has all of a closed and pre_t exactly 0
    x = (torch.randn(B, C, N, H, W, generator=g, dtype=torch.float64).abs() + 0.1).requires_grad_(True)
    w3 = torch.randn(C, C, 3, 1, 1, generator=g, dtype=torch.float64) * 0.3
    w3[0] = w3[0].abs()
    w3.requires_grad_(True)
    w1 = (torch.randn(C, C, 1, 1, 1, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    gy = torch.randn(B, C, N, H, W, generator=g, dtype=torch.float64)
    pre_a = F.conv3d(x, w3, padding=(1, 0, 0))
    pre_t = F.conv3d(F.relu(pre_a), w1)
    assert float(pre_a.detach().abs().min()) > 1e-6 and float(pre_t.detach().abs().min()) > 1e-6     # no pre-activation at a ReLU's kink
    assert 0 < int((pre_a > 0).sum()) < pre_a.numel() and 0 < int((pre_t > 0).sum()) < pre_t.numel()
    y = x + F.relu(pre_t)
    want = torch.autograd.grad(y, (x, w3, w1), gy)
    _, a, t = ag.forward64(x.detach(), w3.detach(), w1.detach())
    got = ag.formulas64(x.detach(), a, t, gy, w3.detach(), w1.detach())[:3]
    for gv, wv in zip(got, want):
        assert gv.shape == wv.shape and float((gv - wv).abs().max()) <= 1e-12 * float(wv.abs().max())


@functools.lru_cache(maxsize=None)
def emulated(regime, C, shape, prec):
    B, N, H, W = shape
    x, w3, w1, gy = ag.make_case(regime, B, C, N, H, W, seed=23 + C + sum(shape))
    a, t = stored(x, w3, w1, prec)
    r = ag.ref64(x, a, t, gy, w3, w1, prec)
    return (x, a, t, gy, w3, w1), r, ag.ratios(ag.emulate(x, a, t, gy, w3, w1, prec, grid_x=ag.grid_x_of(B, H, W, wgs=8)), r)


@pytest.mark.parametrize("prec", ag.PRECISIONS)
@pytest.mark.parametrize("C", [8, 16, 32])
def test_emulation_stays_under_the_bounds(C, prec):
    worst = [0.0, 0.0, 0.0]
    for regime in ("zero_mean",) + (("post_relu", "offset") if C == 16 else ()):
        for shape in ag.SHAPES:
            _, r, rs = emulated(regime, C, shape, prec)
            assert 0 < int(r.mask_a.sum()) < r.mask_a.numel() and 0 < int(r.mask_t.sum()) < r.mask_t.numel()
            assert max(rs) <= 1.0, (regime, shape, rs)
            worst = [max(p, q) for p, q in zip(worst, rs)]
    print("att_grad emulation %s C=%d: worst err/bound grad_x %.3f grad_w3 %.3f grad_w1 %.3f" % (prec, C, *worst))


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 2, 12, 20)])
@pytest.mark.parametrize("C", [8, 16])
def test_integer_data_is_exact(C, shape):
    B, N, H, W = shape
    x, w3, w1, gy = ag.int_case(B, C, N, H, W, seed=3 + C)
    _, a, t = ag.forward64(x.double(), w3.double(), w1.double())
    ref = ag.formulas64(x.double(), a, t, gy.double(), w3.double(), w1.double())
    for v in (a, t, ref[3], ref[4], ref[0]):
        assert ag.exact_in_record(v, "bf16x3")
    assert 0 < int((a > 0).sum()) < a.numel() and 0 < int((t > 0).sum()) < t.numel()
    for grid_x, flush in ((8, ag.FLUSH_STEPS), (ag.grid_x_of(B, H, W), 2)):
        got = ag.emulate(x, a.float(), t.float(), gy, w3, w1, "bf16x3", grid_x=grid_x, flush_steps=flush)
        for gv, rv in zip(got, ref[:3]):
            assert torch.equal(gv.double(), rv)


@pytest.mark.parametrize("prec", ag.PRECISIONS)
@pytest.mark.parametrize("fault", ag.FAULTS)
def test_planted_faults_exceed_the_bounds(fault, prec):
    """(2, 2, 12, 20): two samples, one slice neighbour, a full and a ragged chunk per plane."""
    C, shape = 16, (2, 2, 12, 20)
    args, r, clean = emulated("zero_mean", C, shape, prec)
    assert max(clean) <= 1.0
    rs = ag.ratios(ag.emulate(*args, prec, grid_x=8, fault=fault), r)
    assert max(rs) >= FAULT_FACTOR, (fault, prec, rs)


def test_abi_refusals_without_gpu(eng):
    lib = eng.lib
    for sym in ("dffw_att_tail_backward_workspace_bytes", "dffw_att_tail_backward", "dffw_op_att_tail_backward"):
        assert hasattr(lib, sym) and sym in eng.ABI_SYMBOLS
    wsb = lib.dffw_att_tail_backward_workspace_bytes
    for C in (8, 16, 32):
        assert wsb(2, C, 3, 12, 20) == 8 * ag.grid_x_of(2, 12, 20) * 4 * C * C
    one = torch.zeros(64, dtype=torch.float32)     # host memory: a refused call never reads it
    p = one.data_ptr()
    for B, C, N, H, W in ((1, 0, 2, 8, 8), (1, 24, 2, 8, 8), (1, 40, 2, 8, 8), (1, 8, 0, 8, 8), (0, 8, 2, 8, 8), (1, 8, 2, 0, 8), (1, 8, 2, 8, -1)):
        assert wsb(B, C, N, H, W) == 0
        assert lib.dffw_att_tail_backward(0, 0, p, p, p, p, B, C, N, H, W, p, p, p, p, p, p, 1 << 20, None) == -1     # DFFW_EINVAL
        assert lib.dffw_op_att_tail_backward(0, 0, p, p, p, p, B, C, N, H, W, eng._f32(one), eng._f32(one), p, p, p, None) == -1
        assert lib.dffw_last_error() != b""
    assert wsb(1 << 20, 8, 1, 1 << 10, 1 << 10) == 0                                                                 # 2^33 units
    assert lib.dffw_att_tail_backward(0, 7, p, p, p, p, 1, 8, 2, 8, 8, p, p, p, p, p, p, 1 << 20, None) == -1           # an unknown precision
    assert lib.dffw_att_tail_backward(0, 0, p, p, p, p, 1, 8, 2, 8, 8, p, p, p, p, None, p, 1 << 20, None) == -1        # one weight gradient without the other
    assert lib.dffw_att_tail_backward(0, 0, p, p, p, p, 1, 8, 2, 8, 8, p, p, None, None, None, None, 0, None) == 0      # no output: nothing to launch
