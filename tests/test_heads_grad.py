"""The bound of the regression heads' backward under any upstream gradient on the CPU: the calibration of ALPHA re-measured, the
kernel's formulation in float32 inside ALPHA * G, every planted fault outside it, N = 1 exactly zero.  tests/heads_grad_ref.py holds the
reference, the bound and the cases; tests/test_gpu_heads_grad.py holds the kernels to the same bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_grad_ref as R  # noqa: E402

ALL = [(s["id"], k) for s in R.SPECS for k in R.KINDS]


def test_case_list():
    """loss_ref's cases and the 8x8 stack whose 1/8 head is one element, each under the four gradient kinds"""
    assert [s["id"] for s in R.SPECS[:-1]] == [s["id"] for s in R.L.CASES]
    last = R.SPECS[-1]
    assert (last["N"], last["H"], last["W"]) == (3, 8, 8)
    case, gps, ref, G = R.evaluated(last["id"], "dense")
    assert tuple(case["scores"][0].shape[-2:]) == (1, 1) and len(ALL) == 4 * len(R.SPECS)
    case, gps, _, _ = R.evaluated("n10_b3_dense", "pixel")
    B, H, W = gps[0].shape
    assert int((gps[0] != 0).sum()) == 1 and gps[0][B - 1, H // 3, W - 1] != 0
    frac = float((R.evaluated("n10_b3_dense", "sparse")[1][0] != 0).float().mean())
    assert 0.07 < frac < 0.13


def test_calibration():
    """float32 CPU autograd against float64 over the whole list: at or below the recorded figure, and ALPHA follows from it by the rule"""
    worst, where = 0.0, None
    for cid, kind in ALL:
        case, gps, ref, G = R.evaluated(cid, kind)
        r = R.worst_ratio(R.reference(case, gps, torch.float32), ref, G)
        if max(r) > worst:
            worst, where = max(r), (cid, kind, r.index(max(r)))
    print("float32 autograd: worst err/G %.2f * 2^-24 at %s; ALPHA = %g * 2^-24" % (worst / R.EPS32, where, R.ALPHA / R.EPS32))
    assert worst <= R.CAL_GRAD
    assert R.ALPHA == R.alpha_rule(R.CAL_GRAD)


@pytest.mark.parametrize("cid", [s["id"] for s in R.SPECS])
def test_manual_within_bound(cid):
    for kind in R.KINDS:
        case, gps, ref, G = R.evaluated(cid, kind)
        r = R.worst_ratio(R.manual_grads(case, gps), ref, G)
        assert max(r) <= R.ALPHA, (cid, kind, [x / R.EPS32 for x in r])


@pytest.mark.parametrize("fault", R.FAULTS)
def test_fault_exceeds_bound(fault):
    worst = 0.0
    for spec in R.SPECS:
        if spec["N"] == 1:
            continue
        case, gps, ref, G = R.evaluated(spec["id"], "dense")
        worst = max(worst, max(R.worst_ratio(R.manual_grads(case, gps, fault=fault), ref, G)))
    print(fault, "worst err/G = %.3g * ALPHA" % (worst / R.ALPHA))
    assert worst > R.ALPHA


def test_one_slice_is_zero():
    for kind in R.KINDS:
        case, gps, ref, G = R.evaluated("n1_32x32", kind)
        assert all(float(g.abs().max()) == 0 for g in R.manual_grads(case, gps))
        assert max(R.worst_ratio([torch.zeros_like(g) for g in ref], ref, G)) <= R.ALPHA   # ... and exact zeros are within the bound of the reference
