"""Training loss and regression-head backward, CPU side: tests/loss_ref.py against the goldens recorded from the
reference's own training step (tools/make_goldens_loss.py), the calibration of its gates, and fault injection into the kernel's
formulation to show that the per-element bound has teeth."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as L  # noqa: E402

GOLDENS = ("plain", "ranged", "ranged_conf")


@pytest.fixture(scope="module")
def evaluated():
    """case, float64 reference, float32 reference and bound of every case of the GPU list: computed once, never modified"""
    out = {}
    for spec in L.CASES:
        case = L.make_case(spec)
        out[spec["id"]] = (spec, case, L.reference(case), L.reference(case, torch.float32), L.bound(case))
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_reproduces_goldens(name):
    """The goldens are float32 results of the reference: their distance to the float64 restatement is that of a float32 run, so the
    gates are the calibrated ones (ALPHA * G per gradient element, LOSS_RTOL on the losses), predictions at float32 resolution."""
    case, want = L.load_golden(name)
    ref = L.reference(case)
    ratios = L.worst_ratio(want["grads"], ref["grads"], L.bound(case))
    print(name, "golden grads err/G in 2^-24:", ["%.2f" % (x / L.EPS32) for x in ratios])
    assert max(ratios) <= L.ALPHA
    got = torch.cat([ref["per_head"], ref["total"].reshape(1)])
    assert torch.all((want["losses"].double() - got).abs() <= L.LOSS_RTOL * got.abs())
    for a, b in zip(want["preds"], ref["preds"]):
        assert torch.allclose(a.double(), b, rtol=1e-5, atol=0)
    assert float(torch.cat([s.abs().reshape(-1) for s in case["scores"]]).max()) > 20   # the threshold branch is in the goldens


def test_calibration(evaluated):
    """ALPHA and LOSS_RTOL are 4x the float32 CPU autograd's own worst figures over the GPU case list, rounded up to a power of two."""
    worst_g = worst_l = 0.0
    for spec, case, r64, r32, G in evaluated.values():
        worst_g = max(worst_g, max(L.worst_ratio(r32["grads"], r64["grads"], G)))
        if spec["mask"] != "empty":
            worst_l = max(worst_l, float(((r32["per_head"].double() - r64["per_head"]) / r64["per_head"]).abs().max()))
    print("float32 autograd: worst err/G %.2f * 2^-24, worst loss error %.2e" % (worst_g / L.EPS32, worst_l))
    assert worst_g <= L.CAL_GRAD * 1.25 and worst_l <= L.CAL_LOSS * 1.25      # the recorded figures still describe this torch build
    assert 4 * L.CAL_GRAD <= L.ALPHA < 8 * L.CAL_GRAD
    assert 4 * L.CAL_LOSS <= L.LOSS_RTOL < 8 * L.CAL_LOSS


def test_manual_formulation_is_clean(evaluated):
    for spec, case, r64, r32, G in evaluated.values():
        assert max(L.worst_ratio(L.manual_grads(case), r64["grads"], G)) <= L.ALPHA, spec["id"]


# fault -> the cases in which it can show (no_threshold needs exp to overflow, z_no_conf a conf, mask_mul a NaN outside the mask)
FAULTS = {
    "no_clamp": ("n2_b3_ranged_nan", "n10_b3_dense", "n11_underflow"),
    "missed_pixel": ("n2_b3_ranged_nan", "n10_b3_dense", "n17_dense"),
    "no_threshold": ("n11_underflow", "n17_dense"),
    "mask_mul": ("n2_b3_ranged_nan", "n10_b3_dense", "mask_single"),
    "z_no_conf": ("n5_conf_dense", "n16_conf", "mask_full_b3"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_bound_catches_fault(evaluated, fault):
    for cid in FAULTS[fault]:
        spec, case, r64, r32, G = evaluated[cid]
        ratio = max(L.worst_ratio(L.manual_grads(case, fault=fault), r64["grads"], G))
        print(fault, cid, "err / (ALPHA G) = %.3g" % (ratio / L.ALPHA))
        assert ratio >= 4 * L.ALPHA, (fault, cid)


def test_empty_mask_and_single_slice(evaluated):
    spec, case, r64, r32, G = evaluated["mask_empty"]
    assert torch.isnan(r64["total"]) and torch.isnan(r64["per_head"]).all()
    assert all(float(g.abs().max()) == 0 for g in r64["grads"]) and all(float(g.abs().max()) == 0 for g in L.manual_grads(case))
    spec, case, r64, r32, G = evaluated["n1_32x32"]
    assert all(float(g.abs().max()) == 0 for g in L.manual_grads(case))             # one slice: d is f, exactly no gradient
    assert all(float(g.abs().max()) <= 1e-12 for g in r64["grads"])                 # autograd: zero up to float64 rounding
    assert torch.isfinite(r64["total"])
