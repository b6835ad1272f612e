"""CPU: the reference, bound and emulation of the alpha heads' front half and of fov_warp_kernel (tests/head_front_ref.py) -- the float64 warp
against the goldens made by the reference's own FOV_warp, the reference against a literal composition (torch's grid_sample), the clean
emulation of every form at a quarter of the bound over every case of tests/test_gpu_head_front.py, every planted fault at more than four
times the bound on a named case, what the whole-network gate would have seen of each fault, and the refusals of dffw_op_head_front against
the built library (no GPU)."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

import head_front_ref as hf
import head_tail_ref as ht
from oracle.make_goldens_e2e import case_inputs

PRECS = hf.PRECISIONS
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "e2e_fov_warp_*.npz")))


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_float64_warp_matches_the_reference_goldens(path):
    """The restatement in float64 (positions, flow, bilinear sample with zeros outside, no blend across slices) against what the reference's
    FOV_warp gave in float32: within 1e-5 absolutely, and within the bound of fov_warp_kernel (torch's float32 is one more float32 evaluation)."""
    g = np.load(path)
    x, alpha, fov = (torch.from_numpy(t) for t in case_inputs(int(g["C"]), int(g["N"]), int(g["H"]), int(g["W"]), int(g["seed"])))
    r = hf.fov_reference(x, alpha, fov)
    out, flow = torch.from_numpy(g["out"]), torch.from_numpy(g["flow"])
    assert r.out.shape == out.shape and r.flow.shape == flow.shape
    assert float((r.flow - flow).abs().max()) <= 1e-5 and float((r.out - out).abs().max()) <= 1e-5
    assert float(hf.ratio(out, r.out, r.E_out).max()) <= 1.0 and float(hf.ratio(flow, r.flow, r.E_flow).max()) <= 1.0


def test_goldens_present():
    assert len(GOLDEN) == 3


@pytest.mark.parametrize("prec", PRECS)
def test_reference_matches_a_literal_composition(prec):
    for i, j in ((2, 3), (2, 2), (6, 4), (15, 6), (0, 0), (14, 5)):
        fe, p, alpha, fov, name = hf.case(i, j)
        r = hf.reference(fe, *p, alpha, fov, prec)
        lit = hf.literal(fe, *p, alpha, fov, prec)
        assert r.ref.shape == (fe.shape[0], 2 * fe.shape[1]) + tuple(fe.shape[2:])
        assert torch.allclose(r.ref, lit, rtol=1e-10, atol=1e-11), (name, float((r.ref - lit).abs().max()))


def test_position_error_count():
    """ds and dflow against the float32 arithmetic of warp_point itself, contracted or not: W from 16 to 640, f within 1 +- 0.6, shifts up to
    1.5 W.  The plain rounding count is an upper bound (the emulation stays under it, and uses a good part of it)."""
    worst = 0.0
    g = torch.Generator().manual_seed(7)
    for W in (16, 17, 48, 96, 255, 640):
        B, N = 4, 8
        f = 1.0 + 0.6 * (torch.rand(B, N, generator=g) * 2 - 1)
        fov = 0.9 + 0.2 * torch.rand(B, N, generator=g)
        shift = 1.5 * W * (torch.rand(B, N, generator=g) * 2 - 1)
        alpha = torch.stack([f - fov, shift, torch.zeros(B, N)], 1).float()
        geo = hf.Geometry(alpha, fov, 4, W)
        for contract in (False, True):
            fx, sx = hf._axis32(alpha[:, 0] + fov.float(), alpha[:, 1], W, contract)
            worst = max(worst, float(((sx.double().unsqueeze(2) - geo.sx).abs() / geo.dsx).max()), float(((fx.double().unsqueeze(2) - geo.fx).abs() / geo.dfx).max()))
    print("float32 positions and flow: worst err / count %.3f" % worst)
    assert 0.1 <= worst <= 1.0, worst


def all_cases():
    for i in range(len(hf.SHAPES)):
        for j in range(len(hf.WARPS)):
            yield i, j


def test_calibration():
    """The clean emulation over every case, form, arithmetic and contraction variant: the worst err / E without the safety factor is CAL_WORST
    (the module's constant holds it to two digits), CAL_FACTOR is four times that rounded up to a power of two, and with it the emulation sits
    at E / 4.  (The warp form's arithmetic is the split form's: one emulation serves both.)"""
    worst, where = 0.0, None
    for i, j in all_cases():
        C, (B, N, H, W), _ = hf.SHAPES[i]
        fe, p, alpha, fov, name = hf.case(i, j)
        for prec in PRECS:
            r = hf.reference(fe, *p, alpha, fov, prec, factor=1.0)
            for contract in (False, True):
                vol = hf.emulate_volume(fe, alpha, fov, prec, contract)
                for form in ("split", "whole"):
                    w = float(hf.ratio(hf.emulate(fe, *p, alpha, fov, prec, form, contract, vol=vol), r.ref, r.E).max())
                    if w > worst:
                        worst, where = w, (name, prec, form, contract)
    print("clean emulation: worst err / E = %.3f at %s" % (worst, where))
    assert worst <= hf.CAL_WORST, (worst, where)
    assert worst >= 0.8 * hf.CAL_WORST, "CAL_WORST is stale: the worst ratio is now %.3f" % worst
    assert hf.CAL_FACTOR == 2.0 ** math.ceil(math.log2(4 * hf.CAL_WORST))
    assert worst / hf.CAL_FACTOR <= 0.25


def test_fov_calibration():
    """The same for fov_warp_kernel's bound: out and flow, every case of the GPU test, both contraction variants."""
    worst, where = 0.0, None
    for i in range(len(hf.FOV_SHAPES)):
        for j in range(len(hf.WARPS)):
            x, alpha, fov, compat, name = hf.fov_case(i, j)
            r = hf.fov_reference(x, alpha, fov, compat, factor=1.0)
            for contract in (False, True):
                out, flow = hf.fov_emulate(x, alpha, fov, compat, contract)
                w = max(float(hf.ratio(out, r.out, r.E_out).max()), float(hf.ratio(flow, r.flow, r.E_flow).max()))
                if w > worst:
                    worst, where = w, (name, contract)
    print("clean fov_warp emulation: worst err / E = %.3f at %s" % (worst, where))
    assert worst <= hf.FOV_CAL_WORST, (worst, where)
    assert worst >= 0.8 * hf.FOV_CAL_WORST, "FOV_CAL_WORST is stale: the worst ratio is now %.3f" % worst
    assert hf.FOV_CAL_FACTOR == 2.0 ** math.ceil(math.log2(4 * hf.FOV_CAL_WORST))
    assert worst / hf.FOV_CAL_FACTOR <= 0.25


# The named cases: 3 x 3 columns of 8 x 16, two samples, three slices, the mixed warp regime (f within 1 +- 0.3 on either side of 1, shifts of
# either sign up to 3 pixels, all distinct per sample and slice: positions between W - 1 and W at the right border, footprints outside the
# image on every side) on planes each filled with its own constant (Lx = Ly = 0 inside: E there is the conv's own bound), 8 and 16 channels.
FAULT_CASES = ((2, 6), (9, 6))


@pytest.mark.parametrize("fault", hf.FAULTS)
def test_every_planted_fault_exceeds_four_times_the_bound(fault):
    """Each fault, in every form and arithmetic of the named cases in which it can act, is over 4 E on at least one output element, and the
    clean emulation of the same case is under E / 4."""
    acted = 0
    for i, j in FAULT_CASES:
        C, (B, N, H, W), _ = hf.SHAPES[i]
        fe, p, alpha, fov, name = hf.case(i, j)
        assert name.endswith("mixed/constant"), name
        for prec in PRECS:
            r = hf.reference(fe, *p, alpha, fov, prec)
            for form in hf.forms_of(C, B, N, H, W):
                if not hf.can_act(fault, form, prec, B, N):
                    continue
                assert float(hf.ratio(hf.emulate(fe, *p, alpha, fov, prec, form), r.ref, r.E).max()) <= 0.25
                w = float(hf.ratio(hf.emulate(fe, *p, alpha, fov, prec, form, fault=fault), r.ref, r.E).max())
                assert w > 4.0, (fault, name, prec, form, w)
                acted += 1
    assert acted >= (2 if fault == "lo_dropped" else 6), (fault, acted)


GATE = 2e-6   # test_hip_e2e_head_warp_streaming_kernel: relative L2 over the 30 numbers of a head / alpha tap, split-bf16


def old_gate_table(H, W, prec="bf16x3", C=8, N=10, B=2):
    """fault -> the larger of the raw and alpha taps' relative L2 against the clean emulation, the faulty y0 of the warp form carried through
    the head's tail (head_tail_ref.emulate, tiles form) on smooth features of two samples: what the whole-network gate, which compares these
    3 N numbers per sample, would have seen of each planted fault."""
    fe = hf.features("smooth", (B, C, N, H, W), 1)
    alpha, fov = hf.warp_params("mixed", B, N, H, W, 2)
    w0, bn0 = hf.front_params("post_relu", C, 3)
    tail = ht.head_params("post_relu", 2 * C, seed=11)
    a_in = alpha.clone()
    taps = lambda y0: ht.emulate(y0, *tail, a_in, prec, 0, "tiles")
    clean = taps(hf.emulate(fe, w0, bn0, alpha, fov, prec, "warp"))
    out = {}
    for fault in hf.FAULTS:
        bad = taps(hf.emulate(fe, w0, bn0, alpha, fov, prec, "warp", fault=fault))
        out[fault] = max(ht.gate_rel_l2(bad[0], clean[0]), ht.gate_rel_l2(bad[1], clean[1]))
    return out


def test_old_gate_table():
    """At 32 x 32, the smallest image of the whole-network test: which planted faults its 2e-6 gate on the taps sees (DESIGN §24 lists 256 x 256
    beside it).  The faults that change whole planes are far over the gate; what the table says of the single-pixel faults is recorded, not
    assumed: this test only pins that the table is complete and that a whole-plane fault is seen."""
    t = old_gate_table(32, 32)
    print({k: "%.2e" % v for k, v in t.items()})
    assert set(t) == set(hf.FAULTS)
    for f in ("ref_slice0", "flow_swapped", "alpha0_ref", "ref_neighbour_sample"):
        assert t[f] > 10 * GATE, (f, t[f])


def test_refusals_without_gpu(lib_built):
    """Everything dffw_op_head_front does not serve is DFFW_EINVAL (-1) with a message, from the built library, before any GPU call: this runs
    on a machine without one (dummy non-null addresses stand for the operands)."""
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dffw_op_head_front.argtypes = [ci, ci, vp] + [ci] * 5 + [vp] * 6
    P = 4096   # never dereferenced: every call below is refused first
    names = ("fe", "w0", "bn0", "alpha", "fov", "y0")

    def call(prec=0, shape=(1, 8, 2, 8, 16), **null):
        ptr = {n: (None if n in null else P) for n in names}
        return lib.dffw_op_head_front(0, prec, ptr["fe"], *shape, ptr["w0"], ptr["bn0"], ptr["alpha"], ptr["fov"], ptr["y0"], None)

    def refused(rc, what):
        assert rc == -1 and lib.dffw_last_error(), (what, rc)

    for n in names:
        refused(call(**{n: None}), "null " + n)
    for prec in (-1, 3):
        refused(call(prec=prec), "precision %d" % prec)
    for C in (0, 4, 12, 24, 64):
        refused(call(shape=(1, C, 2, 8, 16)), "C = %d" % C)
    for bad in ((0, 8, 2, 8, 16), (1, 8, 0, 8, 16), (1, 8, 2, 0, 16), (1, 8, 2, 8, 0), (1, 8, 2, -8, 16)):
        refused(call(shape=bad), bad)
