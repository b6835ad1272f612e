"""CPU: the reference, bound and emulation of the alpha heads' back half (tests/head_tail_ref.py) -- the reference against a literal float64
composition, the clean emulation of every form at a quarter of the bound over every case of tests/test_gpu_head_tail.py, every planted fault
at more than four times the bound on a named case, what the whole-network gate would have seen of each fault, the unresolved-ReLU shares of
the GPU test's inputs, and the refusals of dffw_op_head_tail against the built library (no GPU)."""
import ctypes
import math

import pytest
import torch

import head_tail_ref as ht
from oracle import error_bounds as eb

PRECS = ht.PRECISIONS


def all_cases():
    """(name, start, forms, builder) of every case of the GPU test."""
    for i, s in enumerate(ht.PAIR_SHAPES):
        for kind in ("random", "placed"):
            yield "pair %s %s" % (s, kind), 0, ht.FORMS, (lambda i=i, kind=kind: ht.pair_case(i, kind))
    for j, c in enumerate(ht.ROWS_CASES):
        for kind in ("random", "placed"):
            yield "rows %s %s" % (c, kind), 0, ("rows", "planes", "mean"), (lambda j=j, kind=kind: ht.rows_case(j, kind))
    for j, c in enumerate(ht.STORED_CASES):
        yield "stored %s" % (c,), 0, ("planes", "mean"), (lambda j=j: ht.stored_case(j))
    for C in (16, 32, 64):
        for shape in ht.S2_SHAPES:
            for kind in ht.S2_KINDS:
                yield "s2 C%d %s %s" % (C, shape, kind), 2, ("planes", "mean"), (lambda C=C, shape=shape, kind=kind: ht.s2_case(C, shape, kind))


@pytest.mark.parametrize("prec", PRECS)
def test_reference_matches_a_literal_composition(prec):
    for x, p, a, start in [ht.pair_case(3) + (0,), ht.pair_case(2, "placed") + (0,), ht.s2_case(32, (1, 2, 3, 37), "random") + (2,),
                           ht.s2_case(64, (2, 3, 2, 2), "constant") + (2,), ht.s2_case(16, (1, 1, 1, 1), "zero") + (2,)]:
        r = ht.reference(x, *p, a, prec, start, "planes")
        m, al = ht.literal(x, *p, a, prec, start)
        assert torch.allclose(r.raw, m, rtol=1e-12, atol=1e-14) and torch.allclose(r.alpha, al, rtol=1e-12, atol=1e-14)
        assert r.raw.shape == (x.shape[0], 3, x.shape[2])


def test_calibration():
    """The clean emulation over every case, form and arithmetic: the worst err / E without the safety factor is CAL_WORST (the module's
    constant holds it to two digits), CAL_FACTOR is four times that rounded up to a power of two, and with it the emulation sits at E / 4."""
    worst, where = 0.0, None
    for name, start, forms, build in all_cases():
        x, p, a = build()
        for prec in PRECS:
            r = ht.reference(x, *p, a, prec, start, forms, factor=1.0)
            y2 = {}
            for form in forms:
                stored = form in ("planes", "mean")
                if start == 0 and stored not in y2:
                    y2[stored] = ht.emulate_y2(x, *p[:4], prec, stored)
                got = ht.emulate(x, *p, a, prec, start, form, y2=y2.get(stored))
                w = ht.worst(*got, r, form)
                if w > worst:
                    worst, where = w, (name, prec, form)
    print("clean emulation: worst err / E = %.3f at %s" % (worst, where))
    assert worst <= ht.CAL_WORST, (worst, where)
    assert worst >= 0.8 * ht.CAL_WORST, "CAL_WORST is stale: the worst ratio is now %.3f" % worst
    assert ht.CAL_FACTOR == 2.0 ** math.ceil(math.log2(4 * ht.CAL_WORST))
    assert worst / ht.CAL_FACTOR <= 0.25


# fault -> the case on which it is held to 4 E: (builder, start, forms, arithmetics)
S2_PLACED = (lambda: ht.s2_case(16, (2, 3, 12, 20), "placed"), 2, ("planes", "mean"), PRECS)
S2_CHUNKS = (lambda: ht.s2_case(16, (1, 1, 40, 52), "random"), 2, ("planes",), PRECS)           # nine chunks of 232, the last of 224
S0_PLACED = (lambda: ht.pair_case(3, "placed"), 0, ("tiles", "rows"), ("bf16x3",))               # 3 x 3 tiles, impulses through centre taps
FAULT_CASES = {
    "corner_missing": (S2_PLACED, S0_PLACED), "corners_swapped": (S2_PLACED, S0_PLACED), "row_swapped": (S2_PLACED, S0_PLACED),
    "col_swapped": (S2_PLACED, S0_PLACED), "remainder_dropped": (S2_CHUNKS,), "lo_dropped": (S2_CHUNKS,), "interior_as_left": (S0_PLACED,),
    "divisor": (S2_PLACED, S0_PLACED), "damp_c1": (S2_PLACED, S0_PLACED), "raw_damped": (S2_PLACED, S0_PLACED),
    "alpha_overwritten": (S2_PLACED, S0_PLACED), "idx_order": (S2_PLACED, S0_PLACED),
}


@pytest.mark.parametrize("fault", ht.FAULTS)
def test_every_planted_fault_exceeds_four_times_the_bound(fault):
    """Each fault, in every form and arithmetic of its named cases in which it can act, is over 4 E on at least one output number, and the
    clean emulation of the same case is under E / 4.  (Through start = 0 the 16-bit arithmetics' carried term is as large as a border line's
    share of the mean: there the border faults are held by the start = 2 cases, whose carried term is zero.)"""
    acted = 0
    for build, start, forms, precs in FAULT_CASES[fault]:
        x, p, a = build()
        B, C, N, H, W = x.shape
        for prec in precs:
            r = ht.reference(x, *p, a, prec, start, forms)
            for form in forms:
                if not ht.can_act(fault, form, prec, B, N, H, W, C):
                    continue
                assert ht.worst(*ht.emulate(x, *p, a, prec, start, form), r, form) <= 0.25
                w = ht.worst(*ht.emulate(x, *p, a, prec, start, form, fault=fault), r, form)
                assert w > 4.0, (fault, prec, form, w)
                acted += 1
    assert acted, fault


def test_old_gate_table():
    """What the whole-network gate (relative L2 of 2e-5 over a sample's tap) would have seen of each fault on a smooth 64 x 96 input: the
    single-pixel faults sit at the gate (a corner is one pixel in 6144: DESIGN lists them under it at 256 x 256), a last chunk's remainder does
    not exist at sizes that are multiples of 32, and the faults of the last steps are far over it."""
    t = ht.old_gate_table(64, 96)
    assert set(t) == set(ht.FAULTS)
    assert t["remainder_dropped"] == (None, 0.0)
    for f in ("corner_missing", "corners_swapped", "lo_dropped"):
        assert t[f][1] < 4 * ht.GATE, (f, t[f])
    for f in ("damp_c1", "raw_damped", "alpha_overwritten", "idx_order", "divisor"):
        assert t[f][1] > 100 * ht.GATE, (f, t[f])


@pytest.mark.parametrize("prec", PRECS)
def test_unresolved_relu_shares(prec):
    """Where a ReLU's reference input lies within the bound of zero the kernel's ReLU may differ from the reference's and the whole scale
    passes (no output is left out).  From the reference alone: the share of such elements stays under ALPHA * 2^9 for every start = 0 input of
    the GPU test -- 2^9 being about the largest scale-to-value ratio two stacked 3 x 3 convs reach at He scale (oracle/error_bounds.py: "some
    600 |y|"), and a ReLU input spread over its own scale has at most that share of its mass within +- ALPHA * D of zero.  For bf16 the product
    is over 1: no cap, every ReLU may pass its scale, which is what the bound assumes anyway."""
    cap = ht.SHARE_CAP[prec]
    assert cap == min(1.0, eb.ALPHA[prec] * 2.0 ** 9)
    cases = [ht.pair_case(i, k) for i in range(len(ht.PAIR_SHAPES)) for k in ("random", "placed")]
    cases += [ht.rows_case(j, k) for j in range(len(ht.ROWS_CASES)) for k in ("random", "placed")]
    cases += [ht.stored_case(j) for j in range(len(ht.STORED_CASES))]
    for x, p, a in cases:
        r = ht.reference(x, *p, a, prec, 0, "planes")
        assert len(r.shares) == 2 and max(r.shares) <= cap, (tuple(x.shape), r.shares)


def test_refusals_without_gpu(lib_built):
    """Everything dffw_op_head_tail does not serve is DFFW_EINVAL (-1) with a message, from the built library, before any GPU call: this runs
    on a machine without one (dummy non-null addresses stand for the operands)."""
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dffw_op_head_tail.argtypes = [ci, ci, vp] + [ci] * 5 + [vp] * 6 + [ci] + [vp] * 3
    P = 4096   # never dereferenced: every call below is refused first
    names = ("x", "w2", "bn2", "w4", "bn4", "w6", "bias6", "alpha", "raw")

    def call(prec=0, shape=(1, 16, 2, 8, 16), start=0, **null):
        ptr = {n: (None if n in null else P) for n in names}
        return lib.dffw_op_head_tail(0, prec, ptr["x"], *shape, ptr["w2"], ptr["bn2"], ptr["w4"], ptr["bn4"], ptr["w6"], ptr["bias6"], start,
                                     ptr["alpha"], ptr["raw"], None)

    def refused(rc, what):
        assert rc == -1 and lib.dffw_last_error(), (what, rc)

    for n in names:
        refused(call(**{n: None}), "null " + n)
    for prec in (-1, 3):
        refused(call(prec=prec), "precision %d" % prec)
    for C in (0, 8, 24, 48, 128):
        refused(call(shape=(1, C, 2, 8, 16)), "C = %d" % C)
    for start in (-1, 1, 3, 4, 6):
        refused(call(start=start), "start = %d" % start)
    for bad in ((0, 16, 2, 8, 16), (1, 16, 0, 8, 16), (1, 16, 2, 0, 16), (1, 16, 2, 8, 0), (1, 16, 2, -8, 16)):
        refused(call(shape=bad), bad)
    refused(call(shape=(2185, 16, 10, 8, 16)), "B * N * 3 = 65550")
    refused(call(shape=(1 << 20, 16, 1 << 11, 1, 1), start=2), "B * N * 3 past 2^31")
