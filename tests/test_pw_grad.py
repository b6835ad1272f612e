"""CPU tests of the reference, the identities and the bounds of tests/pw_grad_ref.py (backward of the 3x1x1 / 1x1x1 convs,
gradient mask-and-add): the kernels' arithmetic, emulated with the partial lengths the kernel really uses, stays under half the bound at the
shapes of tests/test_gpu_pw_grad.py; planted faults exceed it at least 4x."""
import pytest
import torch

import pw_grad_ref as pw
from oracle import error_bounds as eb

# (B, N, H, W) of tests/test_gpu_pw_grad.py and the persistent grid each runs on there (the last one with DFFW_PWGRAD_WGS=8)
SHAPES = [((2, 3, 8, 8), None), ((1, 1, 8, 8), None), ((2, 2, 12, 20), None), ((1, 5, 16, 24), None), ((2, 10, 32, 32), 8)]


def _ratio(got, r, prec):
    return eb.elementwise_ratio(got, r, prec)[0]


def _grid(shape, cin, cout, wgs):
    B, N, H, W = shape
    return pw.grid_x_of(B, H, W, cin, cout, wgs or 512)


@pytest.mark.parametrize("geom", list(pw.GEOMETRIES))
def test_identities_match_autograd(geom):
    """grad_x is the conv of grad_y with the slice-flipped, channel-swapped filter; grad_w is the contraction wgrad_ref64 writes out."""
    for cin, cout in ((8, 16), (24, 40)):
        x, w, gy = pw.make_case("zero_mean", geom, 2, cin, cout, 3, 8, 12, 1)
        gx, gw = pw.grads64(x, w, gy, geom)
        rx, rw = pw.dgrad_ref64(w, gy, geom), pw.wgrad_ref64(x, gy, geom)
        assert rx.ref.shape == gx.shape and rw.ref.shape == gw.shape == pw.weight_shape(geom, cin, cout)
        assert float((rx.ref - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
        assert float((rw.ref - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


@pytest.mark.parametrize("geom", list(pw.GEOMETRIES))
def test_exact_emulation_matches_autograd(geom):
    """The decomposition itself (columns, ragged chunk, ring of slices, persistent ranges, per-wave blocks) on integer data, exact in every format."""
    for (shape, wgs), (cin, cout) in zip(SHAPES, ((8, 8), (16, 8), (24, 40), (8, 16), (16, 16))):
        B, N, H, W = shape
        x, w, gy = pw.int_case(geom, B, cin, cout, N, H, W, 3)
        ref = pw.grads64(x, w, gy, geom)[1]
        for prec in pw.PRECISIONS:
            for grid_x, flush in ((_grid(shape, cin, cout, wgs), pw.FLUSH_STEPS), (8, 1)):
                got = pw.emulate_pw_wgrad(x, gy, geom, prec, grid_x=grid_x, flush_steps=flush)
                assert torch.equal(got.double(), ref), (shape, prec, grid_x, flush)


@pytest.mark.parametrize("prec", pw.PRECISIONS)
@pytest.mark.parametrize("geom", list(pw.GEOMETRIES))
@pytest.mark.parametrize("regime", ["zero_mean", "post_relu", "offset"])
def test_wgrad_bound_holds_at_the_gpu_shapes(regime, geom, prec):
    worst = 0.0
    for shape, wgs in SHAPES:
        B, N, H, W = shape
        x, w, gy = pw.make_case(regime, geom, B, 16, 16, N, H, W, 5)
        got = pw.emulate_pw_wgrad(x, gy, geom, prec, grid_x=_grid(shape, 16, 16, wgs))
        worst = max(worst, _ratio(got, pw.wgrad_ref64(x, gy, geom), prec))
    print("pw wgrad emulation %s %s %s: err/bound %.3f" % (geom, prec, regime, worst))
    assert worst <= 0.5, (geom, prec, regime, worst)


def test_wgrad_emulation_at_ragged_channel_counts():
    for geom in pw.GEOMETRIES:
        for cin, cout in ((24, 40), (40, 24)):
            x, w, gy = pw.make_case("zero_mean", geom, 2, cin, cout, 2, 12, 20, 5)
            r = pw.wgrad_ref64(x, gy, geom)
            for prec in pw.PRECISIONS:
                assert _ratio(pw.emulate_pw_wgrad(x, gy, geom, prec, grid_x=8, flush_steps=2), r, prec) <= 0.5


# the volume of tests/test_gpu_pw_grad.py::test_full_length_partials: 8 -> 8 channels, 640 steps per workgroup of a grid of 8
FULL = (1, 10, 256, 256)


def test_full_volume_has_full_length_partials():
    B, N, H, W = FULL
    steps = pw.steps_per_workgroup(B, N, H, W, 8)
    assert B * N * H * W <= 2 ** 20 and len(steps) == 8 and min(steps) > pw.FLUSH_STEPS, steps


@pytest.mark.parametrize("geom", list(pw.GEOMETRIES))
def test_wgrad_bound_holds_at_full_length_partials(geom):
    """Split-bf16 with offset inputs (the regime that grew in section 13) on FULL with 8 workgroups: every wave sums a whole 16 384-pixel
    partial in fp32, flushes it and starts a second."""
    B, N, H, W = FULL
    x, w, gy = pw.make_case("offset", geom, B, 8, 8, N, H, W, 41)
    worst = _ratio(pw.emulate_pw_wgrad(x, gy, geom, "bf16x3", grid_x=8), pw.wgrad_ref64(x, gy, geom), "bf16x3")
    print("pw wgrad emulation full-length partials %s bf16x3 offset %s: err/bound %.3f" % (geom, FULL, worst))
    assert worst <= 0.5


# (fault, geometry, (B, cin, cout, N, H, W), precisions).  The contractions are short (a lost lo half is an error of random sign of about
# 2^-9.5 sqrt(K / 2) |x gy| against 2^-16 K |x gy|: K = 240 pixels keeps it 4x over), the faults that move whole products show in every precision
ALL = pw.PRECISIONS
FAULTS = [
    ("taps_reversed", "k311", (2, 8, 8, 3, 8, 8), ALL),
    ("next_sample", "k311", (2, 8, 8, 2, 8, 8), ALL),
    ("ragged_runs_on", "k311", (2, 8, 8, 2, 12, 12), ALL),     # 144 pixels: 112 foreign ones in the ragged chunk, so that bf16's bound notices too
    ("ragged_runs_on", "k111", (2, 8, 8, 2, 12, 12), ALL),
    ("hi_only", "k111", (1, 8, 8, 1, 12, 20), ("bf16x3",)),
    ("hi_only", "k311", (1, 8, 8, 1, 12, 20), ("bf16x3",)),
    ("missing_wave", "k311", (1, 8, 8, 2, 8, 16), ALL),        # one column: the missing wave held a quarter of every contraction
    ("missing_wave", "k111", (1, 8, 8, 2, 8, 16), ALL),
    ("swapped_octets", "k311", (2, 24, 40, 2, 12, 20), ALL),
    ("swapped_octets", "k111", (2, 40, 24, 2, 12, 20), ALL),
    ("swapped_octets", "k111", (2, 104, 56, 2, 12, 20), ALL),
]


@pytest.mark.parametrize("fault,geom,shape,precs", FAULTS)
def test_planted_faults_exceed_the_bound(fault, geom, shape, precs):
    B, cin, cout, N, H, W = shape
    x, w, gy = pw.make_case("zero_mean", geom, B, cin, cout, N, H, W, 7)
    r = pw.wgrad_ref64(x, gy, geom)
    for prec in precs:
        clean = _ratio(pw.emulate_pw_wgrad(x, gy, geom, prec), r, prec)
        worst = _ratio(pw.emulate_pw_wgrad(x, gy, geom, prec, fault=fault), r, prec)
        assert clean <= 0.5 and worst >= 4.0, (fault, geom, prec, clean, worst)


def _combine_case(C=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    shape = (2, C, 3, 12, 20)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g)


@pytest.mark.parametrize("prec", pw.PRECISIONS)
def test_grad_combine_emulation(prec):
    a, y, b = _combine_case()
    # mask only: exact, the record of a or +0
    ref, bound = pw.combine_ref64(a, y, None, prec)
    got = pw.emulate_combine(a, y, None, prec)
    assert float(bound.max()) == 0.0 and torch.equal(got.double(), ref)
    assert torch.equal(got[pw.rounded(y, prec) > 0], pw.rounded(a, prec)[pw.rounded(y, prec) > 0])
    # with b, masked or not: one fp32 rounding and one split
    for yy in (y, None):
        ref, bound = pw.combine_ref64(a, yy, b, prec)
        err = (pw.emulate_combine(a, yy, b, prec).double() - ref).abs()
        assert bool((err <= bound).all()), float(eb._ratio(err, bound).max())
    # the planted faults: the mask taken from a instead of y, the add dropped
    ref, bound = pw.combine_ref64(a, y, b, prec)
    for fault in ("mask_from_a", "add_dropped"):
        err = (pw.emulate_combine(a, y, b, prec, fault=fault).double() - ref).abs()
        assert float(eb._ratio(err, bound).max()) >= 4.0, fault
    ref, _ = pw.combine_ref64(a, y, None, prec)
    assert not torch.equal(pw.emulate_combine(a, y, None, prec, fault="mask_from_a").double(), ref)
