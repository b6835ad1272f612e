"""CPU tests of the conv backward's reference, identities and bound (tests/conv_grad_ref.py): the kernel's arithmetic,
emulated with the partial length the kernel really uses, stays under half the bound; planted faults exceed it at least 4x."""
import pytest
import torch

import conv_grad_ref as cg
from oracle import error_bounds as eb


def _ratio(got, r, prec):
    return eb.elementwise_ratio(got, r, prec)[0]


@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_dgrad_identities_match_autograd(geom):
    """grad_x is a conv of grad_y: flipped, channel-swapped filter at stride 1; the transposed form / the stride-2 conv on the same filter."""
    x, w, gy = cg.make_case("zero_mean", geom, 2, 8, 16, 3, 8, 12, 1)
    gx, _ = cg.grads64(x, w, gy, geom)
    r = cg.dgrad_ref64(w, gy, geom)
    assert r.ref.shape == gx.shape
    assert float((r.ref - gx).abs().max()) <= 1e-12 * float(gx.abs().max())


@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_wgrad_exact_emulation_matches_autograd(geom):
    """The decomposition itself (units, slice taps, persistent ranges, role swap of the transposed form) in an arithmetic without rounding
    error to speak of: integer data, exact in every format."""
    g = torch.Generator().manual_seed(3)
    B, cin, cout, N, H, W = 2, 8, 16, 3, 12, 20
    x = torch.randint(-3, 4, (B, cin, N, H, W), generator=g).float()
    gy = torch.randint(-3, 4, cg.out_shape(geom, B, cin, cout, N, H, W), generator=g).float()
    ref = cg.wgrad_ref64(x, gy, geom, cg.weight_shape(geom, cin, cout)).ref
    for prec in cg.PRECISIONS:
        for grid_x, flush in ((8, cg.FLUSH_UNITS), (16, 1)):
            got = cg.emulate_wgrad(x, gy, geom, prec, grid_x=grid_x, flush_units=flush)
            assert torch.equal(got.double(), ref), (prec, grid_x, flush)


# the longest partial the kernel sums in fp32: one workgroup (of the 8 of the smallest grid) over PARTIAL_PIXELS pixels, K = 8 * 16 384 in all
LONG = dict(B=2, cin=8, cout=8, N=4, H=128, W=128)


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("regime", ["zero_mean", "post_relu", "offset"])
def test_wgrad_bound_holds_at_the_longest_partial(prec, regime):
    x, w, gy = cg.make_case(regime, "k133", seed=11, **LONG)
    assert x.shape[0] * x.shape[2] * x.shape[3] * x.shape[4] == 8 * cg.PARTIAL_PIXELS
    r = cg.wgrad_ref64(x, gy, "k133", tuple(w.shape))
    worst = _ratio(cg.emulate_wgrad(x, gy, "k133", prec, grid_x=8), r, prec)
    print("wgrad emulation %s %s K=%d: err/bound %.3f" % (prec, regime, 8 * cg.PARTIAL_PIXELS, worst))
    assert worst <= 0.5


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
@pytest.mark.parametrize("regime", ["zero_mean", "post_relu", "offset", "impulse", "one_sample"])
def test_wgrad_bound_holds(prec, geom, regime):
    x, w, gy = cg.make_case(regime, geom, 2, 16, 8, 3, 16, 24, 5)
    r = cg.wgrad_ref64(x, gy, geom, tuple(w.shape))
    worst = _ratio(cg.emulate_wgrad(x, gy, geom, prec, grid_x=8, flush_units=4), r, prec)
    assert worst <= 0.5, (prec, geom, regime, worst)


# (fault, geometry, shape): contractions of at most 16 384 pixels (above that one missed product of average size G / K is under 4x the split-bf16
# bound); "hi_only" drops the lo halves of the footprint tensor in every other unit, an error of random sign of about 2^-9.5 sqrt(K / 2) |x gy| against
# 2^-16 K |x gy|: K is kept at 256 pixels so that it stands 4x over the bound
FAULTS = [
    ("drop_product", "k333", (1, 8, 8, 4, 64, 64)),
    ("drop_product", "k333s2", (1, 8, 8, 4, 128, 128)),
    ("hi_only", "k133", (1, 8, 8, 1, 8, 32)),
    ("z_neighbour", "k333", (1, 8, 8, 2, 8, 16)),
    ("odd_pixel", "k333s2", (1, 8, 8, 2, 16, 32)),
    ("odd_pixel", "k333t", (1, 8, 8, 2, 8, 16)),
    ("missing_partial", "k333", (2, 8, 8, 3, 12, 20)),
    ("no_swap", "k333t", (1, 8, 8, 2, 8, 16)),
]


@pytest.mark.parametrize("fault,geom,shape", FAULTS)
def test_planted_faults_exceed_the_bound(fault, geom, shape):
    B, cin, cout, N, H, W = shape
    x, w, gy = cg.make_case("zero_mean", geom, B, cin, cout, N, H, W, 7)
    r = cg.wgrad_ref64(x, gy, geom, tuple(w.shape))
    for prec in (("bf16x3",) if fault in ("hi_only", "drop_product") else cg.PRECISIONS):
        if fault == "no_swap":   # the roles not swapped: the stride-2 conv's gradient of (gy, x) -- another shape altogether where H differs, so compare the square case's values
            got = cg.emulate_wgrad(gy[:, :, :, ::2, ::2].contiguous(), torch.nn.functional.interpolate(x, scale_factor=(1, 2, 2)), geom, prec, fault=None)
            got = got.transpose(0, 1).contiguous()
        else:
            got = cg.emulate_wgrad(x, gy, geom, prec, fault=fault)
        clean = _ratio(cg.emulate_wgrad(x, gy, geom, prec), r, prec)
        worst = _ratio(got, r, prec)
        assert clean <= 0.5 and worst >= 4.0, (fault, prec, clean, worst)
