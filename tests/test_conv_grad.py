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
    for cin, cout in ((8, 16), (24, 40)):
        x, w, gy = cg.make_case("zero_mean", geom, 2, cin, cout, 3, 8, 12, 1)
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


@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_wgrad_emulation_at_ragged_channel_counts(geom):
    """24 -> 40 channels: the reference, the bound helpers and the emulation at counts that are no power of two.  Integer data: bit for bit;
    zero-mean data: under half the bound."""
    g = torch.Generator().manual_seed(9)
    B, cin, cout, N, H, W = 2, 24, 40, 3, 12, 20
    wshape = cg.weight_shape(geom, cin, cout)
    x = torch.randint(-3, 4, (B, cin, N, H, W), generator=g).float()
    gy = torch.randint(-3, 4, cg.out_shape(geom, B, cin, cout, N, H, W), generator=g).float()
    assert torch.equal(cg.emulate_wgrad(x, gy, geom, "bf16x3", grid_x=8, flush_units=2).double(), cg.wgrad_ref64(x, gy, geom, wshape).ref)
    x, w, gy = cg.make_case("zero_mean", geom, B, cin, cout, N, H, W, 5)
    assert tuple(w.shape) == wshape
    r = cg.wgrad_ref64(x, gy, geom, wshape)
    for prec in cg.PRECISIONS:
        worst = _ratio(cg.emulate_wgrad(x, gy, geom, prec, grid_x=8, flush_units=4), r, prec)
        assert worst <= 0.5, (prec, worst)


# the pairs, the shape and the seeds of tests/test_gpu_conv_grad.py::test_ragged_channel_counts
RAGGED = [(24, 40), (40, 24), (48, 72), (104, 56), (120, 96), (64, 128), (128, 128)]


@pytest.mark.parametrize("pair", RAGGED, ids=lambda p: "%dto%d" % p)
def test_ragged_pairs_octet_mutations_exceed_the_bound(pair):
    """What a wrong tail path would do to grad_w, on the GPU test's own data: the last two 8-channel octets of Cout swapped, and the last octet
    of Cin zeroed, each stand at least 4x over the bound of the true reference somewhere, in every precision -- so the GPU test's bound notices
    an octet that lands in the wrong place or is never written."""
    cin, cout = pair
    B, N, H, W = 2, 3, 12, 20
    for geom in ("k333", "k333t"):
        x, w, gy = cg.make_case("zero_mean", geom, B, cin, cout, N, H, W, seed=17 + cin + 3 * cout)
        r = cg.wgrad_ref64(x, gy, geom, tuple(w.shape))
        co_axis, ci_axis = (1, 0) if cg.GEOMETRIES[geom][3] else (0, 1)
        swapped = r.ref.clone()
        a, b = r.ref.narrow(co_axis, cout - 16, 8), r.ref.narrow(co_axis, cout - 8, 8)
        swapped.narrow(co_axis, cout - 16, 8).copy_(b)
        swapped.narrow(co_axis, cout - 8, 8).copy_(a)
        zeroed = r.ref.clone()
        zeroed.narrow(ci_axis, cin - 8, 8).zero_()
        for prec in cg.PRECISIONS:
            assert _ratio(r.ref, r, prec) == 0.0
            ws, wz = _ratio(swapped, r, prec), _ratio(zeroed, r, prec)
            assert ws >= 4.0 and wz >= 4.0, (geom, prec, ws, wz)


def test_records_round_trip_and_layout():
    """to_records / from_records (what tests/test_gpu_train_records.py hands the record entry points): the round trip gives hi + lo of
    round_parts, and the layout is [pixel][part][channel] -- checked on two pixels written out by hand."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 24, 3, 5, 7, generator=g) * 3
    for prec in cg.PRECISIONS:
        r = cg.to_records(x, prec)
        assert r.dtype == torch.int16 and tuple(r.shape) == (2, 3, 5, 7, 2 if prec == "bf16x3" else 1, 24) and r.is_contiguous()
        assert torch.equal(cg.from_records(r, prec, 24), sum(cg.round_parts(x, prec)))
    # B = 1, C = 8, N = 1, H = 1, W = 2: pixel 0 holds 1, 2, ..., 8, pixel 1 holds 1 + 2^-9 in channel 0 and -0.5 in channel 7
    t = torch.zeros(1, 8, 1, 1, 2)
    t[0, :, 0, 0, 0] = torch.arange(1.0, 9.0)
    t[0, 0, 0, 0, 1], t[0, 7, 0, 0, 1] = 1 + 2.0 ** -9, -0.5
    s16 = lambda v: v - 0x10000 if v >= 0x8000 else v
    bf = [0x3F80, 0x4000, 0x4040, 0x4080, 0x40A0, 0x40C0, 0x40E0, 0x4100]            # bfloat16 1 .. 8
    hf = [0x3C00, 0x4000, 0x4200, 0x4400, 0x4500, 0x4600, 0x4700, 0x4800]            # float16 1 .. 8
    flat = lambda prec: cg.to_records(t, prec).reshape(-1).tolist()
    # split-bf16: [pixel 0: hi x 8, lo x 8][pixel 1: hi x 8, lo x 8]; 1 + 2^-9 = bf16 1 (hi) + bf16 2^-9 (lo, 0x3B00)
    assert flat("bf16x3") == bf + [0] * 8 + [0x3F80] + [0] * 6 + [s16(0xBF00)] + [0x3B00] + [0] * 7
    # bf16: 1 + 2^-9 rounds to 1;  fp16: 1 + 2^-9 is 0x3C02
    assert flat("bf16") == bf + [0x3F80] + [0] * 6 + [s16(0xBF00)]
    assert flat("fp16") == hf + [0x3C02] + [0] * 6 + [s16(0xB800)]


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
