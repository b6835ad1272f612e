"""dffw_op_conv3d_backward on the GPU: every element of grad_x and grad_w against float64 CPU autograd under the bounds of
tests/conv_grad_ref.py (the forward's ALPHA * D for the adjoint conv, ALPHA * G for the weight gradient); bit-identity between calls, grids and
`need` subsets; the exact unit-impulse case; the ragged channel counts (every multiple of 8 the entry point admits has tail paths in the kernel's
tiling: RAGGED); one full-length fp32 partial per workgroup on the hardware; the refusals; the autograd node behind HeadsLoss.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 13 is where the per-geometry table of them goes."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_grad_ref as cg  # noqa: E402
import loss_ref as L  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = [(8, 8), (8, 16), (16, 8), (16, 32), (32, 32), (64, 32), (32, 64), (64, 64)]
# channel counts off the powers of two.  In the non-transposed geometries (g = grad_y with Cout channels in 16-channel tiles, f = x with Cin channels
# in 32-channel groups of two 16-wide column tiles): a half-filled last tile of g (Cout 40, 24, 72, 56), a full one with 6 and 8 tiles (96, 128), f tails
# of 8, 16 and 24 channels (Cin 40 / 104, 48, 24 / 120), 1 to 4 groups of f; k333t swaps the roles, so every class also falls on the other operand
RAGGED = [(24, 40), (40, 24), (48, 72), (104, 56), (120, 96), (64, 128), (128, 128)]
# (B, N, H, W): one tile without slice neighbours; both slice paddings on every slice; ragged tile edges and B > 1; several units per workgroup
SHAPES = [(1, 1, 8, 8), (1, 2, 8, 16), (2, 3, 12, 20), (1, 4, 40, 24)]


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def case(geom, cin, cout, shape, regime="zero_mean", channel=None):
    """One case and its float64 references, computed once and shared by the precisions (``channel``: the impulse regime's grad_y channel)."""
    B, N, H, W = shape
    x, w, gy = cg.make_case(regime, geom, B, cin, cout, N, H, W, seed=17 + cin + 3 * cout, impulse_channel=channel)
    return x, w, gy, cg.dgrad_ref64(w, gy, geom), cg.wgrad_ref64(x, gy, geom, tuple(w.shape))


def run(eng, geom, x, w, gy, prec, need=("x", "w")):
    _, s, p, t = cg.GEOMETRIES[geom]
    return eng.op_conv3d_backward(x.cuda(), w, gy.cuda(), stride=s, pad=p, transposed=t, precision=prec, need=need)


def check(eng, geom, cin, cout, shape, prec, regime="zero_mean"):
    x, w, gy, rx, rw = case(geom, cin, cout, shape, regime)
    gx, gw = run(eng, geom, x, w, gy, prec)
    kernels = eng.op_kernels()
    assert len(kernels) == 2 and kernels[0].startswith("dffw::conv_wgrad_kernel<") and kernels[1] == "dffw::conv_wgrad_finish_kernel", kernels
    # a NaN left by the poisoned workspace fails either check
    wx = eb.check_elementwise(gx, rx, prec, "grad_x %s %d->%d %s" % (geom, cin, cout, shape))
    ww = eb.check_elementwise(gw, rw, prec, "grad_w %s %d->%d %s" % (geom, cin, cout, shape))
    print("conv_grad %s %s %d->%d %s %s: grad_x err/bound %.3f (%s), grad_w %.3f" % (geom, prec, cin, cout, shape, regime, wx, eng.last_conv_kernel(), ww))
    return gx, gw


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dto%d" % p)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_every_element_under_its_bound(eng, geom, pair, prec):
    for shape in SHAPES:
        check(eng, geom, pair[0], pair[1], shape, prec)


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_widest_channels(eng, geom, prec):
    check(eng, geom, 128, 64, SHAPES[1], prec)


@pytest.mark.parametrize("regime", ["post_relu", "offset", "one_sample"])
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_regimes(eng, geom, regime):
    for prec in cg.PRECISIONS:
        check(eng, geom, 16, 32, SHAPES[2], prec, regime)


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_bit_identical_runs_grids_and_subsets(eng, geom, prec, monkeypatch):
    """Two calls, and `need` subsets, give identical bits; a persistent grid forced small (DFFW_WGRAD_WGS, one workgroup walks many units) with a short
    flush interval (DFFW_WGRAD_FLUSH_UNITS) is deterministic as well and stays under the bound (its float64 sums differ in order, not in bits kept)."""
    cin, cout, shape = 16, 32, SHAPES[3]
    x, w, gy, rx, rw = case(geom, cin, cout, shape)
    gx, gw = run(eng, geom, x, w, gy, prec)
    gx2, gw2 = run(eng, geom, x, w, gy, prec)
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2)
    only_x, none_w = run(eng, geom, x, w, gy, prec, need=("x",))
    assert none_w is None and torch.equal(only_x, gx) and eng.op_kernels() == []
    none_x, only_w = run(eng, geom, x, w, gy, prec, need=("w",))
    assert none_x is None and torch.equal(only_w, gw)
    monkeypatch.setenv("DFFW_WGRAD_WGS", "8")
    monkeypatch.setenv("DFFW_WGRAD_FLUSH_UNITS", "3")
    _, small = run(eng, geom, x, w, gy, prec, need=("w",))
    _, small2 = run(eng, geom, x, w, gy, prec, need=("w",))
    assert torch.equal(small, small2)
    eb.check_elementwise(small, rw, prec, "grad_w on the small grid")


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_unit_impulse_gives_the_shifted_patch(eng, geom, prec):
    """grad_y = one unit impulse: every grad_w element is ONE product 1 * x, so it equals the rounded operand exactly (hi + lo of an fp32 value
    is an fp32 value; the float64 finish adds zeros)."""
    cin, cout, shape = 16, 8, SHAPES[2]
    x, w, gy, _, rw = case(geom, cin, cout, shape, "impulse")
    _, gw = run(eng, geom, x, w, gy, prec, need=("w",))
    want = cg.wgrad_ref64(sum(cg.round_parts(x, prec)), gy, geom, tuple(w.shape)).ref    # in all four geometries the patch is x's
    assert torch.equal(gw.cpu().double(), want)
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", RAGGED, ids=lambda p: "%dto%d" % p)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_ragged_channel_counts(eng, geom, pair, prec):
    """Every element of grad_x and grad_w (and the two-launch list) at channel counts whose last 16-tile of g is half filled, whose last 32-group
    of f holds 8, 16 or 24 channels, with up to 8 tiles of g and 4 groups of f; grad_x sends the forward dispatch the same counts."""
    for shape in SHAPES[1:3]:
        check(eng, geom, pair[0], pair[1], shape, prec)


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", [(16, 8), (24, 40), (40, 24)], ids=lambda p: "%dto%d" % p)
@pytest.mark.parametrize("geom", list(cg.GEOMETRIES))
def test_unit_impulse_in_the_last_channel_and_ragged_pairs(eng, geom, pair, prec):
    """The unit impulse in grad_y's LAST channel (the last octet of the last tile) and, for the ragged pairs, in cout // 2 as well: every grad_w
    element equals the rounded operand exactly, so an octet or a tile that lands in another place fails outright."""
    cin, cout = pair
    for channel in ((cout - 1,) if pair == (16, 8) else (cout - 1, None)):
        x, w, gy, _, _ = case(geom, cin, cout, SHAPES[2], "impulse", channel)
        assert float(gy[:, cout - 1 if channel is not None else cout // 2].sum()) == 1.0 and float(gy.sum()) == 1.0
        _, gw = run(eng, geom, x, w, gy, prec, need=("w",))
        want = cg.wgrad_ref64(sum(cg.round_parts(x, prec)), gy, geom, tuple(w.shape)).ref
        assert torch.equal(gw.cpu().double(), want), (channel, int((gw.cpu().double() != want).sum()))
        assert float(want.abs().max()) > 0


FULL = (2, 5, 128, 128)   # the grid-side volume (B, N, Hg, Wg): 2 560 units, 320 per workgroup of a grid of 8


@functools.lru_cache(maxsize=None)
def full_case(geom, regime):
    """8 -> 16 channels with the grid-side volume FULL, and the float64 reference of grad_w; shared by the precisions."""
    B, N, Hg, Wg = FULL
    S, transposed = cg.GEOMETRIES[geom][1][1], cg.GEOMETRIES[geom][3]
    H, W = (Hg, Wg) if transposed else (S * Hg, S * Wg)    # the transposed form has x on the grid
    x, w, gy = cg.make_case(regime, geom, B, 8, 16, N, H, W, seed=41)
    return x, w, gy, cg.wgrad_ref64(x, gy, geom, tuple(w.shape))


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("regime", ["zero_mean", "offset"])
@pytest.mark.parametrize("geom", ["k333", "k333s2", "k333t"])
def test_full_length_partials(eng, geom, regime, prec, monkeypatch):
    """The one new term of the ALPHA * G bound, the fp32 accumulation over pixels, at its full length on the hardware: on a grid of 8 workgroups
    (DFFW_WGRAD_WGS=8, the flush interval left at its default) every workgroup walks 320 units of FULL, so at every slice tap some workgroup sums a
    whole 256-unit partial (16 384 pixels), flushes it and goes on into a second one.  Every element of grad_w under ALPHA * G; two calls
    bit-identical.  tests/test_conv_grad.py holds the CPU emulation of the same length (sequential fp32) under 0.5; DESIGN.md section 13 has
    both figures."""
    B, N, Hg, Wg = FULL
    counted = cg.counted_units(geom, B, N, Hg, Wg, 8)
    assert len(counted) == 3 and all(max(c) > cg.FLUSH_UNITS for c in counted), counted
    monkeypatch.setenv("DFFW_WGRAD_WGS", "8")
    monkeypatch.delenv("DFFW_WGRAD_FLUSH_UNITS", raising=False)
    x, w, gy, rw = full_case(geom, regime)
    _, gw = run(eng, geom, x, w, gy, prec, need=("w",))
    _, gw2 = run(eng, geom, x, w, gy, prec, need=("w",))
    worst, _ = eb.elementwise_ratio(gw, rw, prec)
    print("conv_grad full-length partials %s %s %s 8->16 %s: grad_w err/bound %.3f" % (geom, prec, regime, FULL, worst))
    eb.check_elementwise(gw, rw, prec, "grad_w %s %s at full-length partials" % (geom, regime))
    assert torch.equal(gw, gw2)


def test_refusals(eng):
    x = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    w = torch.zeros(8, 8, 3, 3, 3)
    gy = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    ok = dict(stride=1, pad=1, transposed=False)
    with pytest.raises(ValueError):      # a geometry outside the four
        eng.op_conv3d_backward(x, torch.zeros(8, 8, 3, 1, 1), gy, stride=1, pad=(1, 0, 0))
    with pytest.raises(ValueError):
        eng.op_conv3d_backward(x, w, gy, stride=1, pad=0)
    with pytest.raises(ValueError):      # dilation
        eng.op_conv3d_backward(x, w, gy, dilation=2, **ok)
    with pytest.raises(ValueError):      # channels: not a multiple of 8, above 128
        eng.op_conv3d_backward(x[:, :4].contiguous(), w[:, :4].contiguous(), gy, **ok)
    with pytest.raises(ValueError):
        eng.op_conv3d_backward(torch.zeros(1, 136, 1, 8, 8, device="cuda"), torch.zeros(8, 136, 3, 3, 3), gy[:, :, :1], **ok)
    with pytest.raises(ValueError):      # odd H at stride 2
        eng.op_conv3d_backward(torch.zeros(1, 8, 2, 7, 8, device="cuda"), w, torch.zeros(1, 8, 2, 4, 4, device="cuda"), stride=(1, 2, 2), pad=1)
    with pytest.raises(ValueError):      # grad_y of another shape
        eng.op_conv3d_backward(x, w, gy[:, :, :, :4].contiguous(), **ok)
    with pytest.raises(RuntimeError):    # CPU tensors: no fallback
        eng.op_conv3d_backward(x.cpu(), w, gy.cpu(), **ok)
    assert eng.op_kernels() == []        # nothing was launched


def test_autograd_conv_behind_heads_loss(eng):
    """pipeline.conv3d -> HeadsLoss: x.grad and w.grad against the float64 CPU graph of loss and conv backward, evaluated at the score volumes the
    GPU conv produced.  Composed bound: the conv backward's own bound on the score gradient the GPU saw, plus the loss kernel's bound
    (loss_ref.ALPHA * G) carried through the adjoint conv / the weight-gradient contraction with absolute values."""
    from dffinthewild_amd import pipeline
    geom, prec = "k333", "bf16x3"
    g = torch.Generator().manual_seed(5)
    x, w, _ = cg.make_case("zero_mean", geom, 1, 8, 8, 4, 16, 16, 23)
    fd = 0.1 + 1.4 * torch.rand(1, 4, 1, 1, generator=g)
    gt = 0.1 + 1.4 * torch.rand(1, 16, 16, generator=g)
    mask = torch.rand(1, 16, 16, generator=g) < 0.7
    xg, wg = x.cuda().requires_grad_(True), w.clone().requires_grad_(True)
    y = pipeline.conv3d(xg, wg, stride=1, pad=1, precision=prec)
    y.retain_grad()
    total = pipeline.HeadsLoss.apply(y[:, 0], y[:, 1], y[:, 2], y[:, 3], fd.cuda(), gt.cuda(), mask.cuda())
    total.backward()
    assert xg.grad.is_cuda and not wg.grad.is_cuda and wg.grad.shape == w.shape
    gy_gpu = y.grad.cpu()
    assert float(gy_gpu[:, 4:].abs().max()) == 0.0
    # the float64 graph from the GPU's score volumes on
    lcase = dict(scores=[y.detach()[:, k].cpu() for k in range(4)], fd=fd, gt=gt, mask=mask, conf=None, weights=list(L.WEIGHTS), rng=None)
    gy64 = torch.zeros_like(gy_gpu, dtype=torch.float64)
    E = torch.zeros_like(gy64)
    for k, (gk, Gk) in enumerate(zip(L.reference(lcase)["grads"], L.bound(lcase))):
        gy64[:, k], E[:, k] = gk, L.ALPHA * Gk
    assert bool(((gy_gpu.double() - gy64).abs() <= E).all())
    gx64, gw64 = cg.grads64(x, w, gy64, geom)
    rx, rw = cg.dgrad_ref64(w, gy_gpu, geom), cg.wgrad_ref64(x, gy_gpu, geom, tuple(w.shape))
    wa, kw = cg.adjoint_conv(w, geom)
    bx = rx.bound(prec) + eb.conv_ref64(E, wa.abs(), **kw).ref
    bw = rw.bound(prec) + cg.wgrad_ref64(x.abs(), E, geom, tuple(w.shape)).ref
    ex, ew = (xg.grad.cpu().double() - gx64).abs(), (wg.grad.double() - gw64).abs()
    # (eb._ratio: 0 / 0 counts as 0 -- the filter rows of the four unused score channels have gradient and bound exactly zero)
    print("autograd conv -> HeadsLoss: x.grad err/bound %.3f, w.grad %.3f" % (float(eb._ratio(ex, bx).max()), float(eb._ratio(ew, bw).max())))
    assert bool((ex <= bx).all()) and bool((ew <= bw).all())
    with pytest.raises(RuntimeError):
        pipeline.conv3d(x, w, stride=1, pad=1)
