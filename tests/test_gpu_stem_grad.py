"""The weight gradient of the stem on the GPU: every element of grad_w against float64 CPU autograd under the ALPHA * G
bound of tests/stem_grad_ref.py, in three regimes and three precisions; exact unit impulses; small integers bit for bit; bit-identity between
calls; a full-length fp32 partial in every workgroup; the record form on a side stream between guards; stem_conv -> batch_norm3d in the
caller's autograd graph.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 17 is where the table of them goes."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402
import conv_grad_ref as cg  # noqa: E402
import stem_grad_ref as sg  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402
from test_gpu_train_records import Guarded, PREC_ID, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, N, H, W): images smaller than the 17-pixel reach (most taps are pure padding); odd sizes with exactly one in-image position for the
# outermost taps; no multiples of the 16 x 32 unit, two samples and three slices (nothing may cross a row, a slice or a sample); 80 units, ten
# per workgroup of a grid of 8 (run with DFFW_WGRAD_WGS=8)
SHAPES = [(1, 1, 1, 1), (1, 1, 4, 6), (1, 2, 17, 19), (2, 3, 20, 36), (2, 3, 32, 40), (1, 2, 128, 160)]
SMALL_GRID = (1, 2, 128, 160)
# A grid is a multiple of 8 workgroups, so a full 16 384-pixel partial in EVERY workgroup takes more than 8 x 16 384 pixels: SMALL_GRID's 40 960
# cannot give one.  This volume (section 13's) can: 320 units, 40 per workgroup of a grid of 8
FULL = (2, 5, 128, 128)
worst_seen = {}


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def case(regime, shape):
    """One case and its float64 reference, computed once and shared by the precisions."""
    x, gy = sg.make_case(regime, *shape, seed=23 + sum(shape))
    return x, gy, sg.wgrad_ref64(x, gy)


def kernels(prec):
    return ["dffw::stem_wgrad_kernel<%d>" % PREC_ID[prec], "dffw::stem_wgrad_finish_kernel"]


def run(eng, x, gy, prec):
    gw = eng.op_stem_backward(x.cuda(), gy.cuda(), precision=prec)
    assert eng.op_kernels() == kernels(prec) and tuple(gw.shape) == sg.WEIGHT_SHAPE and gw.is_cuda and gw.dtype == torch.float32
    return gw


def check(eng, regime, shape, prec, what=""):
    x, gy, r = case(regime, shape)
    gw = run(eng, x, gy, prec)
    # a NaN left by the poisoned workspace fails the check
    worst = eb.check_elementwise(gw, r, prec, "grad_w %s %s %s" % (regime, shape, what))
    print("stem_grad %s %s %s%s: grad_w err/bound %.3f" % (prec, regime, shape, what, worst))
    worst_seen[(prec, regime)] = max(worst_seen.get((prec, regime), 0.0), worst)
    return gw


@pytest.mark.parametrize("prec", sg.PRECISIONS)
@pytest.mark.parametrize("regime", sg.REGIMES)
def test_every_element_under_its_bound(eng, regime, prec, monkeypatch):
    for shape in SHAPES:
        if shape == SMALL_GRID:
            monkeypatch.setenv("DFFW_WGRAD_WGS", "8")
            assert sg.units_per_workgroup(*shape, wgs=8) == [10] * 8
        gw = check(eng, regime, shape, prec)
        if shape == (1, 1, 1, 1):   # one pixel: only the centre tap lies in the image
            centre = torch.zeros(sg.WEIGHT_SHAPE, dtype=torch.bool)
            centre[:, :, 0, 4, 4] = True
            assert float(gw.cpu()[~centre].abs().max()) == 0.0 and float(gw.cpu()[centre].abs().max()) > 0
    print("stem_grad worst so far %s %s: %.3f" % (prec, regime, worst_seen[(prec, regime)]))


@pytest.mark.parametrize("regime", sg.REGIMES)
def test_full_length_partials(eng, regime, monkeypatch):
    """The one new term of the ALPHA * G bound, the fp32 accumulation over pixels, at its full length on the hardware.  On 8 workgroups
    (DFFW_WGRAD_WGS=8, the flush interval at its default) every workgroup walks 40 units: it sums a whole 32-unit partial (16 384 pixels),
    flushes it and starts a second.  tests/test_stem_grad.py holds the CPU emulation of the same volume under 0.5; DESIGN.md section 17 has
    both figures."""
    counts = sg.units_per_workgroup(*FULL, wgs=8)
    assert len(counts) == 8 and min(counts) > sg.FLUSH_UNITS, counts
    monkeypatch.setenv("DFFW_WGRAD_WGS", "8")
    monkeypatch.delenv("DFFW_WGRAD_FLUSH_UNITS", raising=False)
    x, gy, _ = case(regime, FULL)
    for prec in sg.PRECISIONS:
        gw = check(eng, regime, FULL, prec, " full-length partials")
        assert torch.equal(gw, run(eng, x, gy, prec))


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_unit_impulses(eng, prec):
    """grad_y = one unit impulse: every element of grad_w[co] is ONE product 1 * x, the record-rounded x value 2 ky - 8 rows and 2 kx - 8 columns
    from the impulse (hi + lo as the record holds it), bit for bit; a tap outside the image and every other output channel is exactly 0.  At a
    corner, at an edge, in the interior, and at the last pixel of the last slice of the last sample."""
    B, N, H, W = 2, 3, 32, 40
    x, _ = sg.make_case("zero_mean", B, N, H, W, seed=71)
    xr = sg.rounded(x, prec)
    for co, (b, n, yy, xx) in enumerate([(0, 0, 0, 0), (0, 1, 13, W - 1), (1, 1, 17, 21), (B - 1, N - 1, H - 1, W - 1)]):
        co = (3 * co + 1) % sg.CO
        gy = torch.zeros(B, sg.CO, N, H, W)
        gy[b, co, n, yy, xx] = 1.0
        gw = run(eng, x, gy, prec).cpu()
        want = torch.zeros(sg.WEIGHT_SHAPE)
        inside = 0
        for ky in range(sg.K):
            for kx in range(sg.K):
                sy, sx = yy + sg.DIL * ky - sg.PAD, xx + sg.DIL * kx - sg.PAD
                if 0 <= sy < H and 0 <= sx < W:
                    want[co, :, 0, ky, kx] = xr[b, :, n, sy, sx]
                    inside += 1
        assert torch.equal(gw, want), (prec, (b, n, yy, xx), int((gw != want).sum()))
        assert torch.equal(want.double(), sg.wgrad64(xr, gy))
        assert 25 <= inside <= 81 and float(gw[co].abs().max()) > 0
    assert inside == 25      # the last pixel: taps below and to the right of the centre are outside


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_integers_runs_and_grids(eng, prec, monkeypatch):
    """Small-integer data (exact in every format and order) equals float64 autograd bit for bit, at the default grid and with DFFW_WGRAD_WGS=8 and
    a short flush interval.  Two calls on one grid give identical bits; two grids both stay inside the bound."""
    shape = (2, 3, 32, 40)
    xi, gi = sg.int_case(*shape, seed=3)
    ref = sg.wgrad64(xi, gi)
    x, gy, r = case("zero_mean", shape)
    assert torch.equal(run(eng, xi, gi, prec).cpu().double(), ref)
    a1, a2 = run(eng, x, gy, prec), run(eng, x, gy, prec)
    assert torch.equal(a1, a2)
    monkeypatch.setenv("DFFW_WGRAD_WGS", "8")
    monkeypatch.setenv("DFFW_WGRAD_FLUSH_UNITS", "8")      # 512 pixels: a flush after every unit
    assert sg.units_per_workgroup(*shape, wgs=8) == [3] * 8
    assert torch.equal(run(eng, xi, gi, prec).cpu().double(), ref)
    b1, b2 = run(eng, x, gy, prec), run(eng, x, gy, prec)
    assert torch.equal(b1, b2)
    wa, wb = eb.check_elementwise(a1, r, prec, "default grid"), eb.check_elementwise(b1, r, prec, "grid of 8")
    print("stem_grad two grids %s %s: err/bound %.3f (default) %.3f (8 workgroups)" % (prec, shape, wa, wb))


def test_refusals(eng):
    from dffinthewild_amd import pipeline
    x = torch.zeros(1, 3, 2, 8, 8, device="cuda")
    gy = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    w = torch.zeros(sg.WEIGHT_SHAPE)
    eng.op_stem_backward(x, gy)
    with pytest.raises(ValueError):      # not the stem's channels; grad_y of another shape; dimensions
        eng.op_stem_backward(torch.zeros(1, 8, 2, 8, 8, device="cuda"), gy)
    with pytest.raises(ValueError):
        eng.op_stem_backward(x, gy[:, :4].contiguous())
    with pytest.raises(ValueError):
        eng.op_stem_backward(x, gy[:, :, :, :4].contiguous())
    with pytest.raises(ValueError):
        eng.op_stem_backward(x[0], gy[0])
    with pytest.raises(ValueError):
        eng.op_stem_backward(x[:, :, :0], gy[:, :, :0])      # no slices
    with pytest.raises(KeyError):
        eng.op_stem_backward(x, gy, precision="fp8")
    with pytest.raises(RuntimeError):    # CPU tensors: no fallback
        eng.op_stem_backward(x.cpu(), gy.cpu())
    with pytest.raises(ValueError, match="data gradient"):
        pipeline.stem_conv(x.clone().requires_grad_(), w)
    with pytest.raises(ValueError):
        pipeline.stem_conv(x, torch.zeros(8, 3, 1, 3, 3))


# ---- the record form, as a training step calls it ---------------------------------------------------------------------------------------------
def wgrad_on_records(eng, prec, x, gy, fill):
    """dffw_stem_wgrad on x (device fp32) and the records of gy, on a side stream, workspace and grad_w guarded; grad_w (a copy) after the checks."""
    B, _, N, H, W = x.shape
    dev = torch.cuda.current_device()
    xd, gyr = x.cuda().contiguous(), cg.to_records(gy, prec).cuda()
    wsb = eng.lib.dffw_stem_wgrad_workspace_bytes(B, N, H, W)
    assert wsb == 8 * sg.grid_x_of(B, N, H, W) * sg.CO * sg.CI * sg.K * sg.K
    G = Guarded(dict(ws=wsb, gw=4 * sg.CO * sg.CI * sg.K * sg.K))
    G.raw("ws").fill_(fill)
    stream, sp = side_stream()
    rc = eng.lib.dffw_stem_wgrad(dev, PREC_ID[prec], xd.data_ptr(), gyr.data_ptr(), B, N, H, W, G.ptr("gw"), G.ptr("ws"), wsb, sp)
    assert rc == 0, eng.lib.dffw_last_error().decode()
    assert eng.op_kernels() == kernels(prec)
    stream.synchronize()
    G.check()
    return G.view("gw", torch.float32, sg.WEIGHT_SHAPE).clone()


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_record_form(eng, prec):
    """dffw_stem_wgrad on caller-built records of grad_y, a workspace of exactly dffw_stem_wgrad_workspace_bytes() and a side stream: rc 0, the
    two launches, nothing written outside workspace and grad_w, grad_w bit-identical to op_stem_backward on the same fp32 tensors and under
    ALPHA * G.  A workspace of zeros gives the same bits as one of 0xFF.  (That the reported names are kernel symbols of the library is
    tests/test_stem_grad.py::test_kernel_names_are_symbols_of_the_library.)"""
    shape = (2, 3, 20, 36)
    x, gy, r = case("zero_mean", shape)
    gw = wgrad_on_records(eng, prec, x, gy, 0xFF)
    assert torch.equal(gw, wgrad_on_records(eng, prec, x, gy, 0x00))
    assert torch.equal(gw, run(eng, x, gy, prec))
    worst = eb.check_elementwise(gw, r, prec, "grad_w of the record form")
    print("stem_grad record form %s %s: err/bound %.3f" % (prec, shape, worst))
    # a short workspace: DFFW_ENOMEM before any launch
    wsb = eng.lib.dffw_stem_wgrad_workspace_bytes(*shape)
    buf = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(sg.WEIGHT_SHAPE, device="cuda")
    rec = cg.to_records(gy, prec).cuda()
    rc = eng.lib.dffw_stem_wgrad(torch.cuda.current_device(), PREC_ID[prec], x.cuda().data_ptr(), rec.data_ptr(), *shape, out.data_ptr(), buf.data_ptr(),
                                 wsb - 8, None)
    assert rc == -3 and eng.op_kernels() == [], rc


# ---- the stem in the caller's autograd graph ----------------------------------------------------------------------------------------------------
def test_autograd_stem_bn_relu(eng):
    """pipeline.stem_conv -> pipeline.batch_norm3d(relu=True) at (2, 3, 32, 40), split-bf16, against a random cotangent: weight.grad, gamma.grad
    and beta.grad against the float64 CPU graph evaluated from the GPU's own intermediates, the ReLU mask taken from the GPU's stored output.  The
    forward holds its own bound; the BatchNorm backward holds its own at the cotangent (a record value: nothing is rounded on entry); the stem's
    weight gradient holds ALPHA * G at the gradient the GPU handed it plus the BatchNorm's bound of that gradient carried through the same
    contraction with absolute values."""
    from dffinthewild_amd import pipeline
    prec, shape = "bf16x3", (2, 3, 32, 40)
    B, N, H, W = shape
    g = torch.Generator().manual_seed(19)
    x, _ = sg.make_case("zero_mean", *shape, seed=83)
    w = (torch.rand(sg.WEIGHT_SHAPE, generator=g) * 2 - 1) * (2.0 / 243) ** 0.5 * 1.7
    gamma, beta = 0.5 + torch.rand(sg.CO, generator=g), torch.rand(sg.CO, generator=g) - 0.5
    cot = R.rounded(torch.randn(B, sg.CO, N, H, W, generator=g), prec)
    rm, rv = torch.zeros(sg.CO, device="cuda"), torch.ones(sg.CO, device="cuda")
    wg = w.clone().requires_grad_(True)
    gg, bg = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    xd = x.cuda()
    y1 = pipeline.stem_conv(xd, wg, precision=prec)
    assert eng.last_conv_kernel().startswith("dffw::")
    a = pipeline.batch_norm3d(y1, gg, bg, rm, rv, relu=True, precision=prec)
    y1.retain_grad()
    a.backward(cot.cuda())
    y1c, ac, g1_gpu = y1.detach().cpu(), a.detach().cpu(), y1.grad.cpu()
    # the forward: the stem under the forward's bound
    wf = eb.check_elementwise(y1c, eb.conv_ref64(x, w, **sg.GEOMETRY), prec, "stem forward")
    # stage 1, BatchNorm at the GPU's y1, its stored output's mask, the cotangent as handed
    zero = torch.zeros(sg.CO)
    bcase = dict(x=y1c, gamma=gamma, beta=beta, res=None, gy=cot, rm0=zero, rv0=zero + 1)
    r = R.reference(bcase, prec, True, False, y_stored=ac)
    own = R.bounds(r, prec)
    E1 = own["gx"]
    # stage 2, the stem's weight gradient
    gw64 = sg.wgrad64(x, r["gx"])
    bw = sg.wgrad_ref64(x, g1_gpu).bound(prec) + sg.wgrad64(x.abs(), E1)
    checks = {"y1.grad": (g1_gpu, r["gx"], E1), "gamma.grad": (gg.grad, r["dgamma"], own["dgamma"]), "beta.grad": (bg.grad, r["dbeta"], own["dbeta"]),
              "weight.grad": (wg.grad, gw64, bw)}
    worst = {}
    for name, (got, ref, bound) in checks.items():
        err = (got.detach().cpu().double() - ref).abs()
        worst[name] = float(eb._ratio(err, bound).max())
        assert bool((err <= bound).all()), (name, worst[name])
    print("autograd stem_conv -> BN -> ReLU: forward err/bound %.3f; " % wf + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert not wg.grad.is_cuda and wg.grad.shape == w.shape and float(wg.grad.abs().max()) > 0 and float(gg.grad.abs().max()) > 0
    assert 0 < float((ac > 0).double().mean()) < 1
    with pytest.raises(ValueError, match="data gradient"):
        pipeline.stem_conv(xd.clone().requires_grad_(), wg, precision=prec)
