"""Backward of the pools on the GPU: every element of the gradient against float64 CPU autograd on the record-rounded
operands under the bounds of tests/pool_grad_ref.py (exact for max without b, and for avg without b in the bf16 formats), in all three
precisions, through the op forms and their poisoned workspace; the tie rule in the regimes that hold ties; unit impulses at the row, slice and
sample boundaries; the pyramid against the single levels; bit-identity between calls and grids; the record forms on a side stream between
guards; the autograd chains conv -> max pool -> conv and pyramid -> three convs.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 16 is where the table of them goes."""
import functools
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_grad_ref as cg  # noqa: E402
import pool_grad_ref as pg  # noqa: E402
import pw_grad_ref as pw  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402
from test_gpu_train_records import Guarded, PREC_ID, nbytes_records, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

MODE_ID = {"max": 0, "avg": 1}


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def pool_name(prec, mode, k, add):
    return "dffw::pool_bwd_kernel<%d, %d, %d, %d>" % (PREC_ID[prec], MODE_ID[mode], k, int(add))


def pool3_name(prec, add):
    return "dffw::pool3_bwd_kernel<%d, %d>" % (PREC_ID[prec], int(add))


def small_grid(monkeypatch, case):
    """(2, 10, 32, 32) runs on a grid of 8 workgroups: 40 units, every workgroup walks five."""
    if case == pg.SMALL_GRID:
        monkeypatch.setenv("DFFW_BN_WGS", "8")
    else:
        monkeypatch.delenv("DFFW_BN_WGS", raising=False)


def cuda(t):
    return None if t is None else t.cuda()


@functools.lru_cache(maxsize=None)
def max_case(shape, C, xregime, gregime):
    """One max-pool case, its operands and its float64 references without and with b, computed once and shared by the precisions."""
    seed = 23 + C + sum(shape)
    x, g, b = pg.make_x(xregime, shape, C, seed), pg.make_g(gregime, shape, C, 2, seed + 1), pg.make_g(gregime, shape, C, 1, seed + 2)
    refs = {(prec, wb): pg.pool_ref64(g, x, b if wb else None, 2, "max", prec) for prec in pg.PRECISIONS for wb in (False, True)}
    return x, g, b, refs


@functools.lru_cache(maxsize=None)
def avg_case(shape, C, k, gregime):
    seed = 29 + C + sum(shape) + k
    g, b = pg.make_g(gregime, shape, C, k, seed), pg.make_g(gregime, shape, C, 1, seed + 1)
    refs = {(prec, wb): pg.pool_ref64(g, None, b if wb else None, k, "avg", prec) for prec in pg.PRECISIONS for wb in (False, True)}
    return g, b, refs


@functools.lru_cache(maxsize=None)
def pyramid_case(shape, C, gregime):
    seed = 31 + C + sum(shape)
    g2, g4, g8, b = (pg.make_g(gregime, shape, C, k, seed + k) for k in (2, 4, 8, 1))
    refs = {(prec, wb): pg.pool3_ref64(g2, g4, g8, b if wb else None, prec) for prec in pg.PRECISIONS for wb in (False, True)}
    return g2, g4, g8, b, refs


# 1 + 2^-12 U(0, 1) shares one record under bf16 only: that regime runs there
@pytest.mark.parametrize("xregime,prec", [(r, p) for r in pg.X_REGIMES for p in pg.PRECISIONS if r != "rounding_ties" or p == "bf16"])
def test_max_without_b_is_exact(eng, xregime, prec, monkeypatch):
    """The bits of rounded(g) at the first maximum of the stored x, +0 (sign bit clear) at the window's other three pixels.  A NaN left by the
    poisoned workspace, or an element no thread wrote, fails the comparison."""
    for case in pg.CASES[("max", 2)]:
        small_grid(monkeypatch, case)
        shape, C = case
        x, g, _, refs = max_case(shape, C, xregime, "zero_mean")
        ref, bound = refs[(prec, False)]
        assert float(bound.max()) == 0.0
        out = eng.op_pool_backward(g.cuda(), x=x.cuda(), k=2, mode="max", precision=prec).cpu()
        assert eng.op_kernels() == [pool_name(prec, "max", 2, False)]
        assert pg.same_bits(out, ref.float()) and torch.equal(out.double(), ref), (case, int((out.double() != ref).sum()))
        if xregime == "post_relu" and x.numel() > 32:
            share = pg.tie_share(x, prec)
            print("pool_grad max %s %s C=%d: %.1f %% of the windows hold a tie" % (prec, shape, C, 100 * share))
            assert share >= 0.05
        if xregime == "rounding_ties" and x.numel() > 32:
            assert pg.tie_share(x, prec) == 1.0 and not torch.equal(out, pg.emulate("max", prec, g=g, x=x, fault="argmax_unrounded"))


@pytest.mark.parametrize("prec", pg.PRECISIONS)
@pytest.mark.parametrize("gregime", pg.G_REGIMES)
def test_max_with_b(eng, gregime, prec, monkeypatch):
    worst = 0.0
    for case in pg.CASES[("max", 2)]:
        small_grid(monkeypatch, case)
        shape, C = case
        x, g, b, refs = max_case(shape, C, "post_relu", gregime)
        ref, bound = refs[(prec, True)]
        out = eng.op_pool_backward(g.cuda(), x=x.cuda(), b=b.cuda(), k=2, mode="max", precision=prec).cpu()
        assert eng.op_kernels() == [pool_name(prec, "max", 2, True)]
        worst = max(worst, pg.check(out, ref, bound, "max + b %s %s" % (prec, case)))
        assert torch.equal(out, pg.emulate("max", prec, g=g, x=x, b=b)), case
    print("pool_grad max + b %s %s: err/bound %.3f" % (prec, gregime, worst))


@pytest.mark.parametrize("prec", pg.PRECISIONS)
@pytest.mark.parametrize("gregime", pg.G_REGIMES)
@pytest.mark.parametrize("k", [2, 4, 8])
def test_avg(eng, k, gregime, prec, monkeypatch):
    """Without b: exact in the bf16 formats, within FP16_SUB in fp16.  With b: (u + 2^-23) |ref64| (+ FP16_SUB)."""
    worst = [0.0, 0.0]
    for case in pg.CASES[("avg", k)]:
        small_grid(monkeypatch, case)
        shape, C = case
        g, b, refs = avg_case(shape, C, k, gregime)
        for wb in (False, True):
            ref, bound = refs[(prec, wb)]
            out = eng.op_pool_backward(g.cuda(), b=cuda(b if wb else None), k=k, mode="avg", precision=prec).cpu()
            assert eng.op_kernels() == [pool_name(prec, "avg", k, wb)]
            if not wb and prec != "fp16":
                assert float(bound.max()) == 0.0 and torch.equal(out.double(), ref), case
            worst[wb] = max(worst[wb], pg.check(out, ref, bound, "avg k=%d %s %s b=%s" % (k, prec, case, wb)))
            assert torch.equal(out, pg.emulate("avg", prec, k=k, g=g, b=b if wb else None)), (case, wb)
    print("pool_grad avg k=%d %s %s: err/bound without b %.3f, with b %.3f" % (k, prec, gregime, worst[0], worst[1]))


@pytest.mark.parametrize("prec", pg.PRECISIONS)
@pytest.mark.parametrize("gregime", pg.G_REGIMES)
def test_pyramid(eng, gregime, prec, monkeypatch):
    worst = [0.0, 0.0]
    for case in pg.CASES[("pyramid", 8)]:
        small_grid(monkeypatch, case)
        shape, C = case
        g2, g4, g8, b, refs = pyramid_case(shape, C, gregime)
        for wb in (False, True):
            ref, bound = refs[(prec, wb)]
            out = eng.op_pool3_backward(g2.cuda(), g4.cuda(), g8.cuda(), cuda(b if wb else None), precision=prec).cpu()
            assert eng.op_kernels() == [pool3_name(prec, wb)]
            worst[wb] = max(worst[wb], pg.check(out, ref, bound, "pyramid %s %s b=%s" % (prec, case, wb)))
            assert torch.equal(out, pg.emulate("pyramid", prec, g2=g2, g4=g4, g8=g8, b=b if wb else None)), (case, wb)
    print("pool_grad pyramid %s %s: err/bound without b %.3f, with b %.3f" % (prec, gregime, worst[0], worst[1]))


@pytest.mark.parametrize("prec", pg.PRECISIONS)
def test_small_integers_equal_autograd(eng, prec, monkeypatch):
    """Data exact in every format and at every step: every form with b equals float64 autograd bit for bit, at a channel count with three octets
    and on the small grid."""
    for (mode, k), cases in pg.CASES.items():
        for case in cases[-3::2]:      # C = 24 at the middle shape, and the small grid
            small_grid(monkeypatch, case)
            shape, C = case
            b = pg.int_g(shape, C, 1, 9)
            if mode == "pyramid":
                g2, g4, g8 = (pg.int_g(shape, C, kk, 9 + kk) for kk in (2, 4, 8))
                ref, _ = pg.pool3_ref64(g2, g4, g8, b, prec)
                out = eng.op_pool3_backward(g2.cuda(), g4.cuda(), g8.cuda(), b.cuda(), precision=prec)
            else:
                g, x = pg.int_g(shape, C, k, 9 + k), pg.make_x("plateau", shape, C, 10)
                ref, _ = pg.pool_ref64(g, x, b, k, mode, prec)
                out = eng.op_pool_backward(g.cuda(), x=x.cuda() if mode == "max" else None, b=b.cuda(), k=k, mode=mode, precision=prec)
            assert torch.equal(out.cpu().double(), ref), (mode, k, case)


@pytest.mark.parametrize("prec", pg.PRECISIONS)
def test_unit_impulse(eng, prec):
    """g = 1 at sample 0's last slice, last pooled row, last pooled column, and at sample 1's first pooled pixel, in the last channel: the result is
    nonzero exactly in those two windows (blocks) of that channel -- nothing crosses a row, slice or sample boundary -- with the stated values:
    max: 1 at each window's argmax (x falling in row-major window order puts it at the window's first element; rising, at its last); avg:
    k^-2 over the window; pyramid: 2^-2, 2^-4, 2^-6 over the 2x2, 4x4, 8x8 block of the level that carries the impulse."""
    C = 8

    def impulse(shape, k):
        B, N, H, W = shape
        g = torch.zeros(B, C, N, H // k, W // k)
        g[0, C - 1, N - 1, -1, -1] = 1.0
        g[1, C - 1, 0, 0, 0] = 1.0
        return g

    def windows(shape, k, value):
        B, N, H, W = shape
        want = torch.zeros(B, C, N, H, W)
        want[0, C - 1, N - 1, H - k:, W - k:] = value
        want[1, C - 1, 0, :k, :k] = value
        return want

    for k in (2, 4, 8):
        shape = (2, 3, 16, 24) if k == 8 else (2, 3, 12, 20)
        B, N, H, W = shape
        g = impulse(shape, k)
        out = eng.op_pool_backward(g.cuda(), k=k, mode="avg", precision=prec).cpu()
        assert pg.same_bits(out, windows(shape, k, 1.0 / (k * k))), k
        if k == 2:
            pat = ((torch.arange(H) % 2)[:, None] * 2 + (torch.arange(W) % 2)[None, :]).float().expand(B, C, N, H, W)     # 0 1 / 2 3 in every window
            for x, (dy, dx) in ((-pat, (0, 0)), (pat, (1, 1))):
                out = eng.op_pool_backward(g.cuda(), x=x.cuda(), k=2, mode="max", precision=prec).cpu()
                want = torch.zeros(B, C, N, H, W)
                want[0, C - 1, N - 1, H - 2 + dy, W - 2 + dx] = 1.0
                want[1, C - 1, 0, dy, dx] = 1.0
                assert pg.same_bits(out, want) and pg.same_bits(out, pg.pool_ref64(g, x, None, 2, "max", prec)[0].float()), (dy, dx)
    shape = (2, 3, 16, 24)
    zeros = lambda k: torch.zeros(2, C, 3, 16 // k, 24 // k)
    for k in (2, 4, 8):
        gs = [impulse(shape, kk) if kk == k else zeros(kk) for kk in (2, 4, 8)]
        out = eng.op_pool3_backward(*[t.cuda() for t in gs], precision=prec).cpu()
        assert pg.same_bits(out, windows(shape, k, 1.0 / (k * k))), k


@pytest.mark.parametrize("prec", pg.PRECISIONS)
def test_pyramid_equals_the_single_levels(eng, prec):
    """With two of g2, g4, g8 zero and no b, op_pool3_backward equals op_pool_backward(avg, k) of the remaining one bit for bit."""
    shape, C = (2, 3, 16, 24), 24
    g2, g4, g8, _, _ = pyramid_case(shape, C, "zero_mean")
    for k, g in ((2, g2), (4, g4), (8, g8)):
        gs = [t.cuda() if t is g else torch.zeros_like(t).cuda() for t in (g2, g4, g8)]
        both = eng.op_pool3_backward(*gs, precision=prec)
        single = eng.op_pool_backward(g.cuda(), k=k, mode="avg", precision=prec)
        assert torch.equal(both, single) and float(single.abs().max()) > 0, k


@pytest.mark.parametrize("prec", pg.PRECISIONS)
def test_bit_identical_calls_and_grids(eng, prec, monkeypatch):
    """Two calls give identical bits, and the default grid gives the bits of DFFW_BN_WGS=8."""
    shape, C = pg.SMALL_GRID
    x, g, b, _ = max_case(shape, C, "post_relu", "offset")
    g2, g4, g8, b3, _ = pyramid_case(shape, C, "offset")
    runs = {
        "max": lambda: eng.op_pool_backward(g.cuda(), x=x.cuda(), k=2, mode="max", precision=prec),
        "max + b": lambda: eng.op_pool_backward(g.cuda(), x=x.cuda(), b=b.cuda(), k=2, mode="max", precision=prec),
        "avg + b": lambda: eng.op_pool_backward(g.cuda(), b=b.cuda(), k=2, mode="avg", precision=prec),
        "avg 8": lambda: eng.op_pool_backward(g8.cuda(), k=8, mode="avg", precision=prec),
        "pyramid + b": lambda: eng.op_pool3_backward(g2.cuda(), g4.cuda(), g8.cuda(), b3.cuda(), precision=prec),
    }
    monkeypatch.delenv("DFFW_BN_WGS", raising=False)
    first = {n: f() for n, f in runs.items()}
    for n, f in runs.items():
        assert torch.equal(f(), first[n]), n
    monkeypatch.setenv("DFFW_BN_WGS", "8")
    for n, f in runs.items():
        assert torch.equal(f(), first[n]), n


def test_refusals(eng):
    g = torch.zeros(1, 8, 2, 4, 4, device="cuda")
    x = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    with pytest.raises(ValueError):      # max without x; k other than 2; avg k = 3; an unknown mode
        eng.op_pool_backward(g, k=2, mode="max")
    with pytest.raises(ValueError):
        eng.op_pool_backward(g, x=torch.zeros(1, 8, 2, 16, 16, device="cuda"), k=4, mode="max")
    with pytest.raises(ValueError):
        eng.op_pool_backward(g, k=3, mode="avg")
    with pytest.raises(ValueError):
        eng.op_pool_backward(g, k=2, mode="min")
    with pytest.raises(ValueError):      # x or b of another shape; channels
        eng.op_pool_backward(g, x=g, k=2, mode="max")
    with pytest.raises(ValueError):
        eng.op_pool_backward(g, x=x, b=g, k=2, mode="max")
    with pytest.raises(ValueError):
        eng.op_pool_backward(g[:, :4].contiguous(), x=x[:, :4].contiguous(), k=2, mode="max")
    with pytest.raises(RuntimeError):    # CPU tensors: no fallback
        eng.op_pool_backward(g.cpu(), x=x.cpu(), k=2, mode="max")
    g8 = torch.zeros(1, 8, 2, 1, 1, device="cuda")
    with pytest.raises(ValueError):      # the pyramid: a level of the wrong shape; a missing level
        eng.op_pool3_backward(g, g, g8)
    with pytest.raises(ValueError):
        eng.op_pool3_backward(g, None, g8)
    assert eng.op_kernels() == []        # nothing was launched


# ---- the record forms, as a training step calls them ------------------------------------------------------------------------------------------
REC_SHAPE, REC_C = (2, 3, 16, 24), 16


def run_record_forms(eng, prec, c):
    """dffw_pool_backward(max, b) with out aliasing b, then dffw_pool3_backward, enqueued back to back on one side stream; one host
    synchronisation at the end.  Every buffer the library writes lies between guards."""
    lib, dev, Pn = eng.lib, torch.cuda.current_device(), PREC_ID[prec]
    B, N, H, W = REC_SHAPE
    C = REC_C
    rec = {n: cg.to_records(t, prec).cuda() for n, t in c.items()}
    nrec = nbytes_records(prec, B, C, N, H, W)
    G = Guarded(dict(sum=nrec, pyr=nrec))
    G.raw("sum").copy_(rec["b"].reshape(-1).view(torch.uint8))      # b's records live in the guarded buffer: out aliases b
    stream, sp = side_stream()
    names = []
    rc = lib.dffw_pool_backward(dev, Pn, 0, 2, rec["g"].data_ptr(), rec["x"].data_ptr(), G.ptr("sum"), B, C, N, H, W, G.ptr("sum"), sp)
    assert rc == 0, lib.dffw_last_error().decode()
    names.append(eng.op_kernels())
    rc = lib.dffw_pool3_backward(dev, Pn, rec["g2"].data_ptr(), rec["g4"].data_ptr(), rec["g8"].data_ptr(), None, B, C, N, H, W, G.ptr("pyr"), sp)
    assert rc == 0, lib.dffw_last_error().decode()
    names.append(eng.op_kernels())
    stream.synchronize()      # the only host synchronisation
    G.check()
    assert names == [[pool_name(prec, "max", 2, True)], [pool3_name(prec, False)]], names
    parts = 2 if prec == "bf16x3" else 1
    records = lambda n: G.view(n, torch.int16, (B, N, H, W, parts, C)).cpu().clone()
    return {n: cg.from_records(records(n), prec, C) for n in ("sum", "pyr")}


@pytest.mark.parametrize("prec", pg.PRECISIONS)
def test_record_forms(eng, lib_built, prec):
    """The record forms on caller-built records and a side stream: guards intact; results bit-identical to the op forms on the same fp32
    tensors (record values, so the op shell stages the very same records) and under their bounds; op_kernels() names the kernel launched, and
    that name is a kernel symbol of the library."""
    B, N, H, W = REC_SHAPE
    rd = lambda t: pg.rounded(t, prec)
    c = dict(x=rd(pg.make_x("post_relu", REC_SHAPE, REC_C, 71)), g=rd(pg.make_g("offset", REC_SHAPE, REC_C, 2, 72)),
             b=rd(pg.make_g("offset", REC_SHAPE, REC_C, 1, 73)), g2=rd(pg.make_g("zero_mean", REC_SHAPE, REC_C, 2, 74)),
             g4=rd(pg.make_g("zero_mean", REC_SHAPE, REC_C, 4, 75)), g8=rd(pg.make_g("zero_mean", REC_SHAPE, REC_C, 8, 76)))
    for t in c.values():
        assert torch.equal(rd(t), t)
    a = run_record_forms(eng, prec, c)
    again = run_record_forms(eng, prec, c)
    for n in a:
        assert torch.equal(a[n], again[n]), n
    op_sum = eng.op_pool_backward(c["g"].cuda(), x=c["x"].cuda(), b=c["b"].cuda(), k=2, mode="max", precision=prec)
    op_pyr = eng.op_pool3_backward(c["g2"].cuda(), c["g4"].cuda(), c["g8"].cuda(), precision=prec)
    assert torch.equal(op_sum.cpu(), a["sum"]) and torch.equal(op_pyr.cpu(), a["pyr"])
    ws = pg.check(a["sum"], *pg.pool_ref64(c["g"], c["x"], c["b"], 2, "max", prec), "record form max + b")
    wp = pg.check(a["pyr"], *pg.pool3_ref64(c["g2"], c["g4"], c["g8"], None, prec), "record form pyramid")
    print("pool_grad record forms %s C=%d %s: max + b err/bound %.3f, pyramid %.3f" % (prec, REC_C, REC_SHAPE, ws, wp))
    symbols = subprocess.run(["nm", "-DC", lib_built], capture_output=True, text=True, check=True).stdout
    for name in (pool_name(prec, "max", 2, True), pool3_name(prec, False)):
        assert "void %s(" % name in symbols, name


# ---- the pools in the caller's autograd graph --------------------------------------------------------------------------------------------------
def _le(got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    return bool((err <= bound).all()), float(eb._ratio(err, bound).max())


def test_autograd_conv_maxpool_conv(eng):
    """pipeline.conv3d (3x3x3) -> pipeline.max_pool3d -> pipeline.conv3d (3x3x3) at (1, 4, 16, 16), 8 channels, split-bf16, against the float64
    CPU graph evaluated from the GPU's own intermediates, the max pool's argmax taken from the GPU's forward values.  Each stage's own bound
    holds at the gradient the GPU handed it; the bound of that gradient is carried through the stage's adjoint with absolute values (the pool's
    adjoint is a selection: it adds nothing, its input being record values already).  A window whose float64 argmax is another element has its
    two float64 candidates within the forward bound of each other; such windows are left out of the check of the pool's gradient, and are
    fewer than 2 %."""
    from dffinthewild_amd import pipeline
    import torch.nn.functional as F
    prec, C = "bf16x3", 8
    x, w1, _ = cg.make_case("zero_mean", "k333", 1, C, C, 4, 16, 16, 43)
    _, w2, _ = cg.make_case("zero_mean", "k333", 1, C, C, 4, 8, 8, 47)
    gy = pg.make_g("zero_mean", (1, 4, 8, 8), C, 1, 53)
    xg = x.cuda().requires_grad_(True)
    w1g, w2g = (t.clone().requires_grad_(True) for t in (w1, w2))
    t1 = pipeline.conv3d(xg, w1g, stride=1, pad=1, precision=prec)
    p = pipeline.max_pool3d(t1, precision=prec)
    y = pipeline.conv3d(p, w2g, stride=1, pad=1, precision=prec)
    t1.retain_grad()
    p.retain_grad()
    y.backward(gy.cuda())
    t1c, pc = t1.detach().cpu(), p.detach().cpu()
    gp_gpu, gt1_gpu = p.grad.cpu(), t1.grad.cpu()
    assert torch.equal(pc, F.max_pool3d(t1c, (1, 2, 2)))
    # the forward against float64, and the argmax: a disagreement only between candidates within their bounds of each other
    r1 = eb.conv_ref64(x, w1, pad=1)
    eb.check_elementwise(t1c, r1, prec, "t1")
    _, i_gpu = F.max_pool3d(t1c.double(), (1, 2, 2), return_indices=True)
    v64, i_64 = F.max_pool3d(r1.ref, (1, 2, 2), return_indices=True)
    flat, fb = r1.ref.flatten(2), r1.bound(prec).flatten(2)      # the indices count within a channel's (N, H, W)
    differ = i_gpu != i_64
    gap = (v64 - flat.gather(2, i_gpu.flatten(2)).reshape(v64.shape)).abs()
    room = (fb.gather(2, i_gpu.flatten(2)) + fb.gather(2, i_64.flatten(2))).reshape(v64.shape)
    assert bool((gap[differ] <= room[differ]).all())
    share = float(differ.double().mean())
    print("autograd conv -> max pool -> conv: the float64 argmax differs in %.2f %% of the windows" % (100 * share))
    assert share < 0.02
    # stage 1, the second conv at the GPU's p
    gy64 = gy.double()
    gp64, gw2_64 = cg.grads64(pc, w2, gy64, "k333")
    Ep = cg.dgrad_ref64(w2, gy, "k333").bound(prec)
    bw2 = cg.wgrad_ref64(pc, gy, "k333", tuple(w2.shape)).bound(prec)
    ok, wp = _le(gp_gpu, gp64, Ep)
    assert ok, wp
    # stage 2, the pool at the GPU's argmax: a selection of record values, exact on what it was handed
    route = lambda t: torch.autograd.grad(F.max_pool3d(t1d, (1, 2, 2)), t1d, t)[0]
    t1d = t1c.double().requires_grad_(True)
    gt1_64, Et1 = route(gp64), route(Ep)
    assert torch.equal(gt1_gpu.double(), route(gp_gpu.double()))
    keep = pg.up((~differ).double(), 2) > 0
    ok, wt = _le(torch.where(keep, gt1_gpu.double(), gt1_64), gt1_64, Et1)
    assert ok, wt
    # stage 3, the first conv at x
    gx64, gw1_64 = cg.grads64(x, w1, gt1_64, "k333")
    wa, kw = cg.adjoint_conv(w1, "k333")
    Ex = cg.dgrad_ref64(w1, gt1_gpu, "k333").bound(prec) + eb.conv_ref64(Et1, wa.abs(), **kw).ref
    bw1 = cg.wgrad_ref64(x, gt1_gpu, "k333", tuple(w1.shape)).bound(prec) + cg.wgrad_ref64(x.abs(), Et1, "k333", tuple(w1.shape)).ref
    worst = {"p.grad": wp, "t1.grad": wt}
    for name, (got, ref, bound) in {"x.grad": (xg.grad, gx64, Ex), "w1.grad": (w1g.grad, gw1_64, bw1), "w2.grad": (w2g.grad, gw2_64, bw2)}.items():
        ok, worst[name] = _le(got, ref, bound)
        assert ok, (name, worst[name])
    print("autograd conv -> max pool -> conv: err/bound " + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert xg.grad.is_cuda and float(xg.grad.abs().max()) > 0 and float(w1g.grad.abs().max()) > 0
    assert int((gt1_gpu != 0).sum()) <= gp_gpu.numel()


def test_autograd_pyramid_three_convs(eng):
    """pipeline.avg_pool_pyramid -> one pipeline.conv3d (1x1x1) per level, their outputs contracted with three given gradients and summed, at
    (1, 4, 16, 16), 8 channels, split-bf16: x.grad against the float64 graph evaluated from the GPU's pooled volumes;
    the convs' bounds at the gradients the GPU handed them, carried through the pyramid's adjoint with absolute values, plus the pyramid's own."""
    from dffinthewild_amd import pipeline
    prec, C, shape = "bf16x3", 8, (1, 4, 16, 16)
    x = pg.make_g("zero_mean", shape, C, 1, 59)
    ws = [pw.make_case("zero_mean", "k111", 1, C, C, 4, 16 // k, 16 // k, 60 + k)[1] for k in (2, 4, 8)]
    gys = [pg.make_g("zero_mean", shape, C, k, 70 + k) for k in (2, 4, 8)]
    xg = x.cuda().requires_grad_(True)
    wg = [w.clone().requires_grad_(True) for w in ws]
    ps = pipeline.avg_pool_pyramid(xg, precision=prec)
    ys = [pipeline.conv3d(p, w, pad=0, precision=prec) for p, w in zip(ps, wg)]
    for p in ps:
        p.retain_grad()
    torch.autograd.backward(ys, [g.cuda() for g in gys])
    gp_gpu = [p.grad.cpu() for p in ps]
    g64, E, worst = [], [], {}
    for k, p, w, w_g, gy, gp in zip((2, 4, 8), ps, ws, wg, gys, gp_gpu):
        pc = p.detach().cpu()
        gp64, gw64 = pw.grads64(pc, w, gy.double(), "k111")
        Ek = pw.dgrad_ref64(w, gy, "k111").bound(prec)
        ok, worst["p%d.grad" % k] = _le(gp, gp64, Ek)
        assert ok, (k, worst)
        ok, worst["w%d.grad" % k] = _le(w_g.grad, gw64, pw.wgrad_ref64(pc, gy, "k111").bound(prec))
        assert ok, (k, worst)
        g64.append(gp64)
        E.append(Ek)
    # the pyramid's adjoint at the float64 gradients; its own bound at the gradients the GPU handed it, theirs carried through with absolute values
    ref = sum(pg.up(g, k) / (k * k) for g, k in zip(g64, (2, 4, 8)))
    _, own = pg.pool3_ref64(gp_gpu[0], gp_gpu[1], gp_gpu[2], None, prec)
    bound = own + sum(pg.up(e, k) / (k * k) for e, k in zip(E, (2, 4, 8)))
    ok, worst["x.grad"] = _le(xg.grad, ref, bound)
    assert ok, worst
    print("autograd pyramid -> three convs: err/bound " + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert xg.grad.is_cuda and float(xg.grad.abs().max()) > 0
    # a level without a gradient counts as zeros: the result is the single level's
    xg.grad = None
    p2, p4, p8 = pipeline.avg_pool_pyramid(xg, precision=prec)
    p4.backward(gys[1].cuda())
    assert torch.equal(xg.grad, eng.op_pool_backward(gys[1].cuda(), k=4, mode="avg", precision=prec))
