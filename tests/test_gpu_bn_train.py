"""Train-mode BatchNorm3d on the GPU: every element of y, save_mean, save_invstd, both running statistics, grad_x, grad_res,
grad_gamma and grad_beta against the float64 reference under the bounds of tests/bn_ref.py; bit-identity between calls and on a forced small
grid; the constant channel; the launches; the refusals; conv -> BN(+skip, ReLU) -> conv -> HeadsLoss as one autograd graph.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 14 records them."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402
import conv_grad_ref as cg  # noqa: E402
import loss_ref as L  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = ((False, False), (True, False), (False, True), (True, True))   # (relu, residual)
PREC_ID = {"bf16x3": 0, "fp16": 1, "bf16": 2}
SMALL_GRID = 3   # index of the shape that runs with DFFW_BN_WGS=4


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def case(regime, C, si):
    return R.make_case(regime, C, R.SHAPES[si], R.case_seed(regime, C, si))


def run(eng, c, prec, relu, residual, need=("x", "params")):
    """Forward and backward through the op forms; returns the results keyed like bn_ref.QUANTITIES and the two launch lists."""
    x, gamma, beta = c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()
    rm, rv = c["rm0"].cuda().clone(), c["rv0"].cuda().clone()
    y, mean, invstd = eng.op_bn_train(x, gamma, beta, rm, rv, residual=c["res"].cuda() if residual else None, relu=relu, precision=prec)
    fwd = eng.op_kernels()
    gx, gres, dgamma, dbeta = eng.op_bn_train_backward(x, y, c["gy"].cuda(), gamma, mean, invstd, relu=relu, residual=residual, precision=prec, need=need)
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, gx=gx, gres=gres, dgamma=dgamma, dbeta=dbeta), fwd, eng.op_kernels()


def expected_kernels(prec, relu, residual):
    p, r, s = PREC_ID[prec], int(relu), int(residual)
    return (["dffw::bn_stats_kernel<%d>" % p, "dffw::bn_stats_finish_kernel", "dffw::bn_apply_kernel<%d, %d, %d>" % (p, r, s)],
            ["dffw::bn_bwd_reduce_kernel<%d, %d>" % (p, r), "dffw::bn_bwd_finish_kernel", "dffw::bn_bwd_apply_kernel<%d, %d, %d>" % (p, r, s)])


def check(eng, regime, C, si, prec, relu, residual):
    c = case(regime, C, si)
    got, fwd, bwd = run(eng, c, prec, relu, residual)
    assert (fwd, bwd) == expected_kernels(prec, relu, residual)
    r = R.reference(c, prec, relu, residual, y_stored=got["y"] if relu else None)
    n, ok = R.mask_disagreements(got["y"], r, prec) if relu else (0, True)
    q = R.ratios(got, r, prec)     # a NaN left by the poisoned workspace counts as inf
    print("bn_train %s %s C=%d %s relu=%d res=%d: masks differ at %d; err/bound %s" %
          (regime, prec, C, R.SHAPES[si], relu, residual, n, " ".join("%s %.3f" % kv for kv in q.items())))
    assert ok, "a ReLU mask differs from float64 where |z64| is above the forward bound"
    assert set(q) == set(R.QUANTITIES) - (set() if residual else {"gres"}) and max(q.values()) <= 1.0, q
    return got


@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("regime", R.REGIMES)
def test_every_element_under_its_bound(eng, regime, C, prec, monkeypatch):
    for si in range(len(R.SHAPES)):
        if si == SMALL_GRID:
            monkeypatch.setenv("DFFW_BN_WGS", "4")   # 8 workgroups: each walks 2 or 3 units
        for relu, residual in COMBOS:
            check(eng, regime, C, si, prec, relu, residual)


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_bit_identical_runs_and_small_grid(eng, prec, monkeypatch):
    """Two calls give identical bits; a grid forced small (DFFW_BN_WGS) is deterministic as well and stays under the bounds (its float64 sums differ in
    order only); without "x" in `need` only the parameter gradients are computed, with the same bits."""
    c = case("zero_mean", 32, 3)
    a, _, _ = run(eng, c, prec, True, True)
    b, _, _ = run(eng, c, prec, True, True)
    for k in R.QUANTITIES:
        assert torch.equal(a[k], b[k]), k
    p, _, bwd = run(eng, c, prec, True, True, need=("params",))
    assert p["gx"] is None and p["gres"] is None and torch.equal(p["dgamma"], a["dgamma"]) and torch.equal(p["dbeta"], a["dbeta"])
    assert bwd == expected_kernels(prec, True, True)[1][:2]
    monkeypatch.setenv("DFFW_BN_WGS", "4")
    s1, _, _ = run(eng, c, prec, True, True)
    s2, _, _ = run(eng, c, prec, True, True)
    for k in R.QUANTITIES:
        assert torch.equal(s1[k], s2[k]), k
    r = R.reference(c, prec, True, True, y_stored=s1["y"])
    q = R.ratios(s1, r, prec)
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_constant_channel_gives_the_rounded_beta_exactly(eng, prec):
    for C, si in ((8, 1), (64, 2)):
        c = case("constant", C, si)
        got, _, _ = run(eng, c, prec, False, False)
        k = R.const_channel(C)
        assert bool((got["y"][:, k].cpu() == R.rounded(c["beta"][k], prec)).all())
        assert float(got["mean"][k]) == R.CONST_VALUE


def test_refusals(eng):
    from dffinthewild_amd import pipeline
    v = lambda C: torch.ones(C, device="cuda")
    x = torch.zeros(1, 8, 2, 4, 4, device="cuda")
    with pytest.raises(ValueError):      # channels outside {8, 16, 32, 64, 128}
        eng.op_bn_train(torch.zeros(1, 24, 2, 4, 4, device="cuda"), v(24), v(24))
    with pytest.raises(ValueError):
        eng.op_bn_train(torch.zeros(1, 256, 1, 2, 2, device="cuda"), v(256), v(256))
    with pytest.raises(ValueError):      # one value per channel: PyTorch raises there
        eng.op_bn_train(torch.zeros(1, 8, 1, 1, 1, device="cuda"), v(8), v(8))
    with pytest.raises(ValueError):      # eps
        eng.op_bn_train(x, v(8), v(8), eps=0.0)
    with pytest.raises(ValueError):      # gamma of another length, a residual of another shape
        eng.op_bn_train(x, v(16), v(8))
    with pytest.raises(ValueError):
        eng.op_bn_train(x, v(8), v(8), residual=x[:, :, :1])
    with pytest.raises(KeyError):        # an unknown precision never reaches the library by name ...
        eng.op_bn_train(x, v(8), v(8), precision="fp8")
    rc = eng.lib.dffw_op_bn_train(0, 7, x.data_ptr(), 1, 8, 2, 4, 4, v(8).data_ptr(), v(8).data_ptr(), 1e-5, 0.1, None, None, None, 0, x.data_ptr(),
                                  v(8).data_ptr(), v(8).data_ptr(), None)
    assert rc == -1                      # ... and by number it is DFFW_EINVAL
    with pytest.raises(ValueError):
        eng.op_bn_train_backward(torch.zeros(1, 24, 2, 4, 4, device="cuda"), None, torch.zeros(1, 24, 2, 4, 4, device="cuda"), v(24), v(24), v(24))
    with pytest.raises(ValueError):      # the ReLU mask needs y
        eng.op_bn_train_backward(x, None, x, v(8), v(8), v(8), relu=True)
    # a short workspace of the record forms (Python never passes one): DFFW_ENOMEM, before any launch
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(32 * 2 * 8, dtype=torch.int16, device="cuda")
    need = eng.lib.dffw_bn_train_workspace_bytes(1, 8, 2, 4, 4)
    assert need == 8 * 2 * 8 * 8
    rc = eng.lib.dffw_bn_train_forward(0, 0, rec.data_ptr(), 1, 8, 2, 4, 4, v(8).data_ptr(), v(8).data_ptr(), 1e-5, 0.1, None, None, None, 0,
                                       rec.data_ptr(), v(8).data_ptr(), v(8).data_ptr(), ws.data_ptr(), need - 1, None)
    assert rc == -3 and eng.op_kernels() == []
    rc = eng.lib.dffw_bn_train_backward(0, 0, rec.data_ptr(), None, rec.data_ptr(), 1, 8, 2, 4, 4, v(8).data_ptr(), v(8).data_ptr(), v(8).data_ptr(), 0,
                                        rec.data_ptr(), None, v(8).data_ptr(), v(8).data_ptr(), ws.data_ptr(), need - 1, None)
    assert rc == -3
    assert eng.op_kernels() == []        # nothing was launched
    with pytest.raises(RuntimeError):    # CPU tensors: no fallback
        eng.op_bn_train(x.cpu(), v(8).cpu(), v(8).cpu())
    with pytest.raises(RuntimeError):
        pipeline.batch_norm3d(x.cpu(), v(8), v(8))


def test_autograd_conv_bn_conv_behind_heads_loss(eng):
    """pipeline.conv3d -> pipeline.batch_norm3d(relu, residual=skip) -> pipeline.conv3d -> HeadsLoss: every gradient against the float64 CPU graph
    evaluated from the GPU's own intermediates.  Each stage's own bound holds at the gradient the GPU handed it; the bound of that gradient is
    carried through the stage's adjoint with absolute values (E2: the loss kernel's, through conv 2's adjoint and weight-gradient contraction;
    Ea: that plus the rounding of the fp32 gradient to records, through the BatchNorm backward; E1: through conv 1's)."""
    from dffinthewild_amd import pipeline
    geom, prec, C = "k333", "bf16x3", 8
    u = R.U[prec]
    g = torch.Generator().manual_seed(11)
    x, w1, _ = cg.make_case("zero_mean", geom, 1, C, C, 4, 16, 16, 29)
    _, w2, _ = cg.make_case("zero_mean", geom, 1, C, C, 4, 16, 16, 31)
    skip = R.rounded(torch.randn(1, C, 4, 16, 16, generator=g), prec)       # already a record value: its rounding is no part of the graph
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5
    fd = 0.1 + 1.4 * torch.rand(1, 4, 1, 1, generator=g)
    gt = 0.1 + 1.4 * torch.rand(1, 16, 16, generator=g)
    mask = torch.rand(1, 16, 16, generator=g) < 0.7
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    xg, w1g, w2g = x.cuda().requires_grad_(True), w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    sg, gg, bg = skip.cuda().requires_grad_(True), gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    y1 = pipeline.conv3d(xg, w1g, stride=1, pad=1, precision=prec)
    a = pipeline.batch_norm3d(y1, gg, bg, rm, rv, residual=sg, relu=True, precision=prec)
    y2 = pipeline.conv3d(a, w2g, stride=1, pad=1, precision=prec)
    for t in (y1, a, y2):
        t.retain_grad()
    total = pipeline.HeadsLoss.apply(y2[:, 0], y2[:, 1], y2[:, 2], y2[:, 3], fd.cuda(), gt.cuda(), mask.cuda())
    total.backward()
    assert float(rm.abs().max()) > 0 and not torch.equal(rv, torch.ones_like(rv))      # the forward updated the running statistics in place
    y1c, ac, g2_gpu, ga_gpu, g1_gpu = y1.detach().cpu(), a.detach().cpu(), y2.grad.cpu(), a.grad.cpu(), y1.grad.cpu()
    wshape = tuple(w1.shape)
    # stage 1, the loss: its gradient at the GPU's score volumes
    lcase = dict(scores=[y2.detach()[:, k].cpu() for k in range(4)], fd=fd, gt=gt, mask=mask, conf=None, weights=list(L.WEIGHTS), rng=None)
    g2_64, E2 = torch.zeros_like(g2_gpu, dtype=torch.float64), torch.zeros_like(g2_gpu, dtype=torch.float64)
    for k, (gk, Gk) in enumerate(zip(L.reference(lcase)["grads"], L.bound(lcase))):
        g2_64[:, k], E2[:, k] = gk, L.ALPHA * Gk
    assert bool(((g2_gpu.double() - g2_64).abs() <= E2).all())
    # stage 2, conv 2 at the GPU's `a`
    ga_64, gw2_64 = cg.grads64(ac, w2, g2_64, geom)
    wa, kw = cg.adjoint_conv(w2, geom)
    Ea = cg.dgrad_ref64(w2, g2_gpu, geom).bound(prec) + eb.conv_ref64(E2, wa.abs(), **kw).ref
    bw2 = cg.wgrad_ref64(ac, g2_gpu, geom, wshape).bound(prec) + cg.wgrad_ref64(ac.abs(), E2, geom, wshape).ref
    assert bool(((ga_gpu.double() - ga_64).abs() <= Ea).all())
    # stage 3, BatchNorm at the GPU's y1, its stored output's mask and the gradient the GPU handed it (rounded to records on entry: u |ga|)
    zero = torch.zeros(C)
    bcase = dict(x=y1c, gamma=gamma, beta=beta, res=skip, gy=ga_gpu, rm0=zero, rv0=zero + 1)
    r = R.reference(bcase, prec, True, True, y_stored=ac)
    own = R.bounds(r, prec)
    r64 = R.reference(dict(bcase, gy=ga_64), None, True, True, y_stored=ac)
    dg = (ac > 0) * (Ea + u * ga_gpu.double().abs())
    M, xh, ch, cs = r["M"], r["xh"].abs(), R._ch, R._csum
    carried_gx = ch(r["gamma"].abs() * r["invstd"]) * (dg + ch(cs(dg)) / M + xh * ch(cs(dg * xh)) / M)
    E1 = own["gx"] + carried_gx
    checks = {"skip.grad": (sg.grad, r64["gres"], own["gres"] + dg), "gamma.grad": (gg.grad, r64["dgamma"], own["dgamma"] + cs(dg * xh)),
              "beta.grad": (bg.grad, r64["dbeta"], own["dbeta"] + cs(dg)), "y1.grad": (g1_gpu, r64["gx"], E1)}
    # stage 4, conv 1
    gx_64, gw1_64 = cg.grads64(x, w1, r64["gx"], geom)
    wa1, kw1 = cg.adjoint_conv(w1, geom)
    checks["x.grad"] = (xg.grad, gx_64, cg.dgrad_ref64(w1, g1_gpu, geom).bound(prec) + eb.conv_ref64(E1, wa1.abs(), **kw1).ref)
    checks["w1.grad"] = (w1g.grad, gw1_64, cg.wgrad_ref64(x, g1_gpu, geom, wshape).bound(prec) + cg.wgrad_ref64(x.abs(), E1, geom, wshape).ref)
    checks["w2.grad"] = (w2g.grad, gw2_64, bw2)
    worst = {}
    for name, (got, ref, bound) in checks.items():
        err = (got.detach().cpu().double() - ref).abs()
        worst[name] = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())   # (0 / 0 where a gradient is exactly zero)
        assert bool((err <= bound).all()), (name, worst[name])
    print("autograd conv -> BN -> conv -> HeadsLoss: err/bound " + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert float(sg.grad.abs().max()) > 0 and float(gg.grad.abs().max()) > 0 and float(xg.grad.abs().max()) > 0
