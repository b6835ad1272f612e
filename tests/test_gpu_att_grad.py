"""The fused backward of the attention tail on the GPU: every element of grad_x, grad_w3 and grad_w1 against the float64
formulas under the bounds of tests/att_grad_ref.py; integer data bit for bit on two grids; unit impulses at the sample boundary; shortened
flush intervals; the record form on a side stream between guards; the autograd node; the Feature_Extraction block in training mode against
the same block built from the nodes that existed before.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 27 is where the table of them goes."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import att_grad_ref as ag  # noqa: E402
import conv_grad_ref as cg  # noqa: E402
import pw_grad_ref as pw  # noqa: E402
from test_gpu_train_records import Guarded, PREC_ID, nbytes_records, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

CHANNELS = (8, 16, 32)
worst_seen = {}


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


@pytest.fixture(autouse=True)
def small_grid(monkeypatch):
    """8 workgroups: in the largest shape every workgroup walks two columns."""
    monkeypatch.setenv("DFFW_ATTGRAD_WGS", "8")
    monkeypatch.delenv("DFFW_ATTGRAD_FLUSH_STEPS", raising=False)


@functools.lru_cache(maxsize=None)
def case(regime, C, shape):
    B, N, H, W = shape
    return ag.make_case(regime, B, C, N, H, W, seed=23 + C + sum(shape))


def kernels(prec, C, finish=True):
    return ["dffw::att_tail_bwd_kernel<%d, %d>" % (PREC_ID[prec], C)] + (["dffw::att_tail_bwd_finish_kernel"] if finish else [])


def forward(eng, x, w3, w1, prec):
    y, a, t = eng.op_attention_tail(x.cuda(), w3, w1, precision=prec)
    return y.cpu(), a.cpu(), t.cpu()


def backward(eng, x, a, t, gy, w3, w1, prec, need=("x", "w")):
    got = eng.op_attention_tail_backward(x.cuda(), a.cuda(), t.cuda(), gy.cuda(), w3, w1, precision=prec, need=need)
    return tuple(g.cpu() if g is not None else None for g in got)


def check(eng, regime, C, shape, prec):
    x, w3, w1, gy = case(regime, C, shape)
    _, a, t = forward(eng, x, w3, w1, prec)
    got = backward(eng, x, a, t, gy, w3, w1, prec)
    assert eng.op_kernels() == kernels(prec, C)
    r = ag.ref64(x, a, t, gy, w3, w1, prec)
    for m in (r.mask_a, r.mask_t):     # each mask has both values
        assert 0 < int(m.sum()) < m.numel()
    rx, r3, r1 = ag.ratios(got, r)     # a NaN left by the poisoned workspace is an infinite ratio
    print("att_grad %s C=%d %s %s: err/bound grad_x %.3f grad_w3 %.3f grad_w1 %.3f" % (prec, C, shape, regime, rx, r3, r1))
    key = (prec, C)
    worst_seen[key] = tuple(max(p, q) for p, q in zip(worst_seen.get(key, (0.0, 0.0, 0.0)), (rx, r3, r1)))
    assert max(rx, r3, r1) <= 1.0, (prec, C, shape, regime, rx, r3, r1)
    if shape[1] == 1:     # no neighbouring slice: the outer taps' gradients are exactly 0
        assert float(got[1][:, :, 0].abs().max()) == 0.0 and float(got[1][:, :, 2].abs().max()) == 0.0
    return got


@pytest.mark.parametrize("prec", ag.PRECISIONS)
@pytest.mark.parametrize("C", CHANNELS)
def test_every_element_within_bound(eng, C, prec):
    for regime in ("zero_mean",) + (("post_relu", "offset") if C == 16 else ()):
        for shape in ag.SHAPES:
            check(eng, regime, C, shape, prec)
    print("att_grad worst %s C=%d: grad_x %.3f grad_w3 %.3f grad_w1 %.3f" % ((prec, C) + worst_seen[(prec, C)]))


def int_refs(eng, C, shape, prec="bf16x3"):
    """An integer case whose every intermediate and result a record holds exactly (asserted on the float64 reference), and the GPU forward's a, t."""
    B, N, H, W = shape
    x, w3, w1, gy = ag.int_case(B, C, N, H, W, seed=3 + C)
    _, a64, t64 = ag.forward64(x.double(), w3.double(), w1.double())
    gx, dw3, dw1, ga, gt = ag.formulas64(x.double(), a64, t64, gy.double(), w3.double(), w1.double())
    for v in (a64, t64, ga, gt, gx):
        assert ag.exact_in_record(v, prec)
    for v in (dw3, dw1):
        assert bool((v.float().double() == v).all()) and float(v.abs().max()) > 0
    _, a, t = forward(eng, x, w3, w1, prec)
    assert torch.equal(a.double(), a64) and torch.equal(t.double(), t64)
    return (x, a, t, gy, w3, w1), (gx, dw3, dw1)


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 2, 12, 20)])
@pytest.mark.parametrize("C", [8, 16])
def test_integer_data_is_exact_on_any_grid(eng, C, shape, monkeypatch):
    args, ref = int_refs(eng, C, shape)
    for wgs in ("8", None):
        if wgs is None:
            monkeypatch.delenv("DFFW_ATTGRAD_WGS")
        got = backward(eng, *args, "bf16x3")
        for g, r, name in zip(got, ref, ("grad_x", "grad_w3", "grad_w1")):
            assert torch.equal(g.double(), r), (name, wgs, int((g.double() != r).sum()))


@pytest.mark.parametrize("prec", ag.PRECISIONS)
@pytest.mark.parametrize("C", [8, 32])
def test_impulse(eng, C, prec):
    """grad_y = one unit impulse in the last channel, with w1's last row all ones so that ga = [a > 0]: grad_w1's last row is a's record at the
    impulse and grad_w3[co, :, kz] is [a_co > 0] times x's record one slice before, at and after it, bit for bit.  At sample 0's last slice and
    last pixel (in the ragged chunk) tap kz = 2 lies past the sample: exactly 0, not sample 1's first slice; at sample 1's slice 0, pixel 0,
    tap kz = 0 is exactly 0.  grad_x is nonzero only in the impulse's pixel column."""
    B, N, H, W = 2, 3, 12, 20
    g = torch.Generator().manual_seed(5 + C)
    x = pw.rounded(torch.randn(B, C, N, H, W, generator=g) + 0.01, prec)
    a, t = (pw.rounded(torch.relu(torch.randn(B, C, N, H, W, generator=g)), prec) for _ in range(2))
    w3, w1 = ag.filters(C, g)
    w1[C - 1] = 1.0
    assert float(x.abs().min()) > 0
    for (b, n, yy, xx), dead in (((0, N - 1, H - 1, W - 1), 2), ((1, 0, 0, 0), 0)):
        t[b, C - 1, n, yy, xx] = 1.0
        a[b, :C // 2, n, yy, xx] = 0.5
        gy = torch.zeros(B, C, N, H, W)
        gy[b, C - 1, n, yy, xx] = 1.0
        gx, dw3, dw1 = backward(eng, x, a, t, gy, w3, w1, prec)
        open_a = (a[b, :, n, yy, xx] > 0).float()
        assert 0 < int(open_a.sum()) <= C
        assert float(dw1[:C - 1].abs().max()) == 0.0 and torch.equal(dw1[C - 1, :, 0, 0, 0], a[b, :, n, yy, xx])
        assert float(dw3[:, :, dead].abs().max()) == 0.0
        for kz in (1, 2 - dead):
            assert torch.equal(dw3[:, :, kz, 0, 0], open_a[:, None] * x[b, :, n + kz - 1, yy, xx][None, :]), (b, kz)
        col = torch.zeros(B, 1, 1, H, W, dtype=torch.bool)
        col[b, 0, 0, yy, xx] = True
        assert float(gx.masked_fill(col, 0).abs().max()) == 0.0 and float(gx[b, :, :, yy, xx].abs().max()) > 0
        rx, _, _ = ag.ratios((gx, None, None), ag.ref64(x, a, t, gy, w3, w1, prec))
        assert rx <= 1.0, rx


def test_flush_boundaries(eng, monkeypatch):
    shape, C, steps = (2, 10, 32, 32), 8, 6
    B, N, H, W = shape
    assert ag.grid_x_of(B, H, W, wgs=8) == 8
    per_wg = ag.steps_per_workgroup(B, N, H, W, 8)
    assert min(per_wg) >= 3 * steps, per_wg     # every workgroup flushes at least three times
    x, w3, w1, gy = case("zero_mean", C, shape)
    args, ref = int_refs(eng, C, shape)
    whole = backward(eng, *args, "bf16x3")
    monkeypatch.setenv("DFFW_ATTGRAD_FLUSH_STEPS", str(steps))
    for prec in ag.PRECISIONS:
        _, a, t = forward(eng, x, w3, w1, prec)
        got = backward(eng, x, a, t, gy, w3, w1, prec)
        again = backward(eng, x, a, t, gy, w3, w1, prec)
        rs = ag.ratios(got, ag.ref64(x, a, t, gy, w3, w1, prec))
        print("att_grad flush every %d steps %s C=%d %s: err/bound %.3f %.3f %.3f" % ((steps, prec, C, shape) + tuple(rs)))
        assert max(rs) <= 1.0, rs
        assert all(torch.equal(p, q) for p, q in zip(got, again))
    short = backward(eng, *args, "bf16x3")
    for p, q, r in zip(short, whole, ref):
        assert torch.equal(p, q) and torch.equal(p.double(), r)


REC_SHAPE = (2, 3, 12, 20)


def run_records(eng, prec, C, c, fill, alias=False, short=0):
    """dffw_att_tail_backward on caller-built records on a side stream, every written buffer between guards; one synchronisation."""
    lib, dev, Pn = eng.lib, torch.cuda.current_device(), PREC_ID[prec]
    B, N, H, W = REC_SHAPE
    rec = {n: cg.to_records(c[n], prec).cuda() for n in ("x", "a", "t", "gy")}
    w3d, w1d = c["w3"].cuda().contiguous(), c["w1"].cuda().contiguous()
    wsb = lib.dffw_att_tail_backward_workspace_bytes(B, C, N, H, W)
    assert wsb > 0
    nrec = nbytes_records(prec, B, C, N, H, W)
    G = Guarded(dict(gx=nrec, ws=wsb, gw3=4 * 3 * C * C, gw1=4 * C * C))
    G.raw("ws").fill_(fill)
    if alias:     # grad_y's records live in the guarded output buffer: grad_x aliases grad_y
        G.raw("gx").copy_(rec["gy"].reshape(-1).view(torch.uint8))
    gy_ptr = G.ptr("gx") if alias else rec["gy"].data_ptr()
    stream, sp = side_stream()
    rc = lib.dffw_att_tail_backward(dev, Pn, rec["x"].data_ptr(), rec["a"].data_ptr(), rec["t"].data_ptr(), gy_ptr, B, C, N, H, W, w3d.data_ptr(),
                                    w1d.data_ptr(), G.ptr("gx"), G.ptr("gw3"), G.ptr("gw1"), G.ptr("ws"), wsb - short, sp)
    names = eng.op_kernels()
    stream.synchronize()      # the only host synchronisation
    G.check()
    if short:
        assert rc == -3 and names == [], rc     # DFFW_ENOMEM, and nothing was written
        assert bool((G.buf == 0xFF).all()) or alias or fill != 0xFF
        return None
    assert rc == 0, lib.dffw_last_error().decode()
    assert names == kernels(prec, C), names
    parts = 2 if prec == "bf16x3" else 1
    return (cg.from_records(G.view("gx", torch.int16, (B, N, H, W, parts, C)).cpu().clone(), prec, C),
            G.view("gw3", torch.float32, (C, C, 3, 1, 1)).cpu().clone(), G.view("gw1", torch.float32, (C, C, 1, 1, 1)).cpu().clone())


@pytest.mark.parametrize("prec", ag.PRECISIONS)
@pytest.mark.parametrize("C", [8, 32])
def test_record_chain(eng, C, prec):
    B, N, H, W = REC_SHAPE
    g = torch.Generator().manual_seed(61 + C)
    rd = lambda: pw.rounded(torch.randn(B, C, N, H, W, generator=g), prec)
    w3, w1 = ag.filters(C, g)
    c = dict(x=rd(), a=torch.relu(rd()), t=torch.relu(rd()), gy=rd(), w3=w3, w1=w1)     # record values: staging them again gives the same records
    base = run_records(eng, prec, C, c, 0xFF)
    for other in (run_records(eng, prec, C, c, 0x00), run_records(eng, prec, C, c, 0xFF, alias=True)):
        assert all(torch.equal(p, q) for p, q in zip(base, other))
    op = backward(eng, c["x"], c["a"], c["t"], c["gy"], w3, w1, prec)
    assert all(torch.equal(p, q) for p, q in zip(base, op))
    rs = ag.ratios(base, ag.ref64(c["x"], c["a"], c["t"], c["gy"], w3, w1, prec))
    print("att_grad record form %s C=%d %s: err/bound %.3f %.3f %.3f" % ((prec, C, REC_SHAPE) + tuple(rs)))
    assert max(rs) <= 1.0, rs
    assert run_records(eng, prec, C, c, 0xFF, short=1) is None


@pytest.mark.parametrize("C", [8, 32])
def test_autograd_node(eng, C):
    from dffinthewild_amd import pipeline
    B, N, H, W = 1, 4, 16, 16
    x0, w3, w1, gy = ag.make_case("zero_mean", B, C, N, H, W, seed=7 + C)
    x = x0.cuda().requires_grad_(True)
    w3c, w1g = w3.clone().requires_grad_(True), w1.cuda().requires_grad_(True)     # one filter on the CPU, one on the GPU
    y = pipeline.attention_tail(x, w3c, w1g)
    a = eng.op_conv3d(x0.cuda(), w3, pad=(1, 0, 0), relu=1)
    t = eng.op_conv3d(a, w1, relu=1)
    assert torch.equal(y.detach(), x0.cuda() + t)
    y.backward(gy.cuda())
    want = eng.op_attention_tail_backward(x0.cuda(), a, t, gy.cuda(), w3, w1)
    assert torch.equal(x.grad, want[0]) and torch.equal(w3c.grad, want[1].cpu()) and torch.equal(w1g.grad, want[2])
    assert w3c.grad.device.type == "cpu" and w1g.grad.device.type == "cuda"
    only_x = eng.op_attention_tail_backward(x0.cuda(), a, t, gy.cuda(), w3, w1, need=("x",))
    assert eng.op_kernels() == kernels("bf16x3", C, finish=False)     # no finish kernel without "w"
    assert only_x[1] is None and only_x[2] is None and torch.equal(only_x[0], want[0])
    xg = x0.cuda().requires_grad_(True)
    pipeline.attention_tail(xg, w3, w1).backward(gy.cuda())     # filters that need no gradient
    assert eng.op_kernels() == kernels("bf16x3", C, finish=False) and torch.equal(xg.grad, want[0])


KEYS = ("Focus_Measure.conv.0.0.weight", "Focus_Measure.conv.0.1.weight", "Focus_Measure.conv.0.1.bias", "Focus_Measure.conv.2.0.weight",
        "Focus_Measure.conv.2.1.weight", "Focus_Measure.conv.2.1.bias", "N_ch_attention.0.weight", "N_ch_attention.2.weight")
STATS = ("Focus_Measure.conv.0.1.running_mean", "Focus_Measure.conv.0.1.running_var", "Focus_Measure.conv.2.1.running_mean",
         "Focus_Measure.conv.2.1.running_var")


def block_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    w3, w1 = ag.filters(C, g)
    p = {KEYS[0]: u(C, C, 1, 3, 3) * (2.0 / (9 * C)) ** 0.5 * 1.7, KEYS[1]: 1 + 0.3 * u(C), KEYS[2]: 0.2 * u(C),
         KEYS[3]: u(C, C, 1, 3, 3) * (2.0 / (9 * C)) ** 0.5 * 1.7, KEYS[4]: 1 + 0.3 * u(C), KEYS[5]: 0.2 * u(C), KEYS[6]: w3, KEYS[7]: w1}
    for k in STATS:
        p[k] = torch.zeros(C) if k.endswith("mean") else torch.ones(C)
    return p


def block64(x, p, momentum=0.1):
    """The block in float64 with torch functional ops (train-mode batch_norm updates the running statistics it is given)."""
    bn = lambda v, k: F.batch_norm(v, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], True, momentum, 1e-5)
    h = F.relu(bn(F.conv3d(x, p[KEYS[0]], None, 1, (0, 1, 1)), "Focus_Measure.conv.0.1"))
    h = F.relu(bn(F.conv3d(h, p[KEYS[3]], None, 1, (0, 1, 1)), "Focus_Measure.conv.2.1") + x)
    return ag.forward64(h, p[KEYS[6]], p[KEYS[7]])[0]


def block_existing(pipeline, x, p, precision, momentum=0.1):
    """The same block out of the nodes that existed before this section: the tail as conv3d -> relu -> conv3d -> relu -> +."""
    bn = lambda v, k, **kw: pipeline.batch_norm3d(v, p[k + ".weight"], p[k + ".bias"], p[k + ".running_mean"], p[k + ".running_var"],
                                                  momentum=momentum, precision=precision, **kw)
    h = bn(pipeline.conv3d(x, p[KEYS[0]], pad=(0, 1, 1), precision=precision), "Focus_Measure.conv.0.1", relu=True)
    h = bn(pipeline.conv3d(h, p[KEYS[3]], pad=(0, 1, 1), precision=precision), "Focus_Measure.conv.2.1", residual=x, relu=True)
    a = torch.relu(pipeline.conv3d(h, p[KEYS[6]], pad=(1, 0, 0), precision=precision))
    return h + torch.relu(pipeline.conv3d(a, p[KEYS[7]], precision=precision))


def rel(got, ref):
    return float((got.detach().cpu().double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("C", [8, 16])
def test_feature_extraction_block(eng, C):
    from dffinthewild_amd import pipeline
    prec, (B, N, H, W) = "bf16x3", (2, 3, 16, 16)
    g = torch.Generator().manual_seed(11 + C)
    x0 = torch.randn(B, C, N, H, W, generator=g)
    lin = torch.randn(B, C, N, H, W, generator=g)     # the loss: a fixed random linear functional of the output
    p0 = block_params(C, 19 + C)
    p64 = {k: v.double().clone().requires_grad_(k in KEYS) for k, v in p0.items()}
    x64 = x0.double().requires_grad_(True)
    y64 = block64(x64, p64)
    (y64 * lin.double()).sum().backward()
    cols = []
    for build in (lambda x, p: pipeline.feature_extraction(x, p, precision=prec), lambda x, p: block_existing(pipeline, x, p, prec)):
        p = {k: v.cuda().clone().requires_grad_(k in KEYS) for k, v in p0.items()}
        x = x0.cuda().requires_grad_(True)
        y = build(x, p)
        (y * lin.cuda()).sum().backward()
        figures = {"y": rel(y, y64.detach()), "grad x": rel(x.grad, x64.grad)}
        figures.update({k: rel(p[k], p64[k].detach()) for k in STATS})
        figures.update({"grad " + k: rel(p[k].grad, p64[k].grad) for k in KEYS})
        cols.append((figures, y.detach(), {k: p[k].detach() for k in STATS}))
    (new, y_new, s_new), (old, y_old, s_old) = cols
    assert torch.equal(y_new, y_old) and all(torch.equal(s_new[k], s_old[k]) for k in STATS)     # the forward is the same chain
    for k in new:
        print("feature_extraction C=%d %-52s rel-L2 fused %.3e existing %.3e" % (C, k, new[k], old[k]))
    for k in new:
        assert new[k] <= max(2 * old[k], pw.U[prec]), (k, new[k], old[k])
