"""Backward of the 3x1x1 / 1x1x1 convs and the gradient mask-and-add on the GPU: every element of grad_x and grad_w against
float64 CPU autograd under the bounds of tests/pw_grad_ref.py; the exact unit impulse at the sample boundary; bit-identity between calls and
grids; one full-length fp32 partial per wave on the hardware; the refusals; the record forms on a side stream between guards; the autograd
chain of one attention tail behind HeadsLoss.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 15 is where the table of them goes."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_grad_ref as cg  # noqa: E402
import loss_ref as L  # noqa: E402
import pw_grad_ref as pw  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402
from test_gpu_train_records import Guarded, PREC_ID, i3, nbytes_records, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, N, H, W): a plane smaller than one chunk; N = 1 (the outer k311 taps' gradients are exactly 0); 240 pixels = one full + one ragged chunk, B > 1;
# three full chunks; several columns per workgroup (run with DFFW_PWGRAD_WGS=8)
SHAPES = [(2, 3, 8, 8), (1, 1, 8, 8), (2, 2, 12, 20), (1, 5, 16, 24), (2, 10, 32, 32)]
SMALL_GRID = (2, 10, 32, 32)
# (Cin, Cout): the square pairs the network uses, two rectangular ones, the ragged ones (half-filled last tile of g, f tails of 8 and 24 channels)
PAIRS = [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 32), (32, 16), (24, 40), (40, 24), (104, 56)]
GEOMS = list(pw.GEOMETRIES)
worst_seen = {}


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def case(geom, cin, cout, shape, regime="zero_mean"):
    """One case and its float64 references, computed once and shared by the precisions."""
    B, N, H, W = shape
    x, w, gy = pw.make_case(regime, geom, B, cin, cout, N, H, W, seed=17 + cin + 3 * cout)
    return x, w, gy, pw.dgrad_ref64(w, gy, geom), pw.wgrad_ref64(x, gy, geom)


def run(eng, geom, x, w, gy, prec, need=("x", "w")):
    return eng.op_conv_pw_backward(x.cuda(), w, gy.cuda(), pad=pw.GEOMETRIES[geom][1], precision=prec, need=need)


def wgrad_kernels(geom, prec):
    return ["dffw::conv_pw_wgrad_kernel<%d, %d>" % (PREC_ID[prec], pw.GEOMETRIES[geom][0][0]), "dffw::conv_pw_wgrad_finish_kernel"]


def check(eng, geom, cin, cout, shape, prec, regime="zero_mean"):
    x, w, gy, rx, rw = case(geom, cin, cout, shape, regime)
    gx, gw = run(eng, geom, x, w, gy, prec)
    assert eng.op_kernels() == wgrad_kernels(geom, prec)
    assert tuple(gw.shape) == pw.weight_shape(geom, cin, cout)
    # a NaN left by the poisoned workspace fails either check
    wx = eb.check_elementwise(gx, rx, prec, "grad_x %s %d->%d %s" % (geom, cin, cout, shape))
    ww = eb.check_elementwise(gw, rw, prec, "grad_w %s %d->%d %s" % (geom, cin, cout, shape))
    print("pw_grad %s %s %d->%d %s %s: grad_x err/bound %.3f (%s), grad_w %.3f" % (geom, prec, cin, cout, shape, regime, wx, eng.last_conv_kernel(), ww))
    key = (geom, prec)
    worst_seen[key] = tuple(max(a, b) for a, b in zip(worst_seen.get(key, (0.0, 0.0)), (wx, ww)))
    return gx, gw


def check_all_shapes(eng, monkeypatch, geom, cin, cout, prec, regime="zero_mean"):
    for shape in SHAPES:
        if shape == SMALL_GRID:   # 16 columns on 8 workgroups: every workgroup walks two
            monkeypatch.setenv("DFFW_PWGRAD_WGS", "8")
        gx, gw = check(eng, geom, cin, cout, shape, prec, regime)
        if shape[1] == 1 and geom == "k311":   # no neighbouring slice: the outer taps' gradients are exactly 0
            assert float(gw[:, :, 0].abs().max()) == 0.0 and float(gw[:, :, 2].abs().max()) == 0.0
    print("pw_grad worst so far %s %s: grad_x %.3f grad_w %.3f" % ((geom, prec) + worst_seen[(geom, prec)]))


@pytest.mark.parametrize("prec", pw.PRECISIONS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dto%d" % p)
@pytest.mark.parametrize("geom", GEOMS)
def test_every_element_under_its_bound(eng, geom, pair, prec, monkeypatch):
    check_all_shapes(eng, monkeypatch, geom, pair[0], pair[1], prec)


@pytest.mark.parametrize("regime", ["post_relu", "offset"])
@pytest.mark.parametrize("geom", GEOMS)
def test_regimes(eng, geom, regime, monkeypatch):
    """(zero_mean at 16 -> 16 is a case of test_every_element_under_its_bound)"""
    for prec in pw.PRECISIONS:
        check_all_shapes(eng, monkeypatch, geom, 16, 16, prec, regime)


@pytest.mark.parametrize("prec", pw.PRECISIONS)
@pytest.mark.parametrize("pair", [(8, 8), (24, 40), (40, 24)], ids=lambda p: "%dto%d" % p)
def test_unit_impulse_at_the_sample_boundary(eng, pair, prec):
    """grad_y = one unit impulse in the last channel: every grad_w element is ONE product 1 * x, the record-rounded x value it names, bit for bit.
    At sample 0's last slice and last pixel (in the ragged chunk) tap kz = 2 lies past the sample: exactly 0, not sample 1's first slice.  At
    sample 1's slice 0, pixel 0, tap kz = 0 is exactly 0, not sample 0's last slice."""
    cin, cout = pair
    B, N, H, W = 2, 3, 12, 20
    x, w, _ = pw.make_case("zero_mean", "k311", B, cin, cout, N, H, W, seed=5 + cin)
    xr = pw.rounded(x, prec)
    for geom in GEOMS:
        for (b, n, yy, xx), dead in (((0, N - 1, H - 1, W - 1), 2), ((1, 0, 0, 0), 0)):
            gy = torch.zeros(B, cout, N, H, W)
            gy[b, cout - 1, n, yy, xx] = 1.0
            wz = torch.zeros(pw.weight_shape(geom, cin, cout))
            _, gw = run(eng, geom, x, wz, gy, prec, need=("w",))
            want = pw.wgrad_ref64(xr, gy, geom).ref
            assert torch.equal(gw.cpu().double(), want), (geom, b, int((gw.cpu().double() != want).sum()))
            assert float(want[:cout - 1].abs().max()) == 0.0 and float(want[cout - 1].abs().max()) > 0
            if geom == "k311":
                assert float(gw[:, :, dead].abs().max()) == 0.0
                assert torch.equal(gw[cout - 1, :, 1, 0, 0].cpu(), xr[b, :, n, yy, xx])
                live = 2 - dead
                assert torch.equal(gw[cout - 1, :, live, 0, 0].cpu(), xr[b, :, n + live - 1, yy, xx])


@pytest.mark.parametrize("prec", pw.PRECISIONS)
@pytest.mark.parametrize("geom", GEOMS)
def test_bit_identical_runs_and_grids(eng, geom, prec, monkeypatch):
    """Two calls give identical bits.  With small-integer data (exact in every format and order) the result equals float64 autograd bit for bit at
    the default grid and with DFFW_PWGRAD_WGS=8 (every workgroup walks several columns) and a short flush interval."""
    x, w, gy, _, _ = case(geom, 16, 32, SHAPES[3])
    gx, gw = run(eng, geom, x, w, gy, prec)
    gx2, gw2 = run(eng, geom, x, w, gy, prec)
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2)
    only_x, none_w = run(eng, geom, x, w, gy, prec, need=("x",))
    assert none_w is None and torch.equal(only_x, gx) and eng.op_kernels() == []
    B, N, H, W = SMALL_GRID
    xi, wi, gi = pw.int_case(geom, B, 24, 40, N, H, W, 3)
    ref = pw.grads64(xi, wi, gi, geom)[1]
    _, got = run(eng, geom, xi, wi, gi, prec, need=("w",))
    assert torch.equal(got.cpu().double(), ref)
    monkeypatch.setenv("DFFW_PWGRAD_WGS", "8")
    monkeypatch.setenv("DFFW_PWGRAD_FLUSH_STEPS", "3")
    _, small = run(eng, geom, xi, wi, gi, prec, need=("w",))
    assert torch.equal(small.cpu().double(), ref)
    _, s1 = run(eng, geom, x, w, gy, prec, need=("w",))
    _, s2 = run(eng, geom, x, w, gy, prec, need=("w",))
    assert torch.equal(s1, s2)


FULL = (1, 10, 256, 256)   # 512 columns: 64 per workgroup of a grid of 8, 640 steps each


@functools.lru_cache(maxsize=None)
def full_case(geom):
    B, N, H, W = FULL
    x, w, gy = pw.make_case("offset", geom, B, 8, 8, N, H, W, 41)
    return x, w, gy, pw.wgrad_ref64(x, gy, geom)


@pytest.mark.parametrize("geom", GEOMS)
def test_full_length_partials(eng, geom, monkeypatch):
    """The one new term of the ALPHA * G bound, the fp32 accumulation over pixels, at its full length on the hardware: 8 -> 8 channels, split-bf16,
    offset inputs (the regime that grew in section 13).  On 8 workgroups (DFFW_PWGRAD_WGS=8, the flush interval at its default) every workgroup walks
    640 steps, so every wave sums a whole 512-step partial (16 384 pixels), flushes it and starts a second.  tests/test_pw_grad.py holds the CPU
    emulation of the same volume under 0.5; DESIGN.md section 15 has both figures."""
    B, N, H, W = FULL
    assert B * N * H * W <= 2 ** 20
    assert pw.grid_x_of(B, H, W, 8, 8, wgs=8) == 8
    steps = pw.steps_per_workgroup(B, N, H, W, 8)
    assert len(steps) == 8 and min(steps) > pw.FLUSH_STEPS, steps
    monkeypatch.setenv("DFFW_PWGRAD_WGS", "8")
    monkeypatch.delenv("DFFW_PWGRAD_FLUSH_STEPS", raising=False)
    x, w, gy, rw = full_case(geom)
    _, gw = run(eng, geom, x, w, gy, "bf16x3", need=("w",))
    _, gw2 = run(eng, geom, x, w, gy, "bf16x3", need=("w",))
    worst, _ = eb.elementwise_ratio(gw, rw, "bf16x3")
    print("pw_grad full-length partials %s bf16x3 offset 8->8 %s: grad_w err/bound %.3f" % (geom, FULL, worst))
    eb.check_elementwise(gw, rw, "bf16x3", "grad_w %s at full-length partials" % geom)
    assert torch.equal(gw, gw2)


def test_refusals(eng):
    x = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    w = torch.zeros(8, 8, 3, 1, 1)
    gy = torch.zeros(1, 8, 2, 8, 8, device="cuda")
    ok = dict(pad=(1, 0, 0))
    with pytest.raises(ValueError):      # in-plane taps
        eng.op_conv_pw_backward(x, torch.zeros(8, 8, 3, 3, 3), gy, pad=1)
    with pytest.raises(ValueError):
        eng.op_conv_pw_backward(x, torch.zeros(8, 8, 1, 3, 3), gy, pad=(0, 1, 1))
    with pytest.raises(ValueError):      # stride 2
        eng.op_conv_pw_backward(x, w, gy, stride=(1, 2, 2), **ok)
    with pytest.raises(ValueError):      # k311 with pad 0, k111 with a padding, an in-plane padding
        eng.op_conv_pw_backward(x, w, gy, pad=0)
    with pytest.raises(ValueError):
        eng.op_conv_pw_backward(x, torch.zeros(8, 8, 1, 1, 1), gy, pad=(1, 0, 0))
    with pytest.raises(ValueError):
        eng.op_conv_pw_backward(x, w, gy, pad=(1, 1, 1))
    with pytest.raises(ValueError):      # dilation
        eng.op_conv_pw_backward(x, w, gy, dilation=2, **ok)
    with pytest.raises(ValueError):      # channels: not a multiple of 8, above 128
        eng.op_conv_pw_backward(x[:, :4].contiguous(), w[:, :4].contiguous(), gy, **ok)
    with pytest.raises(ValueError):
        eng.op_conv_pw_backward(torch.zeros(1, 136, 2, 8, 8, device="cuda"), torch.zeros(8, 136, 3, 1, 1), gy, **ok)
    with pytest.raises(ValueError):
        eng.op_conv_pw_backward(x, torch.zeros(136, 8, 3, 1, 1), torch.zeros(1, 136, 2, 8, 8, device="cuda"), **ok)
    with pytest.raises(ValueError):      # grad_y of another shape
        eng.op_conv_pw_backward(x, w, gy[:, :, :, :4].contiguous(), **ok)
    with pytest.raises(RuntimeError):    # CPU tensors: no fallback
        eng.op_conv_pw_backward(x.cpu(), w, gy.cpu(), **ok)
    with pytest.raises(ValueError):      # grad_combine: a copy is no operation; channels; shapes
        eng.op_grad_combine(x)
    with pytest.raises(ValueError):
        eng.op_grad_combine(x[:, :4].contiguous(), y=x[:, :4].contiguous())
    with pytest.raises(ValueError):
        eng.op_grad_combine(x, y=gy[:, :, :1].contiguous())
    with pytest.raises(RuntimeError):
        eng.op_grad_combine(x.cpu(), y=x.cpu())
    assert eng.op_kernels() == []        # nothing was launched
    # the record forms: refused arguments size no workspace; a short workspace is DFFW_ENOMEM, before any launch
    lib = eng.lib
    assert lib.dffw_conv_pw_wgrad_workspace_bytes(1, 8, 2, 8, 8, 8, i3((3, 3, 3)), i3((1, 1, 1))) == 0
    assert lib.dffw_conv_pw_wgrad_workspace_bytes(1, 8, 2, 8, 8, 12, i3((3, 1, 1)), i3((1, 0, 0))) == 0
    wsb = lib.dffw_conv_pw_wgrad_workspace_bytes(1, 8, 2, 8, 8, 8, i3((3, 1, 1)), i3((1, 0, 0)))
    assert wsb > 0
    rec = torch.zeros(1 * 2 * 8 * 8 * 2 * 8, dtype=torch.int16, device="cuda")
    buf = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    gw = torch.zeros(8 * 8 * 3, device="cuda")
    dev = torch.cuda.current_device()
    rc = lib.dffw_conv_pw_wgrad(dev, 0, rec.data_ptr(), 1, 8, 2, 8, 8, rec.data_ptr(), 8, i3((3, 1, 1)), i3((1, 0, 0)), gw.data_ptr(), buf.data_ptr(), wsb - 8, None)
    assert rc == -3 and eng.op_kernels() == [], rc     # DFFW_ENOMEM
    rc = lib.dffw_grad_combine(dev, 0, rec.data_ptr(), None, None, 1, 8, 2, 8, 8, rec.data_ptr(), None)
    assert rc == -1 and eng.op_kernels() == [], rc


# ---- the record forms, as a training step calls them ------------------------------------------------------------------------------------------
REC_SHAPE = (2, 3, 12, 20)


def record_inputs(prec, C):
    """fp32 CPU tensors that ARE record values, so that staging them again gives the same records."""
    B, N, H, W = REC_SHAPE
    g = torch.Generator().manual_seed(61 + C)
    rd = lambda: pw.rounded(torch.randn(B, C, N, H, W, generator=g), prec)
    c = dict(a1=torch.relu(rd()), a2=torch.relu(rd()), gy=rd(), gb=rd())
    for t in c.values():
        assert torch.equal(pw.rounded(t, prec), t)
    return c


def run_record_chain(eng, prec, C, c, fill):
    """dffw_grad_combine(gy, y = a2) -> dffw_conv_pw_wgrad(k111, x = a1, grad_y = the records just written) -> dffw_grad_combine(those, b = gb, out
    aliasing b), enqueued back to back on one side stream; one host synchronisation at the end."""
    lib, dev, Pn = eng.lib, torch.cuda.current_device(), PREC_ID[prec]
    B, N, H, W = REC_SHAPE
    k, p = pw.GEOMETRIES["k111"]
    rec = {n: cg.to_records(c[n], prec).cuda() for n in ("a1", "a2", "gy", "gb")}
    wsb = lib.dffw_conv_pw_wgrad_workspace_bytes(B, C, N, H, W, C, i3(k), i3(p))
    assert wsb > 0
    nrec = nbytes_records(prec, B, C, N, H, W)
    G = Guarded(dict(g2=nrec, sum=nrec, ws=wsb, gw=4 * C * C))
    G.raw("ws").fill_(fill)
    G.raw("sum").copy_(rec["gb"].reshape(-1).view(torch.uint8))      # b's records live in the guarded buffer: out aliases b
    stream, sp = side_stream()
    names = []
    rc = lib.dffw_grad_combine(dev, Pn, rec["gy"].data_ptr(), rec["a2"].data_ptr(), None, B, C, N, H, W, G.ptr("g2"), sp)
    assert rc == 0, lib.dffw_last_error().decode()
    names.append(eng.op_kernels())
    rc = lib.dffw_conv_pw_wgrad(dev, Pn, rec["a1"].data_ptr(), B, C, N, H, W, G.ptr("g2"), C, i3(k), i3(p), G.ptr("gw"), G.ptr("ws"), wsb, sp)
    assert rc == 0, lib.dffw_last_error().decode()
    names.append(eng.op_kernels())
    rc = lib.dffw_grad_combine(dev, Pn, G.ptr("g2"), None, G.ptr("sum"), B, C, N, H, W, G.ptr("sum"), sp)
    assert rc == 0, lib.dffw_last_error().decode()
    names.append(eng.op_kernels())
    stream.synchronize()      # the only host synchronisation
    G.check()
    assert names == [["dffw::grad_combine_kernel<%d, 1, 0>" % Pn], wgrad_kernels("k111", prec), ["dffw::grad_combine_kernel<%d, 0, 1>" % Pn]], names
    parts = 2 if prec == "bf16x3" else 1
    records = lambda n: G.view(n, torch.int16, (B, N, H, W, parts, C)).cpu().clone()
    return dict(g2_records=records("g2"), sum_records=records("sum"), gw=G.view("gw", torch.float32, (C, C, 1, 1, 1)).cpu().clone(),
                gy_records=rec["gy"].cpu())


@pytest.mark.parametrize("prec", pw.PRECISIONS)
@pytest.mark.parametrize("C", [8, 16])
def test_record_chain(eng, C, prec):
    """The record forms on caller-built records, a workspace of exactly dffw_conv_pw_wgrad_workspace_bytes() and a side stream: guards intact; the
    same bits with a zero-filled as with a 0xFF workspace; masked elements +0 and passed elements gy's bits; every result bit-identical to the op
    forms on the same fp32 tensors (record values, so the op shell stages the very same records); grad_w and the sum under their bounds."""
    c = record_inputs(prec, C)
    a = run_record_chain(eng, prec, C, c, 0xFF)
    b = run_record_chain(eng, prec, C, c, 0x00)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    # the mask: y's stored value > 0 keeps gy's record bits, everything else is +0 in every part
    keep = (c["a2"] > 0).permute(0, 2, 3, 4, 1)[:, :, :, :, None, :].expand_as(a["g2_records"])
    assert torch.equal(a["g2_records"], torch.where(keep, a["gy_records"], torch.zeros_like(a["gy_records"])))
    assert 0 < int(keep.sum()) < keep.numel()
    g2 = cg.from_records(a["g2_records"], prec, C)
    # the op forms
    op_g2 = eng.op_grad_combine(c["gy"].cuda(), y=c["a2"].cuda(), precision=prec)
    assert eng.op_kernels() == ["dffw::grad_combine_kernel<%d, 1, 0>" % PREC_ID[prec]]
    assert torch.equal(op_g2.cpu(), g2) and torch.equal(g2.double(), pw.combine_ref64(c["gy"], c["a2"], None, prec)[0])
    _, op_gw = eng.op_conv_pw_backward(c["a1"].cuda(), torch.zeros(C, C, 1, 1, 1), g2.cuda(), pad=0, precision=prec, need=("w",))
    assert torch.equal(op_gw.cpu(), a["gw"])
    op_sum = eng.op_grad_combine(g2.cuda(), b=c["gb"].cuda(), precision=prec)
    got_sum = cg.from_records(a["sum_records"], prec, C)
    assert torch.equal(op_sum.cpu(), got_sum)
    # the bounds
    ww = eb.check_elementwise(a["gw"], pw.wgrad_ref64(c["a1"], g2, "k111"), prec, "grad_w of the record form")
    ref, bound = pw.combine_ref64(g2, None, c["gb"], prec)
    err = (got_sum.double() - ref).abs()
    ws = float(eb._ratio(err, bound).max())
    print("pw record chain %s C=%d %s: grad_w err/bound %.3f, sum %.3f" % (prec, C, REC_SHAPE, ww, ws))
    assert bool((err <= bound).all()) and float(a["gw"].abs().max()) > 0


@pytest.mark.parametrize("prec", pw.PRECISIONS)
def test_grad_combine_op_forms(eng, prec):
    """op_grad_combine in its three forms at a channel count that is no power of two (24) and on a volume of several units with a ragged last one:
    mask only exact, with b under (u + 2^-23) |ref|; the mask comes from y, not from a."""
    g = torch.Generator().manual_seed(7)
    shape = (2, 24, 3, 20, 23)     # 2 760 pixels: five full 512-pixel units and a ragged one
    a, y, b = (torch.randn(shape, generator=g) for _ in range(3))
    out = eng.op_grad_combine(a.cuda(), y=y.cuda(), precision=prec).cpu()
    assert torch.equal(out.double(), pw.combine_ref64(a, y, None, prec)[0])
    for yy, name in ((y, "1, 1"), (None, "0, 1")):
        out = eng.op_grad_combine(a.cuda(), y=None if yy is None else yy.cuda(), b=b.cuda(), precision=prec).cpu()
        assert eng.op_kernels() == ["dffw::grad_combine_kernel<%d, %s>" % (PREC_ID[prec], name)]
        ref, bound = pw.combine_ref64(a, yy, b, prec)
        err = (out.double() - ref).abs()
        assert bool((err <= bound).all()), float(eb._ratio(err, bound).max())
        assert torch.equal(out, pw.emulate_combine(a, yy, b, prec))


# ---- one attention tail behind a conv and the loss, in the caller's autograd graph ------------------------------------------------------------
def test_autograd_attention_tail_behind_heads_loss(eng):
    """pipeline.conv3d (3x1x1) -> relu -> pipeline.conv3d (1x1x1) -> relu -> + feat -> pipeline.conv3d (3x3x3) -> HeadsLoss: feat.grad and the three
    weight gradients against the float64 CPU graph evaluated from the GPU's own intermediates, the ReLU masks taken from the GPU's forward values.
    Each stage's own bound holds at the gradient the GPU handed it; the bound of that gradient is carried through the stage's adjoint with
    absolute values.  Where a GPU mask differs from the float64 forward's, the float64 pre-activation lies within the forward bound of zero."""
    from dffinthewild_amd import pipeline
    prec, C = "bf16x3", 8
    g = torch.Generator().manual_seed(13)
    feat, w3, _ = pw.make_case("zero_mean", "k311", 1, C, C, 4, 16, 16, 29)
    _, w1, _ = pw.make_case("zero_mean", "k111", 1, C, C, 4, 16, 16, 31)
    _, w2, _ = cg.make_case("zero_mean", "k333", 1, C, 8, 4, 16, 16, 37)
    fd = 0.1 + 1.4 * torch.rand(1, 4, 1, 1, generator=g)
    gt = 0.1 + 1.4 * torch.rand(1, 16, 16, generator=g)
    mask = torch.rand(1, 16, 16, generator=g) < 0.7
    fg = feat.cuda().requires_grad_(True)
    w3g, w1g, w2g = (t.clone().requires_grad_(True) for t in (w3, w1, w2))
    t1 = pipeline.conv3d(fg, w3g, pad=(1, 0, 0), precision=prec)
    r1 = torch.relu(t1)
    t2 = pipeline.conv3d(r1, w1g, pad=0, precision=prec)
    r2 = torch.relu(t2)
    s = r2 + fg
    y = pipeline.conv3d(s, w2g, stride=1, pad=1, precision=prec)
    for t in (t1, t2, s, y):
        t.retain_grad()
    total = pipeline.HeadsLoss.apply(y[:, 0], y[:, 1], y[:, 2], y[:, 3], fd.cuda(), gt.cuda(), mask.cuda())
    total.backward()
    t1c, r1c, t2c, sc = (t.detach().cpu() for t in (t1, r1, t2, s))
    gy_gpu, gs_gpu, gt2_gpu, gt1_gpu = y.grad.cpu(), s.grad.cpu(), t2.grad.cpu(), t1.grad.cpu()
    m1, m2 = (t1c > 0).double(), (t2c > 0).double()
    # the forward masks against the float64 forward: a disagreement only where the pre-activation is within its bound of zero
    for name, got, r in (("t1", t1c, eb.conv_ref64(feat, w3, pad=(1, 0, 0))), ("t2", t2c, eb.conv_ref64(r1c, w1))):
        differ = (got > 0) != (r.ref > 0)
        assert bool((r.ref.abs()[differ] <= r.bound(prec)[differ]).all()), name
        eb.check_elementwise(got, r, prec, name)
    # stage 1, the loss: its gradient at the GPU's score volumes
    lcase = dict(scores=[y.detach()[:, k].cpu() for k in range(4)], fd=fd, gt=gt, mask=mask, conf=None, weights=list(L.WEIGHTS), rng=None)
    gy64, Ey = torch.zeros_like(gy_gpu, dtype=torch.float64), torch.zeros_like(gy_gpu, dtype=torch.float64)
    for k, (gk, Gk) in enumerate(zip(L.reference(lcase)["grads"], L.bound(lcase))):
        gy64[:, k], Ey[:, k] = gk, L.ALPHA * Gk
    assert bool(((gy_gpu.double() - gy64).abs() <= Ey).all())
    # stage 2, the 3x3x3 conv at the GPU's s
    gs64, gw2_64 = cg.grads64(sc, w2, gy64, "k333")
    wa, kw = cg.adjoint_conv(w2, "k333")
    Es = cg.dgrad_ref64(w2, gy_gpu, "k333").bound(prec) + eb.conv_ref64(Ey, wa.abs(), **kw).ref
    bw2 = cg.wgrad_ref64(sc, gy_gpu, "k333", tuple(w2.shape)).bound(prec) + cg.wgrad_ref64(sc.abs(), Ey, "k333", tuple(w2.shape)).ref
    assert bool(((gs_gpu.double() - gs64).abs() <= Es).all())
    # stage 3, the second ReLU (torch: exact on the GPU's mask) and the 1x1x1 conv at the GPU's r1
    gt2_64, Et2 = gs64 * m2, Es * m2
    assert bool(((gt2_gpu.double() - gt2_64).abs() <= Et2).all())
    gr1_64, gw1_64 = pw.grads64(r1c, w1, gt2_64, "k111")
    wa1, kw1 = pw.adjoint_conv(w1, "k111")
    Er1 = pw.dgrad_ref64(w1, gt2_gpu, "k111").bound(prec) + eb.conv_ref64(Et2, wa1.abs(), **kw1).ref
    bw1 = pw.wgrad_ref64(r1c, gt2_gpu, "k111").bound(prec) + pw.wgrad_ref64(r1c.abs(), Et2, "k111").ref
    # stage 4, the first ReLU and the 3x1x1 conv at feat
    gt1_64, Et1 = gr1_64 * m1, Er1 * m1
    assert bool(((gt1_gpu.double() - gt1_64).abs() <= Et1).all())
    gfa_64, gw3_64 = pw.grads64(feat, w3, gt1_64, "k311")
    wa3, kw3 = pw.adjoint_conv(w3, "k311")
    Efa = pw.dgrad_ref64(w3, gt1_gpu, "k311").bound(prec) + eb.conv_ref64(Et1, wa3.abs(), **kw3).ref
    bw3 = pw.wgrad_ref64(feat, gt1_gpu, "k311").bound(prec) + pw.wgrad_ref64(feat.abs(), Et1, "k311").ref
    # feat has two consumers: torch adds the skip's gradient and the tail's in fp32 (one rounding of the sum)
    gf64 = gs64 + gfa_64
    checks = {"feat.grad": (fg.grad, gf64, Es + Efa + 2.0 ** -23 * gf64.abs()), "w3.grad": (w3g.grad, gw3_64, bw3), "w1.grad": (w1g.grad, gw1_64, bw1),
              "w2.grad": (w2g.grad, gw2_64, bw2)}
    worst = {}
    for name, (got, ref, bound) in checks.items():
        err = (got.detach().cpu().double() - ref).abs()
        worst[name] = float(eb._ratio(err, bound).max())
        assert bool((err <= bound).all()), (name, worst[name])
    print("autograd 3x1x1 -> relu -> 1x1x1 -> relu -> +feat -> 3x3x3 -> HeadsLoss: err/bound " + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert fg.grad.is_cuda and not w3g.grad.is_cuda and w3g.grad.shape == w3.shape and w1g.grad.shape == w1.shape
    assert float(fg.grad.abs().max()) > 0 and float(w3g.grad.abs().max()) > 0 and float(w1g.grad.abs().max()) > 0
    assert 0 < float(m1.mean()) < 1 and 0 < float(m2.mean()) < 1
