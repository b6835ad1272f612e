"""Backward of the score convs, Cin -> 1, on the GPU: every element of grad_x and grad_w against the float64 formulas on
the record-rounded operands under the derived bounds of tests/score_grad_ref.py, and bit for bit against its emulation of the kernels'
arithmetic, in all three precisions, through the op form and its poisoned workspace; unit impulses at the sample, slice, row and column
boundaries; integer data against float64 autograd and bit-identity between calls; the record forms on a side stream between guards, behind
dffw_loss_heads; the real head chain conv -> score conv -> HeadsLoss in the caller's autograd graph.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 19 is where the table of them goes."""
import functools
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_grad_ref as cg  # noqa: E402
import loss_ref as L  # noqa: E402
import score_grad_ref as sg  # noqa: E402
from test_gpu_train_records import Guarded, PREC_ID, i3, nbytes_records, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

K_OF = {"k111": 1, "k333": 3}


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def dgrad_name(prec, geom, add):
    return "dffw::score_dgrad_kernel<%d, %d, %d>" % (PREC_ID[prec], K_OF[geom], int(add))


def wgrad_names(prec, geom):
    return ["dffw::score_wgrad_kernel<%d, %d>" % (PREC_ID[prec], K_OF[geom]), "dffw::score_wgrad_finish_kernel"]


def set_grid(monkeypatch, wgs):
    """DFFW_SCORE_WGS=8: every workgroup of a volume of more than 8 units walks several of them."""
    if wgs == sg.DEFAULT_WGS:
        monkeypatch.delenv("DFFW_SCORE_WGS", raising=False)
    else:
        monkeypatch.setenv("DFFW_SCORE_WGS", str(wgs))


def pad_of(geom):
    return sg.GEOMETRIES[geom][1]


@functools.lru_cache(maxsize=None)
def op_case(geom, shape, C, aligned_b):
    """One case's operands (the seeds of tests/test_score_grad.py): made once, shared by the tests, never changed."""
    return sg.make_case(geom, shape, C, 11 + C + sum(shape), aligned_b=aligned_b)


@functools.lru_cache(maxsize=None)
def op_refs(geom, shape, C, prec):
    """... and per precision its (ref64, bound, emulation) for grad_x, grad_x + b and, per grid, grad_w."""
    x, w, g, b = op_case(geom, shape, C, geom == "k111" and prec == "fp16")
    out = {}
    for bb, key in ((None, "x"), (b, "x + b")):
        out[key] = sg.dgrad_ref64(w, g, bb, geom, prec) + (sg.emulate_dgrad(w, g, bb, geom, prec),)
    for wgs in sg.grids_of(geom, shape):
        out["w", wgs] = sg.wgrad_ref64(x, g, geom, prec, sg.wgrad_chain(geom, shape, C, wgs)) + (sg.emulate_wgrad(x, g, geom, prec, wgs=wgs),)
    return out


@pytest.mark.parametrize("prec", sg.PRECISIONS)
@pytest.mark.parametrize("geom", sorted(sg.GEOMETRIES))
def test_op_forms(eng, geom, prec, monkeypatch):
    """Every shape and channel count, with and without b, need = both, x, w; the shapes of more than one unit also on the grid of 8.  Every
    element under its bound and equal to the emulation bit for bit; op_kernels() names exactly the launches.  A NaN left by the poisoned
    workspace, or an element no thread wrote, fails the comparison."""
    worst = {"x": 0.0, "x + b": 0.0, "w": 0.0}
    pad = pad_of(geom)
    for shape in sg.SHAPES[geom]:
        for C in sg.CHANNELS[geom]:
            x, w, g, b = (t.cuda() for t in op_case(geom, shape, C, geom == "k111" and prec == "fp16"))
            refs = op_refs(geom, shape, C, prec)
            what = "%s %s %s C=%d" % (geom, prec, shape, C)
            for wgs in sg.grids_of(geom, shape):
                set_grid(monkeypatch, wgs)
                gxb, gw = eng.op_score_conv_backward(x, w, g, pad=pad, b=b, precision=prec)
                assert eng.op_kernels() == [dgrad_name(prec, geom, True)] + wgrad_names(prec, geom), what
                gx, none = eng.op_score_conv_backward(x, w, g, pad=pad, precision=prec, need=("x",))
                assert none is None and eng.op_kernels() == [dgrad_name(prec, geom, False)], what
                none, gw_only = eng.op_score_conv_backward(x, w, g, pad=pad, precision=prec, need=("w",))
                assert none is None and eng.op_kernels() == wgrad_names(prec, geom), what
                assert gw.shape == w.shape and gx.shape == x.shape and sg.same_bits(gw_only, gw), what
                for key, got in (("x", gx), ("x + b", gxb), ("w", gw)):
                    ref, bound, emu = refs[key if key != "w" else ("w", wgs)]
                    worst[key] = max(worst[key], sg.check(got, ref, bound, "%s grad_%s wgs=%d" % (what, key, wgs)))
                    assert torch.equal(got.cpu(), emu), "%s grad_%s wgs=%d differs from the emulation in %d elements" % (
                        what, key, wgs, int((got.cpu() != emu).sum()))
    print("score_grad op forms %s %s: err/bound " % (geom, prec) + " ".join("%s %.3f" % kv for kv in worst.items()))


@pytest.mark.parametrize("prec", sg.PRECISIONS)
@pytest.mark.parametrize("geom", sorted(sg.GEOMETRIES))
def test_unit_impulses(eng, geom, prec):
    """g = 1 at sample 0's last slice, last row, last column and at sample 1's slice 0, pixel (0, 0).  grad_x is the record of the filter at the
    neighbours p + k - 1 that lie inside the impulse's own sample, slice range and plane, and exactly 0 elsewhere; grad_w[c, k] is the sum of
    the (at most two) record values of x at p + k - 1, exactly 0 for a tap that points across a boundary from both impulses."""
    shape, C = (2, 3, 5, 7), 24 if geom == "k111" else 8
    B, N, H, W = shape
    k = K_OF[geom]
    x, w, _, _ = sg.make_case(geom, shape, C, 41)
    g = torch.zeros(B, N, H, W)
    impulses = [(0, N - 1, H - 1, W - 1), (1, 0, 0, 0)]
    for p in impulses:
        g[p] = 1.0
    wr, xr = sg.rounded(w, prec), sg.rounded(x, prec)
    want_x = torch.zeros(B, C, N, H, W)
    want_w = torch.zeros(1, C, k, k, k, dtype=torch.float64)
    outside = torch.ones(k, k, k, dtype=torch.bool)
    for b, n, y, xx in impulses:
        for kz in range(k):
            for ky in range(k):
                for kx in range(k):
                    q = (n + kz - k // 2, y + ky - k // 2, xx + kx - k // 2)
                    if all(0 <= v < m for v, m in zip(q, (N, H, W))):
                        want_x[(b, slice(None)) + q] = wr[0, :, kz, ky, kx]
                        want_w[0, :, kz, ky, kx] += xr[(b, slice(None)) + q].double()
                        outside[kz, ky, kx] = False
    gx, gw = eng.op_score_conv_backward(x.cuda(), w.cuda(), g.cuda(), pad=pad_of(geom), precision=prec)
    assert torch.equal(gx.cpu(), want_x), int((gx.cpu() != want_x).sum())
    assert int((want_x != 0).sum()) == C * (2 if k == 1 else 16)      # two corners: 8 taps each stay inside
    assert torch.equal(gw.cpu(), want_w.float()), int((gw.cpu() != want_w.float()).sum())
    if k == 3:
        assert int(outside.sum()) == 27 - 15 and bool((gw.cpu()[0][:, outside] == 0).all())


@pytest.mark.parametrize("geom", sorted(sg.GEOMETRIES))
def test_exactness_and_determinism(eng, geom, monkeypatch):
    """Integer data: grad_w equals float64 autograd bit for bit on the default grid and on the grid of 8, grad_x (+ b) equals it too.  Two calls
    give identical bits, on integer and on random data."""
    shape, C = sg.SHAPES[geom][-1], 24 if geom == "k111" else 40
    pad = pad_of(geom)
    xi, wi, gi, bi = sg.int_case(geom, shape, C, 5)
    gx64, gw64 = sg.grads64(xi, wi, gi, geom)
    xr, wr, gr, br = op_case(geom, shape, C, False)
    for prec in sg.PRECISIONS:
        first = {}
        for wgs in (sg.DEFAULT_WGS, sg.SMALL_WGS):
            set_grid(monkeypatch, wgs)
            gx, gw = eng.op_score_conv_backward(xi.cuda(), wi.cuda(), gi.cuda(), pad=pad, b=bi.cuda(), precision=prec)
            assert sg.same_bits(gw, gw64.float()) and torch.equal(gw.cpu().double(), gw64), (prec, wgs)
            assert torch.equal(gx.cpu().double(), gx64 + bi.double()), (prec, wgs)
            for run in range(2):
                got = eng.op_score_conv_backward(xr.cuda(), wr.cuda(), gr.cuda(), pad=pad, b=br.cuda(), precision=prec)
                for name, t in zip(("x", "w"), got):
                    assert sg.same_bits(t, first.setdefault((wgs, name), t)), (prec, wgs, name, run)
            assert sg.same_bits(first[wgs, "x"], first[sg.DEFAULT_WGS, "x"])      # grad_x does not depend on the grid at all


# ---- the record forms, as a training step calls them ------------------------------------------------------------------------------------------
REC = dict(B=2, N=3, H=32, W=32)      # the heads' resolutions: 4x4 (conf, k333, C = 32) ... 32x32 (cost3, k111, C = 8)


def run_record_chain(eng, prec, c, fill):
    """dffw_loss_heads -> dffw_score_conv_dgrad with out aliasing b, and dffw_score_conv_wgrad with exactly ..._workspace_bytes(), for the
    coarsest head (k333) and the finest (k111), all enqueued on one side stream; one host synchronisation at the end.  Every buffer the score
    kernels write lies between guards; the workspaces are filled with ``fill`` first."""
    lib, dev, Pn = eng.lib, torch.cuda.current_device(), PREC_ID[prec]
    B, N = REC["B"], REC["N"]
    heads = {"k333": (0, 32), "k111": (3, 8)}
    sizes, wsb = {}, {}
    for geom, (k, C) in heads.items():
        h, w = c["scores"][k].shape[2:]
        kk, pp = i3((K_OF[geom],) * 3), i3((pad_of(geom),) * 3)
        wsb[geom] = lib.dffw_score_conv_wgrad_workspace_bytes(B, C, N, h, w, kk, pp)
        assert wsb[geom] == sg.grid_of(geom, (B, N, h, w)) * C * K_OF[geom] ** 3 * 8
        sizes.update({"gx_" + geom: nbytes_records(prec, B, C, N, h, w), "ws_" + geom: wsb[geom], "gw_" + geom: 4 * C * K_OF[geom] ** 3})
    G = Guarded(sizes)
    rec = {}
    for geom in heads:
        G.raw("ws_" + geom).fill_(fill)
        G.raw("gx_" + geom).copy_(cg.to_records(c["b_" + geom], prec).cuda().reshape(-1).view(torch.uint8))      # b's records: out aliases b
        rec[geom] = cg.to_records(c["x_" + geom], prec).cuda()
    wdev = {geom: c["w_" + geom].cuda() for geom in heads}
    scores = [s.cuda() for s in c["scores"]]
    fd, gt, mask = c["fd"].cuda(), c["gt"].cuda(), c["mask"].cuda()
    stream, sp = side_stream()
    names = []
    with torch.cuda.stream(stream):
        _, _, grads = eng.op_loss_heads(scores, fd, gt, mask, preds=False)
    for geom, (k, C) in heads.items():
        h, w = c["scores"][k].shape[2:]
        kk, pp = i3((K_OF[geom],) * 3), i3((pad_of(geom),) * 3)
        rc = lib.dffw_score_conv_dgrad(dev, Pn, grads[k].data_ptr(), B, C, N, h, w, wdev[geom].data_ptr(), kk, pp, G.ptr("gx_" + geom), G.ptr("gx_" + geom), sp)
        assert rc == 0, lib.dffw_last_error().decode()
        names.append(eng.op_kernels())
        rc = lib.dffw_score_conv_wgrad(dev, Pn, rec[geom].data_ptr(), grads[k].data_ptr(), B, C, N, h, w, kk, pp, G.ptr("gw_" + geom), G.ptr("ws_" + geom),
                                       wsb[geom], sp)
        assert rc == 0, lib.dffw_last_error().decode()
        names.append(eng.op_kernels())
    stream.synchronize()      # the only host synchronisation
    G.check()
    assert names == [[dgrad_name(prec, "k333", True)], wgrad_names(prec, "k333"), [dgrad_name(prec, "k111", True)], wgrad_names(prec, "k111")], names
    parts = 2 if prec == "bf16x3" else 1
    out = {"grads": [t.cpu() for t in grads]}
    for geom, (k, C) in heads.items():
        h, w = c["scores"][k].shape[2:]
        out["gx_" + geom] = cg.from_records(G.view("gx_" + geom, torch.int16, (B, N, h, w, parts, C)).cpu().clone(), prec, C)
        out["gw_" + geom] = G.view("gw_" + geom, torch.float32, sg.weight_shape(geom, C)).cpu().clone()
    return out


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_record_chain(eng, lib_built, prec):
    """The record forms behind dffw_loss_heads on a side stream: guards intact; a zero-filled and a 0xFF workspace give the same bits; results
    bit-identical to the op form on the same fp32 tensors (record values, so the op shell stages the very same records) and under their bounds;
    op_kernels() names the kernels launched, and those names are kernel symbols of the library."""
    B, N, H, W = (REC[k] for k in "BNHW")
    gen = torch.Generator().manual_seed(61)
    c = dict(scores=[torch.rand(B, N, H // s, W // s, generator=gen) * 2 - 1 for s in (8, 4, 2, 1)], fd=0.1 + 1.4 * torch.rand(B, N, 1, 1, generator=gen),
             gt=0.1 + 1.4 * torch.rand(B, H, W, generator=gen), mask=(torch.rand(B, H, W, generator=gen) < 0.7).to(torch.uint8))
    for geom, (k, C) in {"k333": (0, 32), "k111": (3, 8)}.items():
        x, w, _, b = sg.make_case(geom, (B, N) + tuple(c["scores"][k].shape[2:]), C, 67 + C)
        c.update({"x_" + geom: sg.rounded(x, prec), "b_" + geom: sg.rounded(b, prec), "w_" + geom: w})
    a = run_record_chain(eng, prec, c, 0xFF)
    z = run_record_chain(eng, prec, c, 0x00)
    for name in a:
        if name != "grads":
            assert sg.same_bits(a[name], z[name]), name
    worst = {}
    for geom, k in (("k333", 0), ("k111", 3)):
        g = a["grads"][k]
        assert torch.equal(g, z["grads"][k]) and float(g.abs().max()) > 0
        x, w, b = c["x_" + geom], c["w_" + geom], c["b_" + geom]
        gx, gw = eng.op_score_conv_backward(x.cuda(), w.cuda(), g.cuda(), pad=pad_of(geom), b=b.cuda(), precision=prec)
        assert sg.same_bits(gx, a["gx_" + geom]) and sg.same_bits(gw, a["gw_" + geom]), geom
        shape = (B, N) + tuple(g.shape[2:])
        worst["x " + geom] = sg.check(a["gx_" + geom], *sg.dgrad_ref64(w, g, b, geom, prec), "record form grad_x " + geom)
        worst["w " + geom] = sg.check(a["gw_" + geom], *sg.wgrad_ref64(x, g, geom, prec, sg.wgrad_chain(geom, shape, x.shape[1])), "record form grad_w " + geom)
    print("score_grad record chain %s: err/bound " % prec + " ".join("%s %.3f" % kv for kv in worst.items()))
    symbols = subprocess.run(["nm", "-DC", lib_built], capture_output=True, text=True, check=True).stdout
    for name in [dgrad_name(prec, "k333", True), dgrad_name(prec, "k111", True)] + wgrad_names(prec, "k333") + wgrad_names(prec, "k111"):
        assert "%s(" % name in symbols, name


# ---- the real head chain in the caller's autograd graph ------------------------------------------------------------------------------------------
def test_autograd_real_head_chain(eng):
    """Four pipeline.conv3d (3x3x3) features at H/8 (32 channels), H/4 (32), H/2 (16) and H (8) of a (1, 4, 16, 24) stack, each through
    pipeline.score_conv (k333 for the first, k111 for the others), all four into HeadsLoss, split-bf16.  The four feature gradients, the four
    score-conv weight gradients and the four upstream weight gradients against the float64 graph evaluated from the GPU's own intermediates:
    each stage's own bound holds at the gradient the GPU handed it, and the bound of that gradient is carried through the stage's adjoint with
    absolute values."""
    from dffinthewild_amd import pipeline
    prec, (B, N, H, W), Cin = "bf16x3", (1, 4, 16, 24), 8
    gen = torch.Generator().manual_seed(71)
    fd = 0.1 + 1.4 * torch.rand(B, N, 1, 1, generator=gen)
    gt = 0.1 + 1.4 * torch.rand(B, H, W, generator=gen)
    mask = torch.rand(B, H, W, generator=gen) < 0.7
    heads = [(8, 32, "k333"), (4, 32, "k111"), (2, 16, "k111"), (1, 8, "k111")]
    ins, Ws, Vs, feats, scores = [], [], [], [], []
    for i, (s, C, geom) in enumerate(heads):
        xin, Wk, _ = cg.make_case("zero_mean", "k333", B, Cin, C, N, H // s, W // s, 73 + i)
        _, v, _, _ = sg.make_case(geom, (B, N, H // s, W // s), C, 79 + i)
        ins.append(xin)
        Ws.append(Wk.clone().requires_grad_(True))
        Vs.append(v.clone().requires_grad_(True))
        f = pipeline.conv3d(xin.cuda(), Ws[-1], stride=1, pad=1, precision=prec)
        sc = pipeline.score_conv(f, Vs[-1], pad=pad_of(geom), precision=prec)
        assert sc.shape == (B, N, H // s, W // s)
        f.retain_grad()
        sc.retain_grad()
        feats.append(f)
        scores.append(sc)
    total = pipeline.HeadsLoss.apply(*scores, fd.cuda(), gt.cuda(), mask.cuda())
    total.backward()
    # stage 1, the loss: its gradient at the GPU's score volumes
    lcase = dict(scores=[sc.detach().cpu() for sc in scores], fd=fd, gt=gt, mask=mask, conf=None, weights=list(L.WEIGHTS), rng=None)
    g64s, Es = L.reference(lcase)["grads"], [L.ALPHA * Gk for Gk in L.bound(lcase)]
    worst = {}

    def le(name, got, ref, bound):
        worst[name] = sg.worst_ratio(got, ref, bound)
        assert worst[name] <= 1.0, (name, worst[name])

    for i, (s, C, geom) in enumerate(heads):
        g_gpu, g64, E = scores[i].grad.cpu(), g64s[i].double(), Es[i].double()
        le("s%d" % i, g_gpu, g64, E)
        # stage 2, the score conv at the GPU's feature (record values) and the gradient the GPU handed it
        fc, v = feats[i].detach().cpu(), Vs[i].detach()
        assert torch.equal(sg.rounded(fc, prec), fc)
        shape = (B, N, H // s, W // s)
        gf64 = sg.dgrad_of(v.double(), g64, None, geom)
        Ef = sg.dgrad_ref64(v, g_gpu, None, geom, prec)[1] + sg.dgrad_of(v.double().abs(), E, None, geom)
        gf_gpu = feats[i].grad.cpu()
        le("f%d.grad" % i, gf_gpu, gf64, Ef)
        gv64 = sg.wgrad_of(fc.double(), g64, geom)
        bv = sg.wgrad_ref64(fc, g_gpu, geom, prec, sg.wgrad_chain(geom, shape, C))[1] + sg.wgrad_of(fc.double().abs(), E, geom)
        le("v%d.grad" % i, Vs[i].grad, gv64, bv)
        # stage 3, the upstream conv's weight at its input
        wshape = tuple(Ws[i].shape)
        _, gW64 = cg.grads64(ins[i], Ws[i].detach(), gf64, "k333")
        bW = cg.wgrad_ref64(ins[i], gf_gpu, "k333", wshape).bound(prec) + cg.wgrad_ref64(ins[i].abs(), Ef, "k333", wshape).ref
        le("W%d.grad" % i, Ws[i].grad, gW64, bW)
        assert Vs[i].grad.shape == Vs[i].shape and not Vs[i].grad.is_cuda and float(Vs[i].grad.abs().max()) > 0 and float(Ws[i].grad.abs().max()) > 0
    print("autograd conv -> score conv -> HeadsLoss: err/bound " + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert eng.op_kernels()      # the last backward op launched kernels of the library


def test_refusals(eng):
    x = torch.zeros(1, 8, 2, 4, 4, device="cuda")
    g = torch.zeros(1, 2, 4, 4, device="cuda")
    w1, w3 = torch.zeros(1, 8, 1, 1, 1), torch.zeros(1, 8, 3, 3, 3)
    with pytest.raises(RuntimeError):    # CPU tensors: no fallback
        eng.op_score_conv_backward(x.cpu(), w1, g.cpu(), pad=0)
    for C in (4, 136):                   # Cin
        with pytest.raises(ValueError):
            eng.op_score_conv_backward(torch.zeros(1, C, 2, 4, 4, device="cuda"), torch.zeros(1, C, 1, 1, 1), g, pad=0)
    with pytest.raises(ValueError):      # Cout = 8
        eng.op_score_conv_backward(x, torch.zeros(8, 8, 1, 1, 1), g, pad=0)
    with pytest.raises(ValueError):      # kernel (1,3,3)
        eng.op_score_conv_backward(x, torch.zeros(1, 8, 1, 3, 3), g, pad=(0, 1, 1))
    with pytest.raises(ValueError):      # pad mismatch
        eng.op_score_conv_backward(x, w3, g, pad=0)
    with pytest.raises(ValueError):
        eng.op_score_conv_backward(x, w1, g, pad=1)
    with pytest.raises(ValueError):      # grad_score of another shape, or with a channel axis
        eng.op_score_conv_backward(x, w1, torch.zeros(1, 2, 4, 5, device="cuda"), pad=0)
    with pytest.raises(ValueError):
        eng.op_score_conv_backward(x, w1, g[:, None], pad=0)
    with pytest.raises(ValueError):      # b of another shape
        eng.op_score_conv_backward(x, w1, g, pad=0, b=x[:, :, :1])
    assert eng.op_kernels() == []        # nothing was launched
