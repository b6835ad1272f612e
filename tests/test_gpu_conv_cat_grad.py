"""Backward of a conv over a channel concatenation on the GPU: dffw_conv_cat_wgrad (the record form a training step
calls), dffw_op_conv_cat_backward (engine.op_conv_cat_backward) and the autograd node pipeline.conv3d_cat.  Where the plain path exists
(Ca + Cb <= 128) every bit is compared with it; beyond, every element of the three gradients is held to its bound of tests/conv_cat_grad_ref.py.
The op forms poison their workspace with 0xFF; the record form's buffers lie between guard regions (tests/test_gpu_train_records.py: Guarded)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cat_grad_ref as cc  # noqa: E402
import conv_grad_ref as cg  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402
from test_gpu_train_records import Guarded, PREC_ID, i3, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

# where conv3d on the concatenation is served.  The switch lies: on a 16-tile boundary inside a 32-group (16+16), on a group boundary (32+32,
# 64+64), inside a 16-wide MFMA tile (8+8, 8+24, 24+40, 8+120)
SMALL_PAIRS = [(8, 8), (16, 16), (8, 24), (24, 40), (32, 32), (64, 64), (8, 120)]
SMALL_SHAPES = [(2, 3, 12, 20), (1, 1, 8, 8)]
# past 128 channels: on a group boundary (128+64, 64+128), inside a 16-wide tile (104+88: octet 13 of 24; 128+56: a ragged last group)
WIDE_PAIRS = [(128, 64), (64, 128), (104, 88), (128, 56)]
WIDE_SHAPES = [(2, 3, 12, 20), (1, 2, 4, 16)]
KERNELS = lambda prec: ["dffw::conv_wgrad_cat_kernel<%d>" % PREC_ID[prec], "dffw::conv_wgrad_finish_kernel"]   # noqa: E731


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def cat_wgrad_on_records(eng, prec, xa, xb, gy, fill=0xFF):
    """dffw_conv_cat_wgrad on the records of xa, xb and gy as a training step calls it: a workspace of exactly
    dffw_conv_cat_wgrad_workspace_bytes() and grad_w between guard regions, a side stream; returns grad_w (a copy) after the checks."""
    B, ca, N, H, W = xa.shape
    cb, cout = xb.shape[1], gy.shape[1]
    dev = torch.cuda.current_device()
    ar, br, gyr = (cg.to_records(t, prec).cuda() for t in (xa, xb, gy))
    wsb = eng.lib.dffw_conv_cat_wgrad_workspace_bytes(B, ca, cb, N, H, W, cout)
    assert wsb > 0
    wshape = (cout, ca + cb, 3, 3, 3)
    G = Guarded(dict(ws=wsb, gw=4 * cout * (ca + cb) * 27))
    G.raw("ws").fill_(fill)
    stream, sp = side_stream()
    rc = eng.lib.dffw_conv_cat_wgrad(dev, PREC_ID[prec], ar.data_ptr(), ca, br.data_ptr(), cb, B, N, H, W, gyr.data_ptr(), cout, G.ptr("gw"), G.ptr("ws"),
                                     wsb, sp)
    assert rc == 0, eng.lib.dffw_last_error().decode()
    assert eng.op_kernels() == KERNELS(prec)
    stream.synchronize()
    G.check()   # no byte outside the workspace and grad_w
    return G.view("gw", torch.float32, wshape).clone()


def plain_wgrad_on_records(eng, prec, x, gy):
    """dffw_conv_wgrad (3x3x3 stride 1) on the records of the materialised concatenation."""
    B, cin, N, H, W = x.shape
    cout = gy.shape[1]
    k, s, p, t = cg.GEOMETRIES[cc.GEOM]
    xr, gyr = cg.to_records(x, prec).cuda(), cg.to_records(gy, prec).cuda()
    wsb = eng.lib.dffw_conv_wgrad_workspace_bytes(B, cin, N, H, W, cout, i3(k), i3(s), i3(p), int(t))
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    gw = torch.full((cout, cin, 3, 3, 3), float("nan"), device="cuda")
    rc = eng.lib.dffw_conv_wgrad(torch.cuda.current_device(), PREC_ID[prec], xr.data_ptr(), B, cin, N, H, W, gyr.data_ptr(), cout, i3(k), i3(s), i3(p),
                                 int(t), gw.data_ptr(), ws.data_ptr(), wsb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.dffw_last_error().decode()
    torch.cuda.synchronize()
    return gw


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", SMALL_PAIRS, ids=lambda p: "%d+%d" % p)
def test_bit_identical_to_the_plain_path(eng, pair, prec):
    """Where Ca + Cb <= 128 the old path exists: the record form's grad_w has the bits of dffw_conv_wgrad on the concatenated records, the op form's
    grad_w those of op_conv3d_backward, and its grad_xa / grad_xb are the two halves of that one's grad_x."""
    ca, cb = pair
    for cout in (8, 24):
        for shape in SMALL_SHAPES:
            B, N, H, W = shape
            xa, xb, w, gy = cc.cat_case("zero_mean", B, ca, cb, cout, N, H, W, seed=31 + ca + 3 * cb + cout)
            x = torch.cat([xa, xb], 1)
            what = "%d+%d -> %d %s %s" % (ca, cb, cout, shape, prec)
            gw = cat_wgrad_on_records(eng, prec, xa, xb, gy)
            assert torch.equal(gw, plain_wgrad_on_records(eng, prec, x, gy)), "record form, grad_w: " + what
            gxa, gxb, op_gw = eng.op_conv_cat_backward(xa.cuda(), xb.cuda(), w, gy.cuda(), precision=prec)
            assert eng.op_kernels() == KERNELS(prec)
            gx, plain_gw = eng.op_conv3d_backward(x.cuda(), w, gy.cuda(), stride=1, pad=1, precision=prec)
            assert torch.equal(op_gw, gw) and torch.equal(op_gw, plain_gw), "op form, grad_w: " + what
            assert torch.equal(gxa, gx[:, :ca]), "grad_xa: " + what
            assert torch.equal(gxb, gx[:, ca:]), "grad_xb: " + what
    print("conv_cat %d+%d %s: grad_w, grad_xa, grad_xb bit-identical to the plain path at Cout 8 and 24, %s" % (ca, cb, prec, SMALL_SHAPES))


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", WIDE_PAIRS, ids=lambda p: "%d+%d" % p)
def test_beyond_128_channels_every_element_under_its_bound(eng, pair, prec):
    ca, cb = pair
    for cout in (128, 16):
        for shape in WIDE_SHAPES:
            for regime in ("zero_mean", "post_relu"):
                xa, xb, w, gy, ra, rb, rw = cc.case(regime, ca, cb, cout, shape)
                gxa, gxb, gw = eng.op_conv_cat_backward(xa.cuda(), xb.cuda(), w, gy.cuda(), precision=prec)
                assert eng.op_kernels() == KERNELS(prec)
                what = "%d+%d -> %d %s %s" % (ca, cb, cout, shape, regime)
                # a NaN left by the poisoned workspace fails any of the three
                wa = eb.check_elementwise(gxa, ra, prec, "grad_xa " + what)
                wb = eb.check_elementwise(gxb, rb, prec, "grad_xb " + what)
                ww = eb.check_elementwise(gw, rw, prec, "grad_w " + what)
                print("conv_cat %s %s: err/bound grad_xa %.3f grad_xb %.3f (%s) grad_w %.3f" % (prec, what, wa, wb, eng.last_conv_kernel(), ww))


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair", WIDE_PAIRS, ids=lambda p: "%d+%d" % p)
def test_unit_impulse_gives_the_rounded_operand_on_both_sides_of_the_switch(eng, pair, prec):
    """grad_y = one unit impulse in its last channel: every element of that channel's grad_w is ONE product 1 * x, so it is the rounded operand
    exactly (hi + lo of an fp32 value is an fp32 value; the float64 finish adds zeros), from xa below Ca and from xb above."""
    ca, cb = pair
    for cout in (128, 16):
        B, N, H, W = WIDE_SHAPES[0]
        xa, xb, w, gy = cc.cat_case("impulse", B, ca, cb, cout, N, H, W, seed=3 + ca + cb, impulse_channel=cout - 1)
        _, _, gw = eng.op_conv_cat_backward(xa.cuda(), xb.cuda(), w, gy.cuda(), precision=prec, need=("w",))
        rounded = sum(cg.round_parts(torch.cat([xa, xb], 1), prec))
        n, y, x = N // 2, H // 2, W - 2     # where cg.make_case puts the impulse, in the last sample: the patch around it is in the volume
        want = torch.zeros(tuple(w.shape), dtype=torch.float64)
        want[cout - 1] = rounded[B - 1, :, n - 1:n + 2, y - 1:y + 2, x - 1:x + 2].double()
        assert float(gy[B - 1, cout - 1, n, y, x]) == 1.0 and float(gy.abs().sum()) == 1.0
        assert torch.equal(gw.cpu().double(), want)
        assert float(want[cout - 1, :ca].abs().min()) > 0 and float(want[cout - 1, ca:].abs().min()) > 0 and float(want[:cout - 1].abs().max()) == 0


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("pair,cout", [((128, 64), 128), ((104, 88), 16), ((24, 40), 24)], ids=lambda v: "%d+%d" % v if isinstance(v, tuple) else "to%d" % v)
def test_record_form_as_a_training_step_calls_it(eng, pair, cout, prec):
    """An exact workspace between guard regions, a side stream, rc 0 and the two kernel names, no byte outside the workspace and grad_w (all in
    cat_wgrad_on_records); identical bits with a zeroed and a 0xFF workspace and on a second call; the op form's bits; every element under its bound."""
    ca, cb = pair
    xa, xb, w, gy, _, _, rw = cc.case("zero_mean", ca, cb, cout, WIDE_SHAPES[0])
    gw = cat_wgrad_on_records(eng, prec, xa, xb, gy)
    worst = eb.check_elementwise(gw, rw, prec, "grad_w of the record form")
    assert torch.equal(cat_wgrad_on_records(eng, prec, xa, xb, gy, fill=0x00), gw)
    assert torch.equal(cat_wgrad_on_records(eng, prec, xa, xb, gy), gw)
    assert torch.equal(eng.op_conv_cat_backward(xa.cuda(), xb.cuda(), w, gy.cuda(), precision=prec, need=("w",))[2], gw)
    print("conv_cat record form %s %d+%d -> %d %s: grad_w err/bound %.3f" % (prec, ca, cb, cout, WIDE_SHAPES[0], worst))


@pytest.mark.parametrize("prec", cg.PRECISIONS)
def test_partials_on_a_small_grid(eng, prec, monkeypatch):
    """DFFW_WGRAD_WGS=8 at 16+16 -> 8 on (1, 2, 64, 64): 128 units on a grid of 8, so each workgroup sums 16 units of both sources into one set of
    accumulators; with DFFW_WGRAD_FLUSH_UNITS=3 also through several float64 flushes.  Within the bound, and deterministic."""
    xa, xb, w, gy, _, _, rw = cc.case("zero_mean", 16, 16, 8, (1, 2, 64, 64))
    run = lambda: eng.op_conv_cat_backward(xa.cuda(), xb.cuda(), w, gy.cuda(), precision=prec, need=("w",))[2]   # noqa: E731
    monkeypatch.setenv("DFFW_WGRAD_WGS", "8")
    small = run()
    worst = eb.check_elementwise(small, rw, prec, "grad_w on a grid of 8")
    assert torch.equal(run(), small)
    monkeypatch.setenv("DFFW_WGRAD_FLUSH_UNITS", "3")
    flushed = eb.check_elementwise(run(), rw, prec, "grad_w on a grid of 8, flushed every 3 units")
    print("conv_cat partials %s 16+16 -> 8 (1, 2, 64, 64), grid 8: grad_w err/bound %.3f, flushed every 3 units %.3f" % (prec, worst, flushed))


def test_autograd_chain_at_the_coarsest_level(eng):
    """The chain at the 1/32 level of hourglassup: conv3d 64 -> 128 stride (1,2,2) on (1,64,2,8,8) -> conv3d_cat with a (1,64,2,4,4) skip tensor and
    a 192 -> 128 weight -> batch_norm3d(relu) -> score_conv 128 -> 1 -> HeadsLoss.  The node's three gradients are held to their bounds, evaluated
    from the grad_y the GPU produced; xa.grad reaches the stride-2 conv's weight; three pipeline.Adam steps over all parameters (the loss is
    printed, not gated).  The same call through pipeline.conv3d on the concatenation still raises.
    The skip tensor holds record values (hi + lo of bf16x3), as every activation of the network does; xa and grad_y are kernel outputs already.
    w.grad sums as few as 9 products here (a corner tap, 32 pixels), where the statistical argument behind ALPHA["bf16x3"] has nothing to
    average over: with an fp32 skip tensor one of 663 552 elements came to 1.05 of its bound in a later step (0.964 in the first).  With record
    operands the only error of a product is the dropped lo * lo, at most 2^-16 of it, and the bound holds in the worst case."""
    from dffinthewild_amd import pipeline
    gen = torch.Generator().manual_seed(21)
    B, N, H, W = 1, 2, 8, 8
    x0 = torch.randn(B, 64, N, H, W, generator=gen).cuda()
    skip = sum(cg.round_parts(torch.randn(B, 64, N, H // 2, W // 2, generator=gen), "bf16x3")).cuda().requires_grad_(True)
    fd = (0.1 + 1.4 * torch.rand(B, N, 1, 1, generator=gen)).cuda()
    gt = (0.1 + 1.4 * torch.rand(B, H // 2, W // 2, generator=gen)).cuda()
    mask = (torch.rand(B, H // 2, W // 2, generator=gen) < 0.8).cuda()
    w0 = torch.nn.Parameter((0.03 * torch.randn(128, 64, 3, 3, 3, generator=gen)).cuda())
    wc = torch.nn.Parameter((0.02 * torch.randn(128, 192, 3, 3, 3, generator=gen)).cuda())
    gamma = torch.nn.Parameter((1 + 0.1 * torch.randn(128, generator=gen)).cuda())
    beta = torch.nn.Parameter((0.1 * torch.randn(128, generator=gen)).cuda())
    ws = torch.nn.Parameter((0.2 * torch.randn(1, 128, 1, 1, 1, generator=gen)).cuda())
    params = [w0, wc, gamma, beta, ws]
    opt = pipeline.Adam(params, lr=1e-3)
    for t in (1, 2, 3):
        opt.zero_grad()
        skip.grad = None
        xa = pipeline.conv3d(x0, w0, stride=(1, 2, 2), pad=1)
        xa.retain_grad()
        y = pipeline.conv3d_cat(xa, skip, wc)
        y.retain_grad()
        z = pipeline.batch_norm3d(y, gamma, beta, relu=True)
        s = pipeline.score_conv(z, ws, pad=0)
        total = pipeline.HeadsLoss.apply(s, s, s, s, fd, gt, mask)
        total.backward()
        assert tuple(y.shape) == (B, 128, N, H // 2, W // 2) and torch.equal(y.detach(), pipeline.conv3d(torch.cat([xa, skip], 1).detach(), wc, stride=1, pad=1))
        assert all(p.grad is not None and p.grad.is_cuda and p.grad.shape == p.shape for p in params)
        ra, rb, rw = cc.refs64(xa.detach().cpu(), skip.detach().cpu(), wc.detach().cpu(), y.grad.cpu())
        wa = eb.check_elementwise(xa.grad, ra, "bf16x3", "xa.grad of the chain")
        wb = eb.check_elementwise(skip.grad, rb, "bf16x3", "xb.grad of the chain")
        ww = eb.check_elementwise(wc.grad, rw, "bf16x3", "w.grad of the chain")
        assert float(y.grad.abs().max()) > 0 and float(w0.grad.abs().max()) > 0     # xa.grad reached the stride-2 conv's weight
        before = [p.detach().clone() for p in params]
        opt.step()
        assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
        print("conv_cat chain step %d: loss %.6f, err/bound xa.grad %.3f xb.grad %.3f w.grad %.3f" % (t, float(total.detach()), wa, wb, ww))
    with pytest.raises(ValueError, match="up to 128"):
        pipeline.conv3d(torch.cat([xa, skip], 1).detach().requires_grad_(True), wc, stride=1, pad=1).sum().backward()
