"""The enqueue-only record forms a training step calls -- dffw_conv_wgrad, dffw_bn_train_forward, dffw_bn_train_backward (DESIGN.md sections 13, 14) --
called as a training step would: on activation records [pixel][part][channel] built by the caller (conv_grad_ref.to_records), with the caller's
workspace of exactly *_workspace_bytes() and on a side stream, without a host synchronisation between the calls.

Every device buffer the library writes is a slice of one uint8 tensor filled with 0xFF, at a 256-byte-aligned offset with at least 4 KiB of
guard on both sides (Guarded); after the final synchronisation every byte outside the slices must still be 0xFF.  The results are compared
bit for bit with the op forms (which stage the same records from the fp32 tensors and call the same record functions) and held to the bounds
of tests/conv_grad_ref.py and tests/bn_ref.py."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402
import conv_grad_ref as cg  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402

pytestmark = pytest.mark.gpu

PREC_ID = {"bf16x3": 0, "fp16": 1, "bf16": 2}
SHAPE = (2, 3, 12, 20)     # (B, N, H, W): both slice paddings, ragged tile edges, B > 1
GUARD, ALIGN = 4096, 256


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


class Guarded:
    """Named slices of one 0xFF-filled uint8 device tensor: each at an ALIGN-ed offset, with at least GUARD bytes of 0xFF before and after it."""

    def __init__(self, sizes):
        self.at, off = {}, GUARD
        for name, n in sizes.items():
            self.at[name] = (off, int(n))
            off = -(-(off + int(n) + GUARD) // ALIGN) * ALIGN
        self.buf = torch.full((off,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % ALIGN == 0

    def raw(self, name):
        off, n = self.at[name]
        return self.buf[off:off + n]

    def ptr(self, name):
        return ctypes.c_void_p(self.raw(name).data_ptr())

    def view(self, name, dtype, shape):
        return self.raw(name).view(dtype).reshape(shape)

    def check(self):
        """Every byte outside the slices is still 0xFF (call after the stream has drained)."""
        host = self.buf.cpu()
        outside = torch.ones(host.numel(), dtype=torch.bool)
        for off, n in self.at.values():
            assert off % ALIGN == 0 and bool(outside[off - GUARD:off].all())
            outside[off:off + n] = False
        for name, (off, n) in self.at.items():
            assert bool(outside[off + n:off + n + GUARD].all()), name
            before, after = host[off - GUARD:off], host[off + n:off + n + GUARD]
            assert bool((before == 0xFF).all()), "%s: %d bytes written below the buffer" % (name, int((before != 0xFF).sum()))
            assert bool((after == 0xFF).all()), "%s: %d bytes written beyond the buffer" % (name, int((after != 0xFF).sum()))
        assert bool((host[outside] == 0xFF).all())


def i3(v):
    return (ctypes.c_int * 3)(*v)


def side_stream():
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())     # the inputs were written on the current stream
    return s, ctypes.c_void_p(s.cuda_stream)


def nbytes_records(prec, B, C, N, H, W):
    return B * N * H * W * (2 if prec == "bf16x3" else 1) * C * 2


def wgrad_on_records(eng, geom, prec, x, gy, wshape, fill=0xFF):
    """dffw_conv_wgrad on the records of x and gy, on a side stream, workspace and grad_w guarded; returns grad_w (a copy) after the checks."""
    k, s, p, t = cg.GEOMETRIES[geom]
    B, cin, N, H, W = x.shape
    cout = gy.shape[1]
    dev = torch.cuda.current_device()
    xr, gyr = cg.to_records(x, prec).cuda(), cg.to_records(gy, prec).cuda()
    wsb = eng.lib.dffw_conv_wgrad_workspace_bytes(B, cin, N, H, W, cout, i3(k), i3(s), i3(p), int(t))
    assert wsb > 0
    nw = 1
    for d in wshape:
        nw *= d
    G = Guarded(dict(ws=wsb, gw=4 * nw))
    G.raw("ws").fill_(fill)
    stream, sp = side_stream()
    rc = eng.lib.dffw_conv_wgrad(dev, PREC_ID[prec], xr.data_ptr(), B, cin, N, H, W, gyr.data_ptr(), cout, i3(k), i3(s), i3(p), int(t),
                                 G.ptr("gw"), G.ptr("ws"), wsb, sp)
    assert rc == 0, eng.lib.dffw_last_error().decode()
    S = 2 if s[1] == 2 else 1
    assert eng.op_kernels() == ["dffw::conv_wgrad_kernel<%d, %d>" % (PREC_ID[prec], S), "dffw::conv_wgrad_finish_kernel"]
    stream.synchronize()
    G.check()
    return G.view("gw", torch.float32, wshape).clone()


@pytest.mark.parametrize("prec", cg.PRECISIONS)
@pytest.mark.parametrize("geom,pair", [(g, (16, 32)) for g in cg.GEOMETRIES] + [("k333", (40, 24))], ids=lambda v: v if isinstance(v, str) else "%dto%d" % v)
def test_wgrad_record_form(eng, geom, pair, prec):
    """dffw_conv_wgrad on caller-built records, a workspace of exactly dffw_conv_wgrad_workspace_bytes() and a side stream: rc 0, the two
    launches, nothing written outside workspace and grad_w, grad_w bit-identical to op_conv3d_backward on the same fp32 tensors (the op form
    stages the same records and calls the same function) and under ALPHA * G.  A workspace of zeros gives the same bits as one of 0xFF."""
    cin, cout = pair
    B, N, H, W = SHAPE
    x, w, gy = cg.make_case("zero_mean", geom, B, cin, cout, N, H, W, seed=3 + cin + 5 * cout)
    gw = wgrad_on_records(eng, geom, prec, x, gy, tuple(w.shape))
    _, s, p, t = cg.GEOMETRIES[geom]
    _, op_gw = eng.op_conv3d_backward(x.cuda(), w, gy.cuda(), stride=s, pad=p, transposed=t, precision=prec, need=("w",))
    assert torch.equal(gw, op_gw)
    worst = eb.check_elementwise(gw, cg.wgrad_ref64(x, gy, geom, tuple(w.shape)), prec, "grad_w of the record form")
    print("wgrad record form %s %s %d->%d %s: grad_w err/bound %.3f" % (geom, prec, cin, cout, SHAPE, worst))
    assert torch.equal(wgrad_on_records(eng, geom, prec, x, gy, tuple(w.shape), fill=0x00), gw)


# ---- one conv -> BN(+skip, ReLU) layer's training calls on one stream ------------------------------------------------------------------------
C0, C1 = 8, 16     # the conv's input channels; its output channels = the BatchNorm's


def chain_inputs(prec):
    """fp32 CPU tensors that ARE record values (hi + lo of their own records), so that staging them again gives the same records."""
    B, N, H, W = SHAPE
    g = torch.Generator().manual_seed(53)
    rd = lambda t: R.rounded(t, prec)
    c = dict(x0=rd(torch.rand(B, C0, N, H, W, generator=g) * 2 - 1), x=rd(torch.randn(B, C1, N, H, W, generator=g)),
             res=rd(torch.randn(B, C1, N, H, W, generator=g)), gy=rd(torch.randn(B, C1, N, H, W, generator=g)),
             gamma=(0.5 + torch.rand(C1, generator=g)) * torch.where(torch.rand(C1, generator=g) < 0.25, -1.0, 1.0), beta=torch.rand(C1, generator=g) - 0.5,
             rm0=torch.randn(C1, generator=g) * 0.5, rv0=0.5 + torch.rand(C1, generator=g))
    for k in ("x0", "x", "res", "gy"):
        assert torch.equal(rd(c[k]), c[k])
    return c


def run_chain(eng, prec, c, shared_workspace, fill):
    """bn_train_forward -> bn_train_backward -> conv_wgrad (grad_y = the grad_x records the BatchNorm backward wrote), enqueued back to back on one
    side stream; one host synchronisation at the end.  ``shared_workspace``: the three calls use ONE workspace buffer (the largest need) in
    stream order, else each its own of exactly its *_workspace_bytes()."""
    lib, dev, P = eng.lib, torch.cuda.current_device(), PREC_ID[prec]
    B, N, H, W = SHAPE
    k, s, p, t = cg.GEOMETRIES["k333"]
    wshape = cg.weight_shape("k333", C0, C1)
    rec = {n: cg.to_records(c[n], prec).cuda() for n in ("x0", "x", "res", "gy")}
    gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
    bn_b = lib.dffw_bn_train_workspace_bytes(B, C1, N, H, W)
    wg_b = lib.dffw_conv_wgrad_workspace_bytes(B, C0, N, H, W, C1, i3(k), i3(s), i3(p), int(t))
    assert bn_b > 0 and wg_b > 0
    nrec, vec = nbytes_records(prec, B, C1, N, H, W), 4 * C1
    sizes = dict(y=nrec, gx=nrec, gres=nrec, mean=vec, invstd=vec, rm=vec, rv=vec, dgamma=vec, dbeta=vec, gw=4 * C1 * C0 * 27)
    sizes.update(dict(ws=max(bn_b, wg_b)) if shared_workspace else dict(ws_fwd=bn_b, ws_bwd=bn_b, ws_wgrad=wg_b))
    G = Guarded(sizes)
    ws = (lambda n: "ws") if shared_workspace else (lambda n: "ws_" + n)
    for n in set(ws(n) for n in ("fwd", "bwd", "wgrad")):
        G.raw(n).fill_(fill)
    G.view("rm", torch.float32, (C1,)).copy_(c["rm0"])
    G.view("rv", torch.float32, (C1,)).copy_(c["rv0"])
    stream, sp = side_stream()
    rc = lib.dffw_bn_train_forward(dev, P, rec["x"].data_ptr(), B, C1, N, H, W, gamma.data_ptr(), beta.data_ptr(), R.BN_EPS, R.MOMENTUM, G.ptr("rm"), G.ptr("rv"),
                                   rec["res"].data_ptr(), 1, G.ptr("y"), G.ptr("mean"), G.ptr("invstd"), G.ptr(ws("fwd")), bn_b, sp)
    assert rc == 0, lib.dffw_last_error().decode()
    fwd = eng.op_kernels()
    rc = lib.dffw_bn_train_backward(dev, P, rec["x"].data_ptr(), G.ptr("y"), rec["gy"].data_ptr(), B, C1, N, H, W, gamma.data_ptr(), G.ptr("mean"), G.ptr("invstd"), 1,
                                    G.ptr("gx"), G.ptr("gres"), G.ptr("dgamma"), G.ptr("dbeta"), G.ptr(ws("bwd")), bn_b, sp)
    assert rc == 0, lib.dffw_last_error().decode()
    bwd = eng.op_kernels()
    rc = lib.dffw_conv_wgrad(dev, P, rec["x0"].data_ptr(), B, C0, N, H, W, G.ptr("gx"), C1, i3(k), i3(s), i3(p), int(t), G.ptr("gw"), G.ptr(ws("wgrad")), wg_b, sp)
    assert rc == 0, lib.dffw_last_error().decode()
    wgk = eng.op_kernels()
    stream.synchronize()      # the only host synchronisation
    G.check()
    assert fwd == ["dffw::bn_stats_kernel<%d>" % P, "dffw::bn_stats_finish_kernel", "dffw::bn_apply_kernel<%d, 1, 1>" % P]
    assert bwd == ["dffw::bn_bwd_reduce_kernel<%d, 1>" % P, "dffw::bn_bwd_finish_kernel", "dffw::bn_bwd_apply_kernel<%d, 1, 1>" % P]
    assert wgk == ["dffw::conv_wgrad_kernel<%d, 1>" % P, "dffw::conv_wgrad_finish_kernel"]
    parts = 2 if prec == "bf16x3" else 1
    records = lambda n: G.view(n, torch.int16, (B, N, H, W, parts, C1)).cpu()
    out = {n: cg.from_records(records(n), prec, C1) for n in ("y", "gx", "gres")}
    out.update({n: G.view(n, torch.float32, (C1,)).cpu().clone() for n in ("mean", "invstd", "rm", "rv", "dgamma", "dbeta")})
    out["gw"] = G.view("gw", torch.float32, wshape).cpu().clone()
    out["gx_records"] = records("gx")
    return out


@pytest.mark.parametrize("prec", cg.PRECISIONS)
def test_layer_chain_on_records(eng, prec):
    """One conv -> BN(+skip, ReLU) layer's training calls on records, enqueued on one side stream without a host synchronisation in between:
    dffw_bn_train_forward (ReLU, residual, running statistics), dffw_bn_train_backward, then dffw_conv_wgrad (k333, 8 -> 16) reading the grad_x
    records the BatchNorm backward has just written.

    Run 1 gives every call its own workspace of exactly its *_workspace_bytes(), filled with 0xFF; run 2 goes into fresh buffers with ONE
    workspace shared by the three calls in stream order, filled with 0x00.  Both runs: guards intact, identical bits (the workspace need not
    be cleared, and may be reused).

    Against the op forms, stage by stage on from_records of the same tensors: y, save_mean, save_invstd, the running statistics, grad_x,
    grad_res, grad_gamma, grad_beta bit for bit (the inputs are record values, so the op shell stages the very same records and calls the same
    record function; of y the backward reads only the sign).  grad_w bit for bit in fp16 and bf16.  The deliberate exception: in split-bf16 the op
    form re-splits the fp32 grad_x, and where lo had rounded up to exactly half an ulp of hi the re-split picks the other (hi, lo) pair of the same
    value (about one record value in 2^10), whose three MFMA products differ in the last bits; there grad_w is held to its bound only.  The
    BatchNorm quantities are also under bn_ref's bounds, grad_w under ALPHA * G evaluated at the GPU's own grad_x."""
    c = chain_inputs(prec)
    a = run_chain(eng, prec, c, shared_workspace=False, fill=0xFF)
    b = run_chain(eng, prec, c, shared_workspace=True, fill=0x00)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(cg.to_records(a["gx"], prec), a["gx_records"]) or prec == "bf16x3"      # one part: the re-split is the identity
    # the op forms, stage by stage
    x, res, gy, gamma, beta = (c[k].cuda() for k in ("x", "res", "gy", "gamma", "beta"))
    rm, rv = c["rm0"].cuda().clone(), c["rv0"].cuda().clone()
    y, mean, invstd = eng.op_bn_train(x, gamma, beta, rm, rv, residual=res, relu=True, precision=prec)
    gx, gres, dgamma, dbeta = eng.op_bn_train_backward(x, y, gy, gamma, mean, invstd, relu=True, residual=True, precision=prec)
    op = dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, gx=gx, gres=gres, dgamma=dgamma, dbeta=dbeta)
    for k in R.QUANTITIES:
        assert torch.equal(a[k], op[k].cpu()), k
    _, s, p, t = cg.GEOMETRIES["k333"]
    wshape = cg.weight_shape("k333", C0, C1)
    _, op_gw = eng.op_conv3d_backward(c["x0"].cuda(), torch.zeros(wshape), a["gx"].cuda(), stride=s, pad=p, transposed=t, precision=prec, need=("w",))
    if prec != "bf16x3":
        assert torch.equal(a["gw"], op_gw.cpu())
    # the bounds
    case = dict(x=c["x"], gamma=c["gamma"], beta=c["beta"], res=c["res"], gy=c["gy"], rm0=c["rm0"], rv0=c["rv0"])
    r = R.reference(case, prec, True, True, y_stored=a["y"])
    n, ok = R.mask_disagreements(a["y"], r, prec)
    q = R.ratios(a, r, prec)
    rw = cg.wgrad_ref64(c["x0"], a["gx"], "k333", wshape)
    ww = eb.check_elementwise(a["gw"], rw, prec, "grad_w behind the BatchNorm backward")
    wo = eb.check_elementwise(op_gw, rw, prec, "grad_w of the op form")
    print("layer chain on records %s %s: masks differ at %d; err/bound %s grad_w %.3f (op form %.3f)" %
          (prec, SHAPE, n, " ".join("%s %.3f" % kv for kv in q.items()), ww, wo))
    assert ok and set(q) == set(R.QUANTITIES) and max(q.values()) <= 1.0, q
    assert float(a["gw"].abs().max()) > 0 and float(a["gres"].abs().max()) > 0
