"""dffw_heads_backward and pipeline.regress_heads on the GPU: the gradient of the regression heads under any upstream gradient
against tests/heads_grad_ref.py in float64, per element under the calibrated bound ALPHA * G; exact zeros, linearity and repeatability
bit for bit; guarded output buffers on a side stream; the forward's bits; the training scripts' loss written in torch against the loss
goldens; the autograd plumbing; refusals; the ABI.

GPU's worst err/G over SPECS x KINDS per head (mid, pred1, pred2, pred3), in units of 2^-24, gate 64: see DESIGN.md §22."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_grad_ref as R  # noqa: E402
import loss_ref as L  # noqa: E402
from test_gpu_train_records import Guarded, side_stream  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
EINVAL = -1


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def run(eng, case, gps, **kw):
    B, H, W = case["gt"].shape
    grads = eng.op_heads_backward([s.cuda() for s in case["scores"]], case["fd"].cuda(), [g.cuda() if g is not None else None for g in gps], H, W, **kw)
    torch.cuda.synchronize()
    return [g.cpu() if g is not None else None for g in grads]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [s["id"] for s in R.SPECS])
def test_bound(eng, cid):
    """every case x gradient kind, all heads, every element within ALPHA * G (0 where G is 0)"""
    heads = R.spec_of(cid).get("heads", (0, 1, 2, 3))
    for kind in R.KINDS:
        case, gps, ref, G = R.evaluated(cid, kind)
        grads = run(eng, case, gps)
        ratios = R.worst_ratio(grads, ref, G)
        print(cid, kind, "err/G in 2^-24 per head:", ["%.2f" % (x / R.EPS32) for x in ratios])
        assert max(ratios) <= R.ALPHA, (cid, kind, ratios)
        assert eng.op_kernels() == ["dffw::heads_grad_tile<%d>" % (8 >> k) if k < 3 else "dffw::heads_grad_full" for k in heads]


# ---- exact results -----------------------------------------------------------------------------------------------------------------------
def test_one_slice_is_zero(eng):
    for kind in ("dense", "big"):
        case, gps, _, _ = R.evaluated("n1_32x32", kind)
        assert all(float(g.abs().max()) == 0 for g in run(eng, case, gps))


@pytest.mark.parametrize("cid", ["n10_b3_dense", "n11_underflow", "n3_b2_8x8"])
def test_zero_gradient_gives_zeros(eng, cid):
    case, gps, _, _ = R.evaluated(cid, "dense")
    grads = run(eng, case, [torch.zeros_like(g) for g in gps])
    assert all(float(g.abs().max()) == 0 for g in grads)


@pytest.mark.parametrize("cid", ["n5_conf_dense", "n10_b3_dense", "n17_dense", "n3_b2_8x8"])
def test_linear_and_repeatable(eng, cid):
    """two calls give the same bits; grad(2 gp) = 2 grad(gp) bit for bit: a power of two commutes with every rounding short of underflow, so
    this half is asked where sigmoid stays normal (scores within +-30, not the +-100 of n17_dense)"""
    case, gps, _, _ = R.evaluated(cid, "dense")
    g1 = run(eng, case, gps)
    assert same_bits(g1, run(eng, case, gps))
    if R.spec_of(cid)["scale"] <= 30:
        assert same_bits([2 * g for g in g1], run(eng, case, [2 * g for g in gps]))


# ---- buffers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["n11_underflow", "n3_b2_8x8", "one_head"])
def test_guarded_buffers_on_a_side_stream(eng, cid):
    """the gradients written into slices of one 0xFF-filled tensor, enqueued on a side stream and synchronised once: guards intact, no 0xFF
    word left inside a slice (every element is written), and the bits of the plain call"""
    case, gps, _, _ = R.evaluated(cid, "dense")
    B, H, W = case["gt"].shape
    scores, fd, dgps = [s.cuda() for s in case["scores"]], case["fd"].cuda(), [g.cuda() for g in gps]
    mem = Guarded({"g%d" % k: s.numel() * 4 for k, s in enumerate(scores)})
    out = [mem.view("g%d" % k, torch.float32, tuple(s.shape)) for k, s in enumerate(scores)]
    stream, _ = side_stream()
    with torch.cuda.stream(stream):
        got = eng.op_heads_backward(scores, fd, dgps, H, W, out=out)
    stream.synchronize()
    mem.check()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    for k, o in enumerate(out):
        assert int((o.view(torch.int32) == -1).sum()) == 0, "head %d: elements left unwritten" % k
    assert same_bits([o.cpu() for o in out], run(eng, case, gps))


# ---- forward unchanged -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["n1_32x32", "n5_conf_dense", "n10_b3_dense", "n11_underflow"])
def test_forward_bits(eng, cid):
    """regress_heads' maps are dffw_op_regress's, bit for bit: N = 1, 5, 10, 11, dense and (B,N,1,1) focus distances"""
    from dffinthewild_amd import pipeline
    case = R.evaluated(cid, "dense")[0]
    B, H, W = case["gt"].shape
    scores, fd = [s.cuda().requires_grad_(True) for s in case["scores"]], case["fd"].cuda()
    maps = pipeline.regress_heads(scores, fd)
    assert isinstance(maps, tuple) and len(maps) == 4 and all(m.requires_grad and tuple(m.shape) == (B, H, W) for m in maps)
    for s, m in zip(scores, maps):
        assert torch.equal(m.detach().view(torch.int32), eng.op_regress(s.detach(), fd, H, W).view(torch.int32))


# ---- the scripts' loss written in torch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("plain", "ranged", "ranged_conf"))
def test_training_loss_in_torch(eng, name):
    """the reference's training step with the loss of train_code_*.py in float32 torch ops on the maps of regress_heads: the gradients within
    (loss_ref.ALPHA + ALPHA) * loss_ref.bound of the golden ones (the golden's own float32 run, plus this node's; loss_ref.bound dominates
    this issue's G element by element, |d - gt| <= |d| + |gt|), the total within loss_ref.LOSS_RTOL"""
    from dffinthewild_amd import pipeline
    case, want = L.load_golden(name)
    scores = [s.cuda().requires_grad_(True) for s in case["scores"]]
    fd, gt, mask = case["fd"].cuda(), case["gt"].cuda(), case["mask"].cuda()
    c = case["conf"].cuda()[mask] if case["conf"] is not None else torch.ones(int(mask.sum()), device="cuda")
    r = L._range(case, torch.float32).cuda()
    maps = pipeline.regress_heads(scores, fd)
    total = sum(w * ((c * ((d[mask] - gt[mask]) / r) ** 2).sum() / c.sum()) for w, d in zip(case["weights"], maps))
    total.backward()
    torch.cuda.synchronize()
    ratios = L.worst_ratio([s.grad.cpu() for s in scores], [g.double() for g in want["grads"]], L.bound(case))
    lerr = abs(float(total) - float(want["losses"][-1])) / abs(float(want["losses"][-1]))
    print(name, "err/G(loss_ref) in 2^-24 per head:", ["%.2f" % (x / L.EPS32) for x in ratios], "total rel err %.2e" % lerr)
    assert max(ratios) <= L.ALPHA + R.ALPHA
    assert lerr <= L.LOSS_RTOL


# ---- autograd plumbing -------------------------------------------------------------------------------------------------------------------
def test_only_used_heads_are_launched(eng):
    from dffinthewild_amd import pipeline
    case, gps, ref, G = R.evaluated("n5_conf_dense", "dense")
    scores = [s.cuda().requires_grad_(True) for s in case["scores"]]
    maps = pipeline.regress_heads(scores, case["fd"].cuda())
    ((maps[1] * gps[1].cuda()).sum() + (maps[3] * gps[3].cuda()).sum()).backward()
    # engine.op_kernels() as the backward's own thread sees it: autograd runs it on a thread of its own, and the launch list is per thread
    assert pipeline.RegressHeads.backward_kernels == ["dffw::heads_grad_tile<4>", "dffw::heads_grad_full"]
    assert scores[0].grad is None and scores[2].grad is None
    got = [scores[1].grad.cpu(), scores[3].grad.cpu()]
    assert max(R.worst_ratio(got, [ref[1], ref[3]], [G[1], G[3]])) <= R.ALPHA


def test_score_without_requires_grad_gets_none(eng):
    from dffinthewild_amd import pipeline
    case, gps, ref, G = R.evaluated("n5_conf_dense", "dense")
    scores = [s.cuda().requires_grad_(k != 2) for k, s in enumerate(case["scores"])]
    maps = pipeline.regress_heads(scores, case["fd"].cuda())
    sum((m * g.cuda()).sum() for m, g in zip(maps, gps)).backward()
    assert scores[2].grad is None and len(pipeline.RegressHeads.backward_kernels) == 3
    for k in (0, 1, 3):
        assert max(R.worst_ratio([scores[k].grad.cpu()], [ref[k]], [G[k]])) <= R.ALPHA
    # an upstream gradient that is not contiguous is made so
    scores[3].grad = None
    maps = pipeline.regress_heads(scores[3:], case["fd"].cuda())
    strided = gps[3].cuda().transpose(1, 2).contiguous().transpose(1, 2)
    assert not strided.is_contiguous()
    maps[0].backward(strided)
    assert max(R.worst_ratio([scores[3].grad.cpu()], [ref[3]], [G[3]])) <= R.ALPHA


def test_refusals_in_the_forward(eng):
    from dffinthewild_amd import pipeline
    case = R.evaluated("n2_b3_ranged_nan", "dense")[0]
    scores, fd = [s.cuda() for s in case["scores"]], case["fd"].cuda()
    with pytest.raises(ValueError, match="focus_dists"):
        pipeline.regress_heads([s.clone().requires_grad_(True) for s in scores], fd.clone().requires_grad_(True))
    odd = torch.randn(3, 2, 12, 20, device="cuda")
    with pytest.raises(ValueError, match=r"scores\[1\].*12x20"):
        pipeline.regress_heads([scores[3].clone().requires_grad_(True), odd.clone().requires_grad_(True)], fd, size=(32, 32))
    maps = pipeline.regress_heads([scores[3].clone().requires_grad_(True), odd], fd, size=(32, 32))   # without requires_grad it runs
    assert torch.equal(maps[1].detach(), eng.op_regress(odd, fd, 32, 32)) and maps[0].requires_grad
    maps[0].sum().backward()
    assert pipeline.RegressHeads.backward_kernels == ["dffw::heads_grad_full"]


# ---- invalid arguments -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(eng):
    """every refusal is DFFW_EINVAL, decided before the GPU is touched, and leaves the launch list empty"""
    B, N, H, W = 2, 3, 32, 32
    scores = [torch.zeros(B, N, H >> (3 - k), W >> (3 - k), device="cuda") for k in range(4)]
    gps = [torch.zeros(B, H, W, device="cuda") for _ in range(4)]
    outs = [torch.zeros_like(s) for s in scores]
    fd = torch.ones(B, N, 1, 1, device="cuda")
    arr = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in ts])
    ok = dict(n=4, score=arr(scores), h=(ctypes.c_int * 4)(4, 8, 16, 32), w=(ctypes.c_int * 4)(4, 8, 16, 32), B=B, N=N, H=H, W=W, fd=ctypes.c_void_p(fd.data_ptr()),
              st=(ctypes.c_int64 * 4)(N, 1, 0, 0), gp=arr(gps), gs=arr(outs))

    def call(**kw):
        a = dict(ok, **kw)
        rc = eng.lib.dffw_heads_backward(0, a["n"], a["score"], a["h"], a["w"], a["B"], a["N"], a["H"], a["W"], a["fd"], a["st"], a["gp"], a["gs"], None)
        return rc, eng.lib.dffw_last_error().decode()

    bad = [dict(n=0), dict(n=5), dict(score=None), dict(h=None), dict(w=None), dict(fd=None), dict(st=None), dict(gp=None), dict(gs=None),
           dict(score=arr([scores[0], None, scores[2], scores[3]])), dict(B=0), dict(N=0), dict(H=0), dict(W=0), dict(B=65536),
           dict(H=65536, W=32768), dict(h=(ctypes.c_int * 4)(4, 12, 16, 32), w=(ctypes.c_int * 4)(4, 20, 16, 32)),
           dict(h=(ctypes.c_int * 4)(4, 8, 16, 0)), dict(h=(ctypes.c_int * 4)(2, 8, 16, 32), w=(ctypes.c_int * 4)(2, 8, 16, 32)),
           dict(gp=arr([gps[0], None, gps[2], gps[3]])), dict(gs=arr([outs[0], outs[1], None, outs[3]]))]
    for kw in bad:
        assert call()[0] == 0 and len(eng.op_kernels()) == 4      # a served call in between: the list is not empty before the refusal
        rc, msg = call(**kw)
        assert rc == EINVAL and msg, (sorted(kw), rc, msg)
        assert eng.op_kernels() == [], sorted(kw)
    assert "n_heads 5 not in 1..4" in call(n=5)[1] and "null argument" in call(fd=None)[1] and "score[1] is null" in call(score=bad[9]["score"])[1]
    assert "at most 65535 samples" in call(B=65536)[1] and "does not fit 31 bits" in call(H=65536, W=32768)[1]
    assert "is not 32x32 divided by 1, 2, 4 or 8" in call(**bad[16])[1]
    # both entries null: the head is skipped
    rc, _ = call(gp=arr([gps[0], None, None, gps[3]]), gs=arr([outs[0], None, None, outs[3]]))
    assert rc == 0 and eng.op_kernels() == ["dffw::heads_grad_tile<8>", "dffw::heads_grad_full"]
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.op_heads_backward(scores, fd, gps[:3], H, W)
    with pytest.raises(ValueError):
        eng.op_heads_backward([scores[0][:, :, :, :-1]] + scores[1:], fd, gps, H, W)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi(eng):
    header = open(os.path.join(ROOT, "include", "dffw.h")).read()
    assert "int dffw_heads_backward(" in header and "dffw_heads_backward" in eng.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(eng.LIB_PATH), "dffw_heads_backward")
