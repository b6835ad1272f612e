"""dffw_loss_heads on the GPU: the training loss and the regression-head backward against tests/loss_ref.py in float64,
per gradient element under the calibrated bound ALPHA * G; the reference's own training step through the goldens; bit-identity with the
forward heads, between two runs and on a poisoned workspace; the autograd node and the drop-in module's training_loss.

GPU's worst err/G over CASES and the goldens per head (mid, pred1, pred2, pred3), in units of 2^-24, gate 32: see DESIGN.md §12."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDENS = ("plain", "ranged", "ranged_conf")


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


_ref = {}


def evaluated(key):
    """(case, float64 reference, bound) of a seeded case or a golden: computed once, shared, never modified"""
    if key not in _ref:
        if key in GOLDENS:
            case, want = L.load_golden(key)
        else:
            case, want = L.make_case(next(s for s in L.CASES if s["id"] == key)), None
        _ref[key] = (case, L.reference(case), L.bound(case), want)
    return _ref[key]


def run(eng, case, **kw):
    cu = lambda t: t.cuda() if t is not None else None
    losses, preds, grads = eng.op_loss_heads([s.cuda() for s in case["scores"]], cu(case["fd"]), cu(case["gt"]), case["mask"].cuda().view(torch.uint8),
                                             cu(case["conf"]), case["weights"], case["rng"], **kw)
    torch.cuda.synchronize()
    return losses.cpu(), [p.cpu() for p in preds] if preds else None, [g.cpu() for g in grads] if grads else None


def check(case, ref, G, losses, preds, grads, tag):
    ratios = L.worst_ratio(grads, ref["grads"], G)
    want = torch.cat([ref["per_head"], ref["total"].reshape(1)])
    lerr = float(((losses - want).abs() / want.abs()).max()) if not torch.isnan(want).any() else 0.0
    print(tag, "err/G in 2^-24 per head:", ["%.2f" % (x / L.EPS32) for x in ratios], "loss rel err %.2e" % lerr)
    assert max(ratios) <= L.ALPHA, (tag, ratios)
    if torch.isnan(want).any():
        assert torch.isnan(losses).all()
    else:
        assert lerr <= L.LOSS_RTOL, (tag, lerr)
    for a, b in zip(preds, ref["preds"]):   # test_gpu_ops.py::test_regression_head's tolerance
        assert float((a.double() - b).norm() / b.norm()) <= 2e-6


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(eng, name):
    """the reference's own training step: float64 restatement of its score volumes as the reference, and the recorded float32 values
    themselves within the sum of the two float32 runs' bounds"""
    case, ref, G, want = evaluated(name)
    losses, preds, grads = run(eng, case)
    check(case, ref, G, losses, preds, grads, name)
    assert max(L.worst_ratio(grads, [g.double() for g in want["grads"]], G)) <= 2 * L.ALPHA
    assert torch.all((losses[:5] - want["losses"].double()).abs() <= 2 * L.LOSS_RTOL * want["losses"].double().abs())


@pytest.mark.parametrize("cid", [s["id"] for s in L.CASES])
def test_cases(eng, cid):
    case, ref, G, _ = evaluated(cid)
    losses, preds, grads = run(eng, case)
    check(case, ref, G, losses, preds, grads, cid)
    spec = next(s for s in L.CASES if s["id"] == cid)
    if spec["N"] == 1 or spec["mask"] == "empty":
        assert all(float(g.abs().max()) == 0 for g in grads)      # exactly zero
    assert all(torch.isfinite(g).all() for g in grads)
    names = eng.op_kernels()
    assert names[:2] == ["dffw::loss_norm_partial", "dffw::loss_norm_finish"] and names[-1] == "dffw::loss_finish"
    want = ["dffw::loss_head_tile<%d>" % (8 >> k) if k < 3 else "dffw::loss_head_full" for k in spec.get("heads", (0, 1, 2, 3))]
    assert names[2:-1] == want


@pytest.mark.parametrize("cid", ["n10_b3_dense", "n11_underflow", "n1_32x32", "n5_conf_dense"])
def test_bit_identity(eng, cid):
    """predictions = dffw_op_regress bit for bit; two runs, a run on a poisoned workspace and runs without pred / grad give the same bits"""
    case, ref, G, _ = evaluated(cid)
    B, H, W = case["gt"].shape
    losses, preds, grads = run(eng, case)
    for s, p in zip(case["scores"], preds):
        d = eng.op_regress(s.cuda(), case["fd"].cuda(), H, W).cpu()
        print(cid, tuple(s.shape), "pixels that differ from op_regress:", int((d != p).sum()), "max |diff| %.3g" % float((d - p).abs().max()))
        assert torch.equal(d, p)
    ws = torch.full((eng.loss_workspace_bytes(B, case["scores"][0].shape[1], H, W),), 0xFF, dtype=torch.uint8, device="cuda")
    l2, p2, g2 = run(eng, case, workspace=ws)
    same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert same(preds, p2) and same(grads, g2) and torch.equal(losses.view(torch.int64), l2.view(torch.int64))
    l3, p3, g3 = run(eng, case, preds=False)
    assert p3 is None and same(grads, g3) and torch.equal(losses.view(torch.int64), l3.view(torch.int64))
    l4, p4, g4 = run(eng, case, grads=False)
    assert g4 is None and same(preds, p4) and torch.equal(losses.view(torch.int64), l4.view(torch.int64))


def test_invalid_arguments(eng):
    case = evaluated("n5_conf_dense")[0]
    bad = dict(case, scores=[case["scores"][0][:, :, :, :-1]] + case["scores"][1:])
    with pytest.raises(ValueError):
        run(eng, bad)
    with pytest.raises(Exception):
        run(eng, case, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        run(eng, dict(case, rng=(2.0, 2.0)))


def test_heads_loss_autograd(eng):
    """HeadsLoss: total and the four gradients, scaled by the incoming gradient, against loss_ref (not numerical differentiation)."""
    from dffinthewild_amd import pipeline
    case, ref, G, _ = evaluated("n5_conf_dense")
    scores = [s.cuda().requires_grad_(True) for s in case["scores"]]
    total = pipeline.HeadsLoss.apply(*scores, case["fd"].cuda(), case["gt"].cuda(), case["mask"].cuda(), case["conf"].cuda(), case["weights"], case["rng"])
    (3.0 * total).backward()
    assert abs(float(total) - float(ref["total"])) <= (L.LOSS_RTOL + L.EPS32) * float(ref["total"])     # + the rounding of the total to float32
    got = [s.grad.cpu() for s in scores]
    # + the float32 rounding of 3 * g (|g| <= G: every factor of E bounds the factor of the gradient it stands for)
    assert max(L.worst_ratio(got, [3.0 * g for g in ref["grads"]], [3.0 * g for g in G])) <= L.ALPHA + L.EPS32
    t2, per, preds, grads = pipeline.training_loss([s.detach() for s in scores], case["fd"].cuda(), case["gt"].cuda(), case["mask"].cuda(),
                                                   case["conf"].cuda(), case["weights"], case["rng"], grads=False)
    assert grads is None and t2.is_cuda and per.is_cuda and per.shape == (4,) and len(preds) == 4
    assert abs(float(t2) - float(ref["total"])) <= L.LOSS_RTOL * float(ref["total"])


def test_network_training_loss(eng, golden_dir):
    """Network.training_loss = forward with the four score taps + pipeline.training_loss, bit for bit (den_tiny_taps size)."""
    from dffinthewild_amd import graph, pipeline, synth
    from dffinthewild_amd.Depth_Estimation_Network import Network
    g = np.load(os.path.join(golden_dir, "den_tiny_taps.npz"))
    B, N, H, W = (int(g[k]) for k in ("B", "N", "H", "W"))
    entries = list(graph.param_entries(graph.dff_net_convs()))
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(entries, g["wseed"].item(), g["profile"].item()).items()}
    model = Network()
    model.load_state_dict(sd)
    model = model.cuda().eval()
    FS = torch.from_numpy(synth.focal_stack(B, N, H, W, seed=g["iseed"].item())).cuda()
    fd = torch.from_numpy(synth.focus_dists(B, N, 1, 1)).cuda()
    gen = torch.Generator().manual_seed(5)
    gt = (0.1 + 1.4 * torch.rand(B, H, W, generator=gen)).cuda()
    mask = (torch.rand(B, H, W, generator=gen) < 0.7).cuda()
    with torch.no_grad():
        total, per, preds, grads = model.training_loss(FS, fd, gt, mask)
        outs, taps = model.forward_with_taps(FS, fd, ["conf", "cost1", "cost2", "cost3"])
        t2, per2, preds2, grads2 = pipeline.training_loss([taps[k] for k in ("conf", "cost1", "cost2", "cost3")], fd, gt, mask)
    torch.cuda.synchronize()
    assert torch.equal(total, t2) and torch.equal(per, per2) and torch.isfinite(total)
    assert all(torch.equal(a, b) for a, b in zip(preds, preds2)) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert [tuple(x.shape) for x in grads] == [tuple(taps[k].shape) for k in ("conf", "cost1", "cost2", "cost3")]
