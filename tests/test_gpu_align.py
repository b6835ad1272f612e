"""GPU: the alignment network's feature blocks (the six resnet_block_2d_OF of FlowNetwork, End_to_End.py:135-145: of_first_kernel,
of_roll8_kernel, of_roll_kernel, of_s2_kernel, or the general convs), called one block at a time through dffw_op_of_block -- the
forward's own dispatch on a private, NaN-poisoned workspace -- and held element by element to the composed forward-error bound of
oracle/error_bounds.py (of_ref64) against a float64 reference.  Every path of each block is checked, the kernels that ran are asserted
from the op's launch list, two paths agree to twice the bound, a repeated call is bit-identical, and the forward's feature taps
(fe1, fe2, fe3) tie the op to the forward's dispatch at the End_to_End golden sizes."""
import json
import os

import numpy as np
import pytest
import torch

from dffinthewild_amd import graph, synth
from oracle import error_bounds as eb
from oracle.make_goldens_e2e import net_inputs

pytestmark = pytest.mark.gpu

PRECS = ("bf16x3", "fp16", "bf16")
WORST = {}   # (kernel family, precision) -> max err / bound seen in this module
SWITCHES = ("DFFW_NO_FUSED_OF", "DFFW_NO_OF_FIRST", "DFFW_NO_TILE", "DFFW_ROLL_MIN_UNITS", "DFFW_SRD_WGS")


@pytest.fixture(scope="module")
def eng(lib_built):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dffinthewild_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def worst_ratio_report():
    """With ERROR_BOUND_REPORT=<file>, the worst err / bound per kernel family and precision is merged into that JSON file."""
    yield
    path = os.environ.get("ERROR_BOUND_REPORT")
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for (fam, prec), v in WORST.items():
            key = "%s/%s" % (fam, prec)
            old[key] = max(old.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def family(kernels):
    """The block's distinguishing kernel: the last launch, without its template arguments ("conv" for the general convs)."""
    k = kernels[-1].split("<")[0].replace("dffw::", "")
    return k if k.startswith("of_") else "of_block_convs"


def bounded(got, r, prec, kernels, what):
    """Finite everywhere (the workspace is NaN), within the bound on every element, exactly 0 where D == 0; logs the worst ratio."""
    got = got.cpu()
    assert torch.isfinite(got).all(), (what, kernels)
    worst = eb.check_elementwise(got, r, prec, "%s %s" % (what, kernels))
    zero = r.D == 0
    assert torch.equal(got[zero], torch.zeros_like(got[zero])), (what, "non-zero where the bound is 0")
    k = (family(kernels), prec)
    WORST[k] = max(WORST.get(k, 0.0), worst)
    return worst


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def match_kernels(got, want):
    """``want`` with "conv" any single general conv launch (none of the block's fused kernels)."""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        if w == "conv":
            assert not any(s in g for s in ("of_", "head_", "ncdhw")), (got, want)
        else:
            assert g == w, (got, want)


def of_expected(block, H, W, path, pi):
    """The launches of one block on a path: "stream" (DFFW_ROLL_MIN_UNITS=1), "no_fused" (DFFW_NO_FUSED_OF), "no_first"
    (DFFW_NO_OF_FIRST).  The stride-1 streaming kernels need whole 8 x 16 columns, of_s2 whole 16 x 32 input columns."""
    cin, cout, s = block
    cols = H % 8 == 0 and W % 16 == 0 and path != "no_fused"
    cols2 = H % 16 == 0 and W % 32 == 0 and path != "no_fused"
    if block == (3, 8, 1):
        if cols and path == "stream":
            return ["dffw::of_first_kernel<%d>" % pi]
        return ["dffw::from_ncdhw_pad_kernel<%d>" % pi] + (["dffw::of_roll8_kernel<%d>" % pi] if cols else ["conv", "conv"])
    if block == (8, 8, 1) and cols:
        return ["dffw::of_roll8_kernel<%d>" % pi]
    if block == (16, 16, 1) and cols:
        return ["dffw::of_roll_kernel<%d, false>" % pi]
    if block == (8, 16, 2) and cols2:
        return ["dffw::of_s2_kernel<%d>" % pi]
    return ["conv"] * (2 if s == 1 else 3)


# (B, N, H, W, wgs) of the block's input: slice counts 1, 2, 3, 10, batch up to 4, one column per workgroup and long column streams
# (DFFW_SRD_WGS 8 / 16), and sizes that miss the streaming forms: W % 16 (24 x 40), H % 8 (20 x 32), and of_s2's W % 32 only (16 x 48)
OF_SHAPES = [(1, 10, 32, 64, 0), (2, 1, 16, 32, 8), (4, 3, 16, 32, 16), (1, 2, 32, 96, 0), (2, 3, 24, 40, 0), (1, 2, 20, 32, 8),
             (3, 1, 16, 48, 8),
             # fewer columns than XCDs at stride 1 (4; of_s2: 1), and of_s2's own remainder on 8 workgroups (3 x 3 = 9 output columns; stride 1: 36)
             (1, 2, 16, 32, 0), (3, 1, 16, 96, 8)]


def _of_case(block, shape, prec):
    """Input, weights and the float64 reference of one case (the ReLUs resolved for ``prec``)."""
    B, N, H, W, _ = shape
    cin, cout, s = block
    regime = eb.REGIMES[(OF_SHAPES.index(shape) + eb.OF_BLOCKS.index(block)) % len(eb.REGIMES)]
    x = eb.regime_input(regime, (B, cin, N, H, W), seed=B * N + cin)
    wts = eb.of_params(regime, cin, cout, seed=400 + cout + N + s)
    return x, wts, eb.of_ref64(x, *wts, s, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("block", eb.OF_BLOCKS, ids=lambda b: "%d_%d_s%d" % b)
@pytest.mark.parametrize("shape", OF_SHAPES, ids=lambda s: "B%dN%d_%dx%d_w%d" % s)
def test_of_block_every_path(eng, shape, block, prec, monkeypatch):
    B, N, H, W, wgs = shape
    cin, cout, s = block
    x, wts, r = _of_case(block, shape, prec)
    xd = x.cuda()
    pi = eng.PRECISIONS[prec]
    paths = [("stream", {}), ("no_fused", {"DFFW_NO_FUSED_OF": "1"})]
    if block == (3, 8, 1):
        paths.append(("no_first", {"DFFW_NO_OF_FIRST": "1"}))
    first = None
    for name, env in paths:
        _set(monkeypatch, dict(env, DFFW_ROLL_MIN_UNITS="1", **({"DFFW_SRD_WGS": str(wgs)} if wgs else {})))
        y = eng.op_of_block(xd, *wts, stride=s, precision=prec)
        ks = eng.op_kernels()
        match_kernels(ks, of_expected(block, H, W, name, pi))
        bounded(y, r, prec, ks, "OF %s %s" % (block, name))
        if first is None:
            first = y.cpu()
            assert torch.equal(eng.op_of_block(xd, *wts, stride=s, precision=prec), y), "repeated call differs"
        else:
            eb.check_pair(y.cpu(), first, r, prec, "OF %s %s vs stream" % (block, name))


def test_of_block_rejects_shapes_the_network_does_not_have(eng):
    x = torch.zeros(1, 8, 1, 16, 32, device="cuda")
    wts = eb.of_params("plain", 8, 32, seed=1)
    with pytest.raises((ValueError, RuntimeError), match="no alignment feature block"):
        eng.op_of_block(x, *wts, stride=2)


# ---- the forward's own dispatch: the feature taps through the op ---------------------------------------------------------------
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
P = "optical_flow_aggregation."
OF_NAMES = ("OF_feature.0", "OF_feature.1", "OF_feature1.0", "OF_feature1.1", "OF_feature2.0", "OF_feature2.1")


def _e2e_case(name):
    g = np.load(os.path.join(GOLDEN_DIR, "e2e_net_%s.npz" % name))
    entries = list(graph.param_entries(graph.e2e_convs()))
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(entries, seed=int(g["wseed"]), profile=str(g["profile"])).items()}
    FS, fd, fov = net_inputs(int(g["H"]), int(g["W"]), int(g["iseed"]))
    return sd, torch.from_numpy(FS), torch.from_numpy(fd), torch.from_numpy(fov)


def _layer_kernels(prof, prefix):
    return [k for k, layer, *_ in prof if layer == prefix or layer.startswith(prefix + ".")]


@pytest.mark.parametrize("which,min_units", [("smooth_64x96", None), ("smooth_64x96", "1"), ("smooth_480x640", None),
                                             ("smooth_480x640", "1")])
def test_of_ops_match_the_forward_taps(eng, which, min_units, monkeypatch):
    """Each level's two blocks through the op, fed the stack or the previous level's tap, give the forward's tap within twice the
    bound, launching the kernels the forward's profile shows for those layers (the default thresholds and every streaming kernel
    forced on)."""
    from dffinthewild_amd.End_to_End import Network
    _set(monkeypatch, {"DFFW_ROLL_MIN_UNITS": min_units} if min_units else {})
    sd, FS, fd, fov = _e2e_case(which)
    model = Network()
    model.load_state_dict(sd)
    model = model.cuda().eval()
    engine = model._engine_on(torch.device("cuda", torch.cuda.current_device()))
    engine.profile(True)
    try:
        with torch.no_grad():
            _, taps = model.forward_with_taps(FS.cuda(), fd.cuda(), fov.cuda(),
                                              ["fe1", "fe2", "fe3", "head3", "head2", "head1", "alpha3", "alpha2", "alpha"])
        prof = engine.profile_collect()
    finally:
        engine.profile(False)
    w = lambda k: sd[k]
    bn = lambda k: tuple(sd[k + s] for s in (".weight", ".bias", ".running_mean", ".running_var"))
    src = FS.cuda()
    for lvl, tap in enumerate(("fe1", "fe2", "fe3")):
        for j in range(2):
            name = OF_NAMES[2 * lvl + j]
            cin, cout, s = eb.OF_BLOCKS[2 * lvl + j]
            p = P + name
            wts = (w(p + ".conv.0.0.weight"), bn(p + ".conv.0.1"), w(p + ".conv.2.0.weight"), bn(p + ".conv.2.1"), w(p + ".feature.weight"))
            r = eb.of_ref64(src.cpu(), *wts, s, "bf16x3")
            y = eng.op_of_block(src, *wts, stride=s)
            ks = eng.op_kernels()
            fwd = _layer_kernels(prof, p)
            if name == "OF_feature.0":
                fwd = [k for k, layer, *_ in prof if layer == "flow.stack_in"] + fwd
            assert ks == fwd, (p, ks, fwd)
            bounded(y, r, "bf16x3", ks, "OF %s at %s" % (name, which))
            if j == 1:
                eb.check_pair(y.cpu(), taps[tap].cpu(), r, "bf16x3", "%s op vs forward tap %s (%s)" % (name, tap, which))
                # (not bit for bit: the op's block-to-block handoff goes through fp32 and is split into a record again, and about 1 %
                # of fe1 differs from the forward's in the last bits; the pair check above holds every element to twice the bound)
                print("%s: %d of %d elements differ from the forward's tap %s (%s)" % (
                    name, int((y != taps[tap]).sum()), y.numel(), tap, which))
                src = taps[tap]
            else:
                src = y
    check_alpha_taps(taps)


def check_alpha_taps(taps):
    """alpha3 / alpha2 / alpha hold the accumulated warp parameters AFTER each level's update: alpha3 = damp(head3), alpha2 = alpha3 +
    damp(head2), alpha = alpha2 + damp(head1), damp scaling the scale term (channel 0) by 0.001 (End_to_End.py:86,94,102).  The update
    is one fp32 add (perhaps fused with the damping multiply), so each identity holds to 2^-21 of |previous| + |step|; the alpha before
    the update would miss by the whole step."""
    prev = torch.zeros_like(taps["alpha"])
    for h, a in (("head3", "alpha3"), ("head2", "alpha2"), ("head1", "alpha")):
        step = taps[h].clone()
        step[:, 0] = step[:, 0] * 0.001
        tol = 2.0 ** -21 * (prev.abs() + step.abs()) + 1e-30
        assert bool(((taps[a] - (prev + step)).abs() <= tol).all()), (a, taps[a], prev + step)
        assert bool((step.abs() > 1e3 * tol).any()), (h, "the step is too small to tell before from after")
        prev = taps[a]
