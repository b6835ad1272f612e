"""GPU: the front half of the alignment network's alpha heads (head_first_conv() of csrc/dffw_align.cpp: the FOV warp of the level features and
the head's first conv over [warped ref | warped cur | flow]), one call at a time through dffw_op_head_front -- the forward's own dispatch
on a private, NaN-poisoned workspace -- and fov_warp_kernel through dffw_op_fov_warp, held element by element to the bounds of
tests/head_front_ref.py against its float64 reference, in all three arithmetics.  No element is left out: a float32 sample position on the
other side of an integer than the reference's is inside the bound.

Forms (head_front_ref.FORMS) and how they are reached, the switches read per call:
  warp    C = 8 / 16 on whole 8 x 16 columns, B N <= 320, DFFW_ROLL_MIN_UNITS=1: flow_volume_kernel (mode 2), conv .0.0#ref, head_warp_kernel<P, C>
  split   DFFW_NO_HEAD_WARP=1, or C = 32, sizes off the columns, B N > 320: flow_volume_kernel (modes 2 and 1, one profile record for the
          two launches), conv .0.0#ref, conv .0.0#cur with the slice-broadcast residual
  whole   DFFW_NO_HEAD_SPLIT=1: flow_volume_kernel (mode 0), conv .0.0 over [ref | cur | flow | pad]
(DFFW_NO_SMALL=1 on the forced forms, as the whole-network test sets it for the partner; where the warp form does not apply the split form
is also run under the warp form's switches: what the dispatch then takes by itself.)
Every call: y0 inside one 0xFF-filled buffer with guards; finite, |got - ref| <= E on every element, the launch list the form's, a second
call bit-identical, the guards intact.  Every pair of forms on one input agrees within the sum of their bounds."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_front_ref as hf  # noqa: E402
from test_gpu_train_records import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = hf.PRECISIONS
SWITCHES = ("DFFW_NO_HEAD_WARP", "DFFW_NO_HEAD_SPLIT", "DFFW_NO_SMALL", "DFFW_ROLL_MIN_UNITS", "DFFW_SRD_WGS", "DFFW_NO_TILE", "DFFW_NO_ROLL", "DFFW_NO_SLICE32")
WORST = {}                             # (what, precision) -> max err / E seen in this module
SEEN = {p: set() for p in PRECS}       # precision -> every kernel name an op of this module launched
FORMS_SEEN = {p: set() for p in PRECS}  # precision -> (form, C) whose launch list was asserted


@pytest.fixture(scope="module")
def eng(lib_built):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dffinthewild_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def worst_ratio_report():
    """With ERROR_BOUND_REPORT=<file>, the worst err / E per form and precision is merged into that JSON file."""
    yield
    path = os.environ.get("ERROR_BOUND_REPORT")
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for (what, prec), v in WORST.items():
            key = "head_front %s/%s" % (what, prec)
            old[key] = max(old.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def is_conv(name):
    """A general conv launch: none of the front's own kernels, no staging kernel."""
    return name.startswith("dffw::conv_") and not any(s in name for s in ("head_warp", "flow_volume", "ncdhw"))


def match_kernels(got, form, pi, C):
    volume = "dffw::flow_volume_kernel<%d>" % pi
    want = {"warp": [volume, "conv", "dffw::head_warp_kernel<%d, %d>" % (pi, C)], "split": [volume, "conv", "conv"], "whole": [volume, "conv"]}[form]
    assert len(got) == len(want), (form, got, want)
    for g, w in zip(got, want):
        assert is_conv(g) if w == "conv" else g == w, (form, got, want)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def call(eng, fed, p, ad, fd, prec):
    """One op call with y0 in a guarded buffer: y0 on the host, the launch list; the guards are checked."""
    B, C, N, H, W = fed.shape
    g = Guarded({"y0": 4 * B * 2 * C * N * H * W})
    y0 = g.view("y0", torch.float32, (B, 2 * C, N, H, W))
    eng.op_head_front(fed, *p, ad, fd, precision=prec, out=y0)
    ks = eng.op_kernels()
    torch.cuda.synchronize()
    g.check()
    SEEN[prec].update(ks)
    return y0.cpu(), ks


def paths(C, B, N, H, W, wgs):
    """(form, switches) of every way a shape is run."""
    base = dict(DFFW_ROLL_MIN_UNITS="1", **({"DFFW_SRD_WGS": str(wgs)} if wgs else {}))
    forced = dict(base, DFFW_NO_SMALL="1")
    first = "warp" if "warp" in hf.forms_of(C, B, N, H, W) else "split"
    return [(first, base), ("split", dict(forced, DFFW_NO_HEAD_WARP="1")), ("whole", dict(forced, DFFW_NO_HEAD_SPLIT="1"))]


def run_case(eng, i, j, prec, monkeypatch):
    C, (B, N, H, W), wgs = hf.SHAPES[i]
    pi = eng.PRECISIONS[prec]
    fe, p, alpha, fov, name = hf.case(i, j)
    r = hf.reference(fe, *p, alpha, fov, prec)
    fed, ad, fd = fe.cuda(), alpha.cuda(), fov.cuda()
    results = []
    for form, env in paths(C, B, N, H, W, wgs):
        _set(monkeypatch, env)
        y0, ks = call(eng, fed, p, ad, fd, prec)
        match_kernels(ks, form, pi, C)
        FORMS_SEEN[prec].add((form, C))
        assert torch.isfinite(y0).all(), (name, prec, form, ks)
        rt = hf.ratio(y0, r.ref, r.E)
        w = float(rt.max())
        print("%s %s %s: worst err / E %.3f" % (name, prec, form, w))
        assert w <= 1.0, (name, prec, form, ks, eb_report(rt))
        y0b, _ = call(eng, fed, p, ad, fd, prec)
        assert same_bits(y0, y0b), (name, prec, form, "a repeated call differs")
        WORST[(form, prec)] = max(WORST.get((form, prec), 0.0), w)
        results.append((form, y0))
    for a in range(len(results)):
        for b in range(a + 1, len(results)):
            d = (results[a][1].double() - results[b][1].double()).abs()
            assert bool((d <= 2.0 * r.E).all()), (name, prec, results[a][0], results[b][0], float((d / r.E.clamp_min(1e-300)).max()))


def eb_report(rt):
    flat = int(torch.argmax(rt.reshape(-1)))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), rt.shape))
    return "%d of %d elements over the bound; worst at %s (b, c, n, y, x)" % (int((rt > 1).sum()), rt.numel(), idx)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("i", range(len(hf.SHAPES)), ids=lambda i: "C%d_B%dN%d_%dx%d" % ((hf.SHAPES[i][0],) + hf.SHAPES[i][1]))
def test_front_forms(eng, i, prec, monkeypatch):
    """Every warp regime (identity, integer shifts, everything outside, fractional shifts, f = 1.4, f = 0.6, mixed signs; distinct per sample
    and slice) on a feature regime each (eb.REGIMES, smooth, one 1.0 per plane; cycling with the shape), in every form the shape can take.
    (32, 10, 8, 16) fills head_warp_kernel's table of 320 planes exactly; (33, 10, 8, 16) must report the split form's launches under the warp
    form's switches (match_kernels: launch_head_warp would refuse it)."""
    for j in range(len(hf.WARPS)):
        run_case(eng, i, j, prec, monkeypatch)


@pytest.mark.parametrize("i", range(len(hf.FOV_SHAPES)), ids=lambda i: "B%dC%dN%d_%dx%d%s" % (hf.FOV_SHAPES[i][0] + ("_compat" if hf.FOV_SHAPES[i][1] else "",)))
def test_fov_warp(eng, i):
    """fov_warp_kernel: flow within dflow, out within the position term plus the slice blend's Lz dsz (the kernel blends across slices where its
    float32 slice coordinate falls an ulp short, the reference does not), in guarded buffers, bit-identical on a second call.  N = 1, 2, 3,
    10, 15; planes one pixel high or wide; two samples; the batch quirk (compat_batch_alpha0).  The 64-bit-offset instantiation needs a volume
    of 4 GiB per (sample, channel) and is not run."""
    (B, C, N, H, W), compat = hf.FOV_SHAPES[i]
    for j in range(len(hf.WARPS)):
        x, alpha, fov, compat, name = hf.fov_case(i, j)
        r = hf.fov_reference(x, alpha, fov, compat)
        xd, ad, fd = x.cuda(), alpha.cuda(), fov.cuda()
        got = []
        for _ in range(2):
            g = Guarded({"out": 4 * x.numel(), "flow": 4 * B * 2 * N * H * W})
            out, flow = g.view("out", torch.float32, tuple(x.shape)), g.view("flow", torch.float32, (B, 2, N, H, W))
            eng.op_fov_warp(xd, ad, fd, compat_batch_alpha0=compat, out=out, flow=flow)
            torch.cuda.synchronize()
            g.check()
            got.append((out.cpu(), flow.cpu()))
        out, flow = got[0]
        assert torch.isfinite(out).all() and torch.isfinite(flow).all(), name
        ro, rf = hf.ratio(out, r.out, r.E_out), hf.ratio(flow, r.flow, r.E_flow)
        print("%s: worst err / E out %.3f flow %.3f" % (name, float(ro.max()), float(rf.max())))
        assert float(rf.max()) <= 1.0, (name, "flow", eb_report(rf))
        assert float(ro.max()) <= 1.0, (name, "out", eb_report(ro))
        assert same_bits(out, got[1][0]) and same_bits(flow, got[1][1]), (name, "a repeated call differs")
        WORST[("fov_warp out", "fp32")] = max(WORST.get(("fov_warp out", "fp32"), 0.0), float(ro.max()))
        WORST[("fov_warp flow", "fp32")] = max(WORST.get(("fov_warp flow", "fp32"), 0.0), float(rf.max()))


# ---- one tie to the forward: the op launches what the forward launches for these layers ---------------------------------------------
def test_op_launches_what_the_forward_launches(eng):
    """At the 64 x 96 End_to_End golden's three level sizes, B = 1, N = 10, default switches: the op's launch names are the forward's profile
    rows of that head's volume and .0.0 layers (names only: what the op tests is the dispatch the forward takes)."""
    import numpy as np
    from dffinthewild_amd import graph, synth
    from dffinthewild_amd.End_to_End import Network
    from oracle.make_goldens_e2e import net_inputs
    for k in SWITCHES:
        assert k not in os.environ, k
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e_net_smooth_64x96.npz"))
    entries = list(graph.param_entries(graph.e2e_convs()))
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(entries, seed=int(g["wseed"]), profile=str(g["profile"])).items()}
    H, W = int(g["H"]), int(g["W"])
    FS, fd, fov = (torch.from_numpy(t) for t in net_inputs(H, W, int(g["iseed"])))
    assert FS.shape[0] == 1 and FS.shape[2] == 10
    model = Network()
    model.load_state_dict(sd)
    model = model.cuda().eval()
    engine = model._engine_on(torch.device("cuda", torch.cuda.current_device()))
    engine.profile(True)
    try:
        with torch.no_grad():
            model(FS.cuda(), fd.cuda(), fov.cuda())
        prof = engine.profile_collect()
    finally:
        engine.profile(False)
    for C, lvl in ((8, 1), (16, 2), (32, 4)):
        head = hf.HEADS[C]
        hp = "optical_flow_aggregation." + head
        fwd = [k for k, layer, *_ in prof if layer == "flow.%s.volume" % head or layer.startswith(hp + ".0.0")]
        assert fwd, (hp, [layer for _, layer, *_ in prof])
        fe = hf.features("smooth", (1, C, 10, H // lvl, W // lvl), 7)
        bn0 = tuple(sd[hp + ".0.1" + s] for s in (".weight", ".bias", ".running_mean", ".running_var"))
        alpha, fv = hf.warp_params("fractional", 1, 10, H // lvl, W // lvl, 8)
        _, ks = call(eng, fe.cuda(), (sd[hp + ".0.0.weight"], bn0), alpha.cuda(), fv.cuda(), "bf16x3")
        assert ks == fwd, (hp, ks, fwd)


def _front_kernels_missing(prec, pi):
    want = ["dffw::head_warp_kernel<%d, 8>" % pi, "dffw::head_warp_kernel<%d, 16>" % pi, "dffw::flow_volume_kernel<%d>" % pi]
    missing = [k for k in want if k not in SEEN[prec]]
    # flow_volume_kernel's modes and the three packed filters, by the forms whose launch lists were asserted: warp = mode 2 + #ref, split = modes
    # 2 and 1 + #ref + #cur, whole = mode 0 + the whole filter
    return missing + ["the %s form at C = %d" % fc for fc in [(f, C) for C in (8, 16, 32) for f in hf.forms_of(C, 1, 1, 8, 16)] if fc not in FORMS_SEEN[prec]]


def test_zz_every_front_kernel_ran(eng, monkeypatch):
    """Over this module, per arithmetic: head_warp_kernel<P, 8> and <P, 16>, flow_volume_kernel<P> in its three modes (mode 2 alone in the warp
    form, 2 and 1 in the split form, 0 in the whole form: each form's launch list was asserted and its output, which a volume never written
    would leave NaN, was inside the bound) and the #ref / #cur / whole convs, at 8, 16 and 32 channels.  Run on its own, this test first runs
    one small case per channel count."""
    for prec in PRECS:
        pi = eng.PRECISIONS[prec]
        if _front_kernels_missing(prec, pi):
            for i in (1, 8, 14):
                run_case(eng, i, 3, prec, monkeypatch)
        assert not _front_kernels_missing(prec, pi), (prec, _front_kernels_missing(prec, pi), sorted(SEEN[prec]))
