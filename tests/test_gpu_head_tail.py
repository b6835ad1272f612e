"""GPU: the back half of the alignment network's alpha heads (head_tail() of csrc/dffw_align.cpp: convs .2, .4, .6 and the plane mean, to
alpha += damped mean and raw = mean), one call at a time through dffw_op_head_tail -- the forward's own dispatch on a private, NaN-poisoned
workspace -- and held number by number to the bound of tests/head_tail_ref.py against its float64 reference, in all three arithmetics.

Forms (head_tail_ref.FORMS) and how they are reached, the switches read per call:
  tiles   start = 0, C = 16, whole 8 x 16 columns, DFFW_ROLL_MIN_UNITS=1: of_roll_kernel<P, false, true> + head_tail_tiles_reduce / finish
  rows    start = 0, C = 32 / 64 at conv_sums_ok's floor of 256 tiles: conv .4 as a row-sums conv + head_tail_rows_reduce / finish
  planes  stored y2 (DFFW_NO_HEAD_SUMS_FUSED=1, DFFW_NO_FUSED_OF=1, small shapes, start = 2): plane_sums_kernel + head_tail_finish_kernel
  mean    stored y2, DFFW_NO_HEAD_SUMS=1: conv .6 into three fp32 planes + alpha_mean_kernel
Every call: alpha_in random and non-zero, alpha and raw inside one 0xFF-filled buffer with guards; the results finite, |got - ref| <= E on
each of the 2 * 3 * B * N numbers, the launch list the form's, a second call bit-identical, the guards intact.  Every pair of forms on one
input agrees within the sum of their bounds.  start = 2 feeds the reduction kernels planes the convs never hand them (H or W of 1, 2, 3,
planes under one chunk, a short last chunk, border lines under 256 / C phases) and inputs placed pixel by pixel; on an all-zero plane with
alpha_in = 0 the plane sums give bias6 and its damped value exactly.

Both finish kernels share the profile record of the kernel in front of them (one record for the two launches of launch_head_tail /
launch_head_tail_tiles / launch_head_tail_rows), so the launch list names plane_sums_kernel / the reduce kernels only; the numbers checked
are the finish kernels' output.  conv_slice32 / conv_slice64 exist in split-bf16 only (slice32_ok / slice64_ok refuse the 16-bit arithmetics)."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_tail_ref as ht  # noqa: E402
from test_gpu_train_records import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = ht.PRECISIONS
SWITCHES = ("DFFW_NO_FUSED_OF", "DFFW_NO_HEAD_SUMS", "DFFW_NO_HEAD_SUMS_FUSED", "DFFW_ROLL_MIN_UNITS", "DFFW_SRD_WGS", "DFFW_NO_TILE", "DFFW_NO_ROLL",
            "DFFW_NO_SLICE32")
WORST = {}    # (form, precision) -> max err / E seen in this module
SEEN = {p: set() for p in PRECS}   # precision -> every kernel name an op of this module launched
TILE_SUMS = re.compile(r"^dffw::conv_tile<(\d), 3, \d+, 5, 4, 16, \d+, \d+, \d+, true, false, \d+>$")   # the per-slice 1x3x3 geometry's row-sums variant
SLICE32_SUMS, SLICE64_SUMS = "dffw::conv_slice32<true, false, true>", "dffw::conv_slice64<true, true>"


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
        for (form, prec), v in WORST.items():
            key = "head_tail %s/%s" % (form, prec)
            old[key] = max(old.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def match_kernels(got, want):
    """``want`` with "conv" any single general conv launch (none of the head's own kernels) and "sums" any row-sums conv."""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        if w == "conv":
            assert not any(s in g for s in ("of_", "head_", "ncdhw", "plane_sums", "alpha_mean")) and g not in (SLICE32_SUMS, SLICE64_SUMS) and \
                not TILE_SUMS.match(g), (got, want)
        elif w == "sums":
            assert g in (SLICE32_SUMS, SLICE64_SUMS) or TILE_SUMS.match(g), (got, want)
        else:
            assert g == w, (got, want)


def call(eng, xd, p, alpha_in, prec, start):
    """One op call on guarded alpha / raw buffers: (raw, alpha_out) on the host, the launch list; the guards are checked."""
    B, _, N = xd.shape[:3]
    g = Guarded({"alpha": 4 * B * 3 * N, "raw": 4 * B * 3 * N})
    alpha, raw = g.view("alpha", torch.float32, (B, 3, N)), g.view("raw", torch.float32, (B, 3, N))
    alpha.copy_(alpha_in)
    eng.op_head_tail(xd, *p, alpha, raw, start=start, precision=prec)
    ks = eng.op_kernels()
    torch.cuda.synchronize()
    g.check()
    SEEN[prec].update(ks)
    return raw.cpu(), alpha.cpu(), ks


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def checked(eng, xd, p, alpha_in, r, prec, start, form, want, what):
    """The checks every case makes of one form; returns (raw, alpha_out)."""
    raw, alpha, ks = call(eng, xd, p, alpha_in, prec, start)
    match_kernels(ks, want)
    assert torch.isfinite(raw).all() and torch.isfinite(alpha).all(), (what, ks, raw, alpha)
    E_raw, E_alpha = r.E(form)
    rr, ra = ht.ratio(raw, r.raw, E_raw), ht.ratio(alpha, r.alpha, E_alpha)
    w = max(float(rr.max()), float(ra.max()))
    print("%s %s %s: worst err / E %.3f" % (what, prec, form, w))
    assert w <= 1.0, (what, prec, form, ks, "raw err / E", rr, "alpha err / E", ra)
    raw2, alpha2, _ = call(eng, xd, p, alpha_in, prec, start)
    assert same_bits(raw, raw2) and same_bits(alpha, alpha2), (what, "a repeated call differs")
    WORST[(form, prec)] = max(WORST.get((form, prec), 0.0), w)
    return raw, alpha


def agree(results, r, what):
    """Every pair of forms within the sum of their bounds, on every number."""
    forms = list(results)
    for i, fa in enumerate(forms):
        for fb in forms[i + 1:]:
            for k in (0, 1):
                d = (results[fa][k].double() - results[fb][k].double()).abs()
                assert bool((d <= r.E(fa)[k] + r.E(fb)[k]).all()), (what, fa, fb, "raw" if k == 0 else "alpha", d)


def pair_paths(pi):
    roll, rolls = "dffw::of_roll_kernel<%d, false>" % pi, "dffw::of_roll_kernel<%d, false, true>" % pi
    planes = "dffw::plane_sums_kernel<%d>" % pi
    return [("tiles", {}, [rolls, "dffw::head_tail_tiles_reduce_kernel"]),
            ("planes", {"DFFW_NO_HEAD_SUMS_FUSED": "1"}, [roll, planes]),
            ("mean", {"DFFW_NO_HEAD_SUMS": "1"}, [roll, "conv", "dffw::alpha_mean_kernel"]),
            ("planes", {"DFFW_NO_FUSED_OF": "1"}, ["conv", "conv", planes])]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ("random", "placed"))
@pytest.mark.parametrize("i", range(len(ht.PAIR_SHAPES)), ids=lambda i: "B%dN%d_%dx%d_w%d" % ht.PAIR_SHAPES[i])
def test_pair_forms(eng, i, kind, prec, monkeypatch):
    """C = 16 on whole 8 x 16 columns: the pair with sums, the stored pair with plane sums, the stored pair with conv .6 + alpha_mean, and no
    pair, on one input."""
    run_pair(eng, i, kind, prec, monkeypatch)


def run_pair(eng, i, kind, prec, monkeypatch):
    wgs = ht.PAIR_SHAPES[i][4]
    x, p, a = ht.pair_case(i, kind)
    r = ht.reference(x, *p, a, prec, 0, ht.FORMS)
    xd, results = x.cuda(), {}
    for n, (form, env, want) in enumerate(pair_paths(eng.PRECISIONS[prec])):
        _set(monkeypatch, dict(env, DFFW_ROLL_MIN_UNITS="1", **({"DFFW_SRD_WGS": str(wgs)} if wgs else {})))
        results["%s %d" % (form, n)] = checked(eng, xd, p, a, r, prec, 0, form, want, "pair %s %s" % (ht.PAIR_SHAPES[i], kind))
    agree({k: v for k, v in results.items()}, _ByPath(r), "pair %s %s" % (ht.PAIR_SHAPES[i], kind))


class _ByPath:
    """r.E by a results key "<form> <n>"."""

    def __init__(self, r):
        self.r = r

    def E(self, key):
        return self.r.E(key.split()[0])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ("random", "placed"))
@pytest.mark.parametrize("j", range(len(ht.ROWS_CASES)), ids=lambda j: "C%d_B%dN%d_%dx%d" % ((ht.ROWS_CASES[j][0],) + ht.ROWS_CASES[j][1]))
def test_rows_forms(eng, j, kind, prec, monkeypatch):
    """C = 32 / 64 at the smallest shapes where conv_sums_ok holds: conv .4 as a row-sums conv (the streaming conv_slice32 / conv_slice64 in
    split-bf16 on whole 8 x 16 columns, conv_tile's variant otherwise), and the two stored forms on the same input."""
    run_rows(eng, j, kind, prec, monkeypatch)


def run_rows(eng, j, kind, prec, monkeypatch):
    C, (B, N, H, W) = ht.ROWS_CASES[j]
    pi = eng.PRECISIONS[prec]
    x, p, a = ht.rows_case(j, kind)
    r = ht.reference(x, *p, a, prec, 0, ("rows", "planes", "mean"))
    xd, results, what = x.cuda(), {}, "rows %s %s" % (ht.ROWS_CASES[j], kind)
    planes = "dffw::plane_sums_kernel<%d>" % pi
    for form, env, want in (("rows", {}, ["conv", "sums", "dffw::head_tail_rows_reduce_kernel"]),
                            ("planes", {"DFFW_NO_HEAD_SUMS_FUSED": "1"}, ["conv", "conv", planes]),
                            ("mean", {"DFFW_NO_HEAD_SUMS": "1"}, ["conv", "conv", "conv", "dffw::alpha_mean_kernel"])):
        _set(monkeypatch, dict(env, DFFW_ROLL_MIN_UNITS="1"))
        results[form] = checked(eng, xd, p, a, r, prec, 0, form, want, what)
        if form == "rows":
            sums = eng.op_kernels()[1]
            if prec == "bf16x3" and H % 8 == 0:
                assert sums == (SLICE32_SUMS if C == 32 else SLICE64_SUMS), sums
            else:
                assert TILE_SUMS.match(sums) and int(TILE_SUMS.match(sums).group(1)) == pi, sums
    agree(results, r, what)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("j", range(len(ht.STORED_CASES)), ids=lambda j: "C%d_B%dN%d_%dx%d" % ((ht.STORED_CASES[j][0],) + ht.STORED_CASES[j][1]))
def test_small_shapes_take_the_stored_forms(eng, j, prec, monkeypatch):
    """Under conv_sums_ok's floor (32 / 64 channels) and off the 8 x 16 columns (16 channels) y2 is stored, whatever the switches allow."""
    x, p, a = ht.stored_case(j)
    r = ht.reference(x, *p, a, prec, 0, ("planes", "mean"))
    xd, results, what = x.cuda(), {}, "stored %s" % (ht.STORED_CASES[j],)
    for form, env, want in (("planes", {}, ["conv", "conv", "dffw::plane_sums_kernel<%d>" % eng.PRECISIONS[prec]]),
                            ("mean", {"DFFW_NO_HEAD_SUMS": "1"}, ["conv", "conv", "conv", "dffw::alpha_mean_kernel"])):
        _set(monkeypatch, dict(env, DFFW_ROLL_MIN_UNITS="1"))
        results[form] = checked(eng, xd, p, a, r, prec, 0, form, want, what)
    agree(results, r, what)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", (16, 32, 64))
@pytest.mark.parametrize("shape", ht.S2_SHAPES, ids=lambda s: "B%dN%d_%dx%d" % s)
def test_stored_forms_from_y2(eng, shape, C, prec, monkeypatch):
    """start = 2: the plane sums and conv .6 + alpha_mean on a given y2 -- random, one 1.0 per plane (every plane at another place: the
    corners, the border lines, the interior), all ones (every border correction as large as it gets), all zeros with alpha_in = 0 (exact)."""
    pi = eng.PRECISIONS[prec]
    for kind in ht.S2_KINDS:
        x, p, a = ht.s2_case(C, shape, kind)
        r = ht.reference(x, *p, a, prec, 2, ("planes", "mean"))
        xd, results, what = x.cuda(), {}, "y2 C%d %s %s" % (C, shape, kind)
        for form, env, want in (("planes", {}, ["dffw::plane_sums_kernel<%d>" % pi]), ("mean", {"DFFW_NO_HEAD_SUMS": "1"}, ["conv", "dffw::alpha_mean_kernel"])):
            _set(monkeypatch, env)
            results[form] = checked(eng, xd, p, a, r, prec, 2, form, want, what)
        agree(results, r, what)
        if kind == "zero":     # nothing to sum: the plane sums give bias6, and its damped value, exactly (the mean form sums HW copies of it in fp32)
            bias = p[5].float().reshape(1, 3, 1).expand(shape[0], 3, shape[1]).contiguous()
            step = bias.clone()
            step[:, 0] = torch.tensor(ht.DAMP32, dtype=torch.float32) * bias[:, 0]
            raw, alpha = results["planes"]
            assert same_bits(raw, bias) and same_bits(alpha, step), (what, raw, alpha)


# ---- one tie to the forward: the op launches what the forward launches for these layers ---------------------------------------------
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")


def test_op_launches_what_the_forward_launches(eng):
    """At the 64 x 96 End_to_End golden's three level sizes, B = 1, N = 10, default switches: the op's launch names are the forward's profile
    rows of that head's .2.0, .4.0, .6 and mean layers (names only: what the op tests is the dispatch the forward takes)."""
    from dffinthewild_amd import graph, synth
    from dffinthewild_amd.End_to_End import Network
    from oracle.make_goldens_e2e import net_inputs
    for k in SWITCHES:
        assert k not in os.environ, k
    g = np.load(os.path.join(GOLDEN_DIR, "e2e_net_smooth_64x96.npz"))
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
    bn = lambda k: tuple(sd[k + s] for s in (".weight", ".bias", ".running_mean", ".running_var"))
    for C, lvl in ((16, 1), (32, 2), (64, 4)):
        head = ht.HEADS[C]
        hp = "optical_flow_aggregation." + head
        fwd = [k for k, layer, *_ in prof if layer == "flow.%s.mean" % head or any(layer.startswith(hp + s) for s in (".2", ".4", ".6"))]
        assert fwd, (hp, [layer for _, layer, *_ in prof])
        x = ht.smooth_input(1, C, 10, H // lvl, W // lvl)
        p = (sd[hp + ".2.0.weight"], bn(hp + ".2.1"), sd[hp + ".4.0.weight"], bn(hp + ".4.1"), sd[hp + ".6.weight"], sd[hp + ".6.bias"])
        _, _, ks = call(eng, x.cuda(), p, ht.alpha_input(1, 10, 3), "bf16x3", 0)
        assert ks == fwd, (hp, ks, fwd)


def _tail_kernels_missing(prec, pi):
    seen = SEEN[prec]
    want = ["dffw::of_roll_kernel<%d, false, true>" % pi, "dffw::head_tail_tiles_reduce_kernel", "dffw::head_tail_rows_reduce_kernel",
            "dffw::plane_sums_kernel<%d>" % pi, "dffw::alpha_mean_kernel"] + ([SLICE32_SUMS, SLICE64_SUMS] if prec == "bf16x3" else [])
    missing = [k for k in want if k not in seen]
    if not any(TILE_SUMS.match(k) and int(TILE_SUMS.match(k).group(1)) == pi for k in seen):
        missing.append("a conv_tile row-sums instantiation of arithmetic %d" % pi)
    return missing


def test_zz_every_tail_kernel_ran(eng, monkeypatch):
    """Over this module, per arithmetic: the pair with sums, both reduce kernels, the plane sums, alpha_mean and conv_tile's row-sums variant; in
    split-bf16 also the two streaming row-sums convs, which the 16-bit arithmetics do not have (slice32_ok / slice64_ok: prec != P_BF16X3).
    The two finish kernels share their predecessor's record (module docstring).  Run on its own, this test first runs the cases that
    launch them: one pair shape and the first four row-sums cases."""
    for prec in PRECS:
        pi = eng.PRECISIONS[prec]
        if _tail_kernels_missing(prec, pi):
            run_pair(eng, 0, "random", prec, monkeypatch)
            for j in range(4):
                run_rows(eng, j, "random", prec, monkeypatch)
        assert not _tail_kernels_missing(prec, pi), (prec, _tail_kernels_missing(prec, pi), sorted(SEEN[prec]))
