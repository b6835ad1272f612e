"""GPU: the fused front-end block kernels (the SRD blocks behind V1, V2, V3 and the two EFD blocks between them), called one block at
a time through dffw_op_srd / dffw_op_efd -- the forward's own srd() / efd() dispatch on a private, NaN-poisoned workspace -- and held
element by element to the composed forward-error bound of oracle/error_bounds.py (srd_ref64 / efd_ref64) against a float64 reference.
Every path of each block is checked, the kernels that ran are asserted from the op's launch list, two paths of one block agree to twice
the bound, a repeated call is bit-identical, and the forward's own taps tie the op to the forward's dispatch at the golden sizes."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dffinthewild_amd import graph, synth
from oracle import error_bounds as eb

pytestmark = pytest.mark.gpu

PRECS = ("bf16x3", "fp16", "bf16")
WORST = {}   # (kernel family, precision) -> max err / bound seen in this module


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
    """The block's distinguishing kernel: the last launch that is not a plain pool, without its template arguments."""
    main = [k for k in kernels if not k.startswith("dffw::pool_kernel")][-1]
    return main.split("<")[0].replace("dffw::", "")


def bounded(got, r, prec, kernels, what):
    """Finite everywhere (the workspace is NaN), within the bound on every element, exactly 0 where D == 0 (also in fp16, whose bound
    has an absolute subnormal term there); logs the worst ratio under the block's kernel family."""
    got = got.cpu()
    assert torch.isfinite(got).all(), (what, kernels)
    worst = eb.check_elementwise(got, r, prec, "%s %s" % (what, kernels))
    zero = r.D == 0
    assert torch.equal(got[zero], torch.zeros_like(got[zero])), (what, "non-zero outside the footprint")
    k = (family(kernels), prec)
    WORST[k] = max(WORST.get(k, 0.0), worst)
    return worst


def regime_of(i):
    return eb.REGIMES[i % len(eb.REGIMES)]


def _set(monkeypatch, env):
    for k in ("DFFW_NO_FUSED_SRD", "DFFW_NO_FUSED_ATTENTION", "DFFW_NO_FUSED_POOL", "DFFW_SRD_PIPE", "DFFW_NO_FUSED_EFD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- SRD, 8 and 16 channels --------------------------------------------------------------------------------------------------
# (B, N, H, W, wgs): realistic V1 / V2 tiles (8 x 16 and 4 x 16 columns), slice counts 1, 2, 3, 10, 15, non-square maps, batch up to
# 4, one column per workgroup and long column streams, column counts that are not a multiple of 8 (2 x 4 x 3 = 24 / 2 x 8 x 3 = 48
# columns of 8 x 16; 3 x 4 x 5 = 60 of 4 x 16), fewer columns than XCDs (3 x 2 = 6 of 8 x 16 / of 4 x 16: two XCDs' workgroups have nothing to do)
SRD_SHAPES = [(1, 10, 64, 128, 0), (2, 1, 32, 48, 8), (4, 3, 16, 32, 16), (1, 2, 32, 64, 0), (2, 15, 16, 32, 8), (3, 3, 16, 80, 16), (3, 2, 16, 16, 0)]


def srd_paths(C):
    """(name, env, the kernels that must run with the pooled copy requested)."""
    p = "{p}"
    paths = [
        ("fused+pool", {}, ["dffw::srd_roll%s_kernel<%s, true>" % ("16" if C == 16 else "", p)]),
        ("fused", {"DFFW_NO_FUSED_POOL": "1"}, ["dffw::srd_roll%s_kernel<%s, false>" % ("16" if C == 16 else "", p), "dffw::pool_kernel<%s>" % p]),
        ("three-launch", {"DFFW_NO_FUSED_SRD": "1"}, ["conv", "conv", "dffw::srd_attention_kernel<%s, %d>" % (p, C)]),
        ("gather-gemm", {"DFFW_NO_FUSED_ATTENTION": "1"}, ["conv", "conv", "conv", "conv", "dffw::pool_kernel<%s>" % p]),
    ]
    if C == 16:
        paths.insert(1, ("pipe", {"DFFW_SRD_PIPE": "1"}, ["dffw::srd_pipe16_kernel<%s, true, 0>" % p]))
    return paths


def match_kernels(got, want, pi):
    """``want`` with "{p}" the precision index ``pi`` and "conv" any single conv launch (not one of the block's fused kernels)."""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        if w == "conv":
            assert not any(s in g for s in ("srd_", "efd", "pool_kernel")), (got, want)
        else:
            assert g == w.replace("{p}", str(pi)), (got, want)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("shape", SRD_SHAPES, ids=lambda s: "B%dN%d_%dx%d_w%d" % s)
def test_srd_block_every_path(eng, shape, C, prec, monkeypatch):
    B, N, H, W, wgs = shape
    if C == 16:   # the stage-2 maps: half the V1 rows
        H //= 2
    regime = regime_of(SRD_SHAPES.index(shape) + C)
    x = eb.regime_input(regime, (B, C, N, H, W), seed=B * N + C)
    wts = eb.srd_params(regime, C, seed=100 + C + N)
    r, rp = eb.srd_ref64(x, *wts, prec)
    xd = x.cuda()
    monkeypatch.setenv("DFFW_ROLL_MIN_UNITS", "1")
    if wgs:
        monkeypatch.setenv("DFFW_SRD_WGS", str(wgs))
    first = None
    for name, env, want in srd_paths(C):
        _set(monkeypatch, env)
        y, pooled = eng.op_srd(xd, *wts, pooled=True, precision=prec)
        ks = eng.op_kernels()
        match_kernels(ks, want, eng.PRECISIONS[prec])
        bounded(y, r, prec, ks, "SRD %d %s y" % (C, name))
        bounded(pooled, rp, prec, ks, "SRD %d %s pooled" % (C, name))
        # y is the stored value (hi + lo is exact in fp32) and the split is monotone: the pooled copy is max_pool(y) bit for bit on every path
        assert torch.equal(pooled, F.max_pool3d(y, (1, 2, 2))), "SRD %d %s: pooled copy is not max_pool(y)" % (C, name)
        if first is None:
            first = (y.cpu(), pooled.cpu())
            y2, p2 = eng.op_srd(xd, *wts, pooled=True, precision=prec)
            assert torch.equal(y2, y) and torch.equal(p2, pooled), "repeated call differs"
            assert torch.equal(p2, F.max_pool3d(y2, (1, 2, 2)))
        else:
            eb.check_pair(y.cpu(), first[0], r, prec, "SRD %d %s vs fused" % (C, name))
            eb.check_pair(pooled.cpu(), first[1], rp, prec, "SRD %d %s pooled vs fused" % (C, name))


@pytest.mark.parametrize("C,B,N,H,W", [(8, 1, 10, 256, 256), (16, 2, 10, 128, 128)])
def test_srd_block_at_the_forward_threshold(eng, C, B, N, H, W, monkeypatch):
    """At the benchmark's V1 / V2 sizes the fused kernel takes the block under the default column threshold."""
    _set(monkeypatch, {})
    monkeypatch.delenv("DFFW_ROLL_MIN_UNITS", raising=False)
    x = eb.regime_input("post_relu", (B, C, N, H, W), seed=5)
    wts = eb.srd_params("trained_bn", C, seed=6)
    r, rp = eb.srd_ref64(x, *wts, "bf16x3")
    y, pooled = eng.op_srd(x.cuda(), *wts, pooled=True)
    ks = eng.op_kernels()
    assert ks == ["dffw::srd_roll%s_kernel<0, true>" % ("16" if C == 16 else "")], ks
    bounded(y, r, "bf16x3", ks, "SRD %d y" % C)
    bounded(pooled, rp, "bf16x3", ks, "SRD %d pooled" % C)
    assert torch.equal(pooled, F.max_pool3d(y, (1, 2, 2))), "SRD %d: pooled copy is not max_pool(y)" % C


# ---- SRD, 32 channels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,N,H,W", [(1, 10, 32, 64), (2, 1, 16, 32), (4, 3, 8, 48), (1, 2, 16, 16), (2, 15, 8, 32), (1, 3, 16, 40), (2, 2, 8, 24)])
def test_srd32_block_every_path(eng, B, N, H, W, prec, monkeypatch):
    """srd_attention_mfma where W % 16 == 0, else (W = 40, 24) the gather-GEMM convs; DFFW_NO_FUSED_ATTENTION forces the latter."""
    _set(monkeypatch, {})
    regime = regime_of(B + N + W)
    x = eb.regime_input(regime, (B, 32, N, H, W), seed=B + N)
    wts = eb.srd_params(regime, 32, seed=200 + N)
    r, _ = eb.srd_ref64(x, *wts, prec)
    xd = x.cuda()
    y = eng.op_srd(xd, *wts, precision=prec)
    ks = eng.op_kernels()
    if W % 16 == 0:
        assert len(ks) == 3 and ks[2] == "dffw::srd_attention_mfma<%d>" % eng.PRECISIONS[prec], ks
    else:
        assert len(ks) == 4 and not any("srd_" in k for k in ks), ks
    bounded(y, r, prec, ks, "SRD 32 y")
    assert torch.equal(eng.op_srd(xd, *wts, precision=prec), y), "repeated call differs"
    yp, pooled = eng.op_srd(xd, *wts, pooled=True, precision=prec)
    assert torch.equal(pooled, F.max_pool3d(yp, (1, 2, 2))), ("SRD 32: pooled copy is not max_pool(y)", eng.op_kernels())
    if W % 16 == 0:
        monkeypatch.setenv("DFFW_NO_FUSED_ATTENTION", "1")
        y2 = eng.op_srd(xd, *wts, precision=prec)
        ks2 = eng.op_kernels()
        assert len(ks2) == 4 and not any("srd_" in k for k in ks2), ks2
        bounded(y2, r, prec, ks2, "SRD 32 gather-GEMM y")
        eb.check_pair(y2.cpu(), y.cpu(), r, prec, "SRD 32 gather-GEMM vs mfma")


# ---- EFD 8 -> 16 and 16 -> 32 ---------------------------------------------------------------------------------------------------
# (B, N, H, W, wgs) of the block's input: outputs tiled 4 x 16 (conv_roll_efd) or 8 x 8 (conv_efd16); 2 x 2 x 3 = 12 / 2 x 1 x 6 = 12
# columns; long streams with few workgroups
def fused_efd(kernel):
    """Both branches of the block in one launch (conv_roll_efd's dual form, or conv_efd16); conv_roll_efd's single form is a conv."""
    return kernel == "dffw::conv_efd16" or re.match(r"dffw::conv_roll_efd<\d, \d+, true,", kernel) is not None


EFD_SHAPES = [(1, 10, 64, 128, 0), (2, 1, 16, 96, 8), (4, 3, 16, 32, 16), (1, 2, 32, 64, 0), (2, 15, 16, 32, 8)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cin", [8, 16])
@pytest.mark.parametrize("shape", EFD_SHAPES, ids=lambda s: "B%dN%d_%dx%d_w%d" % s)
def test_efd_block_every_path(eng, shape, cin, prec, monkeypatch):
    B, N, H, W, wgs = shape
    _set(monkeypatch, {})
    regime = regime_of(EFD_SHAPES.index(shape) + cin)
    x = eb.regime_input(regime, (B, cin, N, H, W), seed=B * N + cin)
    wts = eb.efd_params(regime, cin, seed=300 + cin + N)
    r = eb.efd_ref64(x, *wts)
    xd = x.cuda()
    pi = eng.PRECISIONS[prec]
    monkeypatch.setenv("DFFW_ROLL_MIN_UNITS", "1")
    if wgs:
        monkeypatch.setenv("DFFW_ROLL_WGS", str(wgs))
    y = eng.op_efd(xd, *wts, pooled_at_hand=True, precision=prec)
    ks = eng.op_kernels()
    assert ks[0] == "dffw::pool_kernel<%d>" % pi, ks
    fused = cin == 8 or prec == "bf16x3"          # conv_efd16 exists in split-bf16 only: fp16 / bf16 fall back to two convs
    if cin == 8:
        assert len(ks) == 2 and ks[1].startswith("dffw::conv_roll_efd<%d, 5, true," % pi), ks
    elif fused:
        assert ks[1:] == ["dffw::conv_efd16"], ks
    else:
        assert len(ks) == 3 and not any(fused_efd(k) for k in ks), ks
    bounded(y, r, prec, ks, "EFD %d" % cin)
    assert torch.equal(eng.op_efd(xd, *wts, pooled_at_hand=True, precision=prec), y), "repeated call differs"
    for name, hand, env in (("two-launch, pooled at hand", True, {"DFFW_NO_FUSED_EFD": "1"}), ("two-launch, pools for itself", False, {})):
        _set(monkeypatch, env)
        y2 = eng.op_efd(xd, *wts, pooled_at_hand=hand, precision=prec)
        ks2 = eng.op_kernels()
        assert len(ks2) == 3 and not any(fused_efd(k) for k in ks2), (name, ks2)
        assert ks2[0 if hand else 1] == "dffw::pool_kernel<%d>" % pi, (name, ks2)
        bounded(y2, r, prec, ks2, "EFD %d %s" % (cin, name))
        if fused:
            eb.check_pair(y2.cpu(), y.cpu(), r, prec, "EFD %d %s vs fused" % (cin, name))


# ---- the forward's own dispatch: tapped block inputs through the op ---------------------------------------------------------------
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
SRD_PREFIX = {8: "DFF_net.FM_measure.Focus_extraction.2", 16: "DFF_net.FM_conv1.1", 32: "DFF_net.FM_conv2.1"}
EFD_PREFIX = {8: "DFF_net.FM_conv1.0", 16: "DFF_net.FM_conv2.0"}


def _golden_case(which):
    g = np.load(os.path.join(GOLDEN_DIR, "den_%s.npz" % which))
    meta = {k: g[k].item() for k in ("B", "N", "H", "W", "layout", "profile", "wseed", "iseed")}
    FS = torch.from_numpy(synth.focal_stack(meta["B"], meta["N"], meta["H"], meta["W"], seed=meta["iseed"]))
    fd = synth.focus_dists(meta["B"], meta["N"], meta["H"], meta["W"]) if meta["layout"] == "dense" \
        else synth.focus_dists(meta["B"], meta["N"], 1, 1)
    entries = list(graph.param_entries(graph.dff_net_convs()))
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(entries, meta["wseed"], meta["profile"]).items()}
    return FS, torch.from_numpy(np.ascontiguousarray(fd)), sd


def _layer_kernels(prof, prefix):
    return [k for k, layer, *_ in prof if layer == prefix or layer.startswith(prefix + ".")]


@pytest.mark.parametrize("which,min_units", [("tiny_taps", "1"), ("batch2_bcast", "1"), ("he_n10_64", "1"), ("tiny_taps", None)])
def test_blocks_match_the_forward_taps(eng, which, min_units, monkeypatch):
    """The three configurations of test_streaming_kernels_at_golden_sizes (every streaming kernel forced on) and the fallback-sized
    tiny case: each block's tapped input and the checkpoint's weights through the op give the forward's tapped output within twice
    the bound, launching the kernels the forward's profile shows for that layer."""
    from dffinthewild_amd.Depth_Estimation_Network import Network
    _set(monkeypatch, {})
    if min_units:
        monkeypatch.setenv("DFFW_ROLL_MIN_UNITS", min_units)
    FS, fd, sd = _golden_case(which)
    model = Network()
    model.load_state_dict(sd)
    model = model.cuda().eval()
    engine = model._engine_on(torch.device("cuda", torch.cuda.current_device()))
    names = ["stem", "V1", "E1", "V2", "E2", "V3"]
    engine.profile(True)
    try:
        with torch.no_grad():
            _, taps = model.forward_with_taps(FS.cuda(), fd.cuda(), names)
        prof = engine.profile_collect()
    finally:
        engine.profile(False)
    w = lambda k: sd[k]
    bn = lambda k: tuple(sd[k + s] for s in (".weight", ".bias", ".running_mean", ".running_var"))
    for C, src, dst in ((8, "stem", "V1"), (16, "E1", "V2"), (32, "E2", "V3")):
        p = SRD_PREFIX[C]
        wts = (w(p + ".Focus_Measure.conv.0.0.weight"), bn(p + ".Focus_Measure.conv.0.1"), w(p + ".Focus_Measure.conv.2.0.weight"),
               bn(p + ".Focus_Measure.conv.2.1"), w(p + ".N_ch_attention.0.weight"), w(p + ".N_ch_attention.2.weight"))
        r, _ = eb.srd_ref64(taps[src].cpu(), *wts, "bf16x3")
        y = eng.op_srd(taps[src], *wts, pooled=C < 32)
        if C < 32:
            assert torch.equal(y[1], F.max_pool3d(y[0], (1, 2, 2))), "SRD %d at %s: pooled copy is not max_pool(y)" % (C, which)
        y = y[0] if C < 32 else y
        ks = eng.op_kernels()
        fwd = _layer_kernels(prof, p)
        assert ks[:len(fwd)] == fwd and all(k.startswith("dffw::pool_kernel") for k in ks[len(fwd):]), (p, ks, fwd)
        bounded(y, r, "bf16x3", ks, "SRD %d at %s" % (C, which))
        eb.check_pair(y.cpu(), taps[dst].cpu(), r, "bf16x3", "SRD %d op vs forward tap (%s)" % (C, which))
    for C, src, dst in ((8, "V1", "E1"), (16, "V2", "E2")):
        p = EFD_PREFIX[C]
        wts = (w(p + ".stride_conv.0.weight"), bn(p + ".stride_conv.1"), w(p + ".max_pooling.1.0.weight"), bn(p + ".max_pooling.1.1"))
        r = eb.efd_ref64(taps[src].cpu(), *wts)
        y = eng.op_efd(taps[src], *wts, pooled_at_hand=True)
        ks = eng.op_kernels()
        fwd = _layer_kernels(prof, p)
        assert ks[0].startswith("dffw::pool_kernel") and ks[1:] == fwd, (p, ks, fwd)   # (the forward's SRD block wrote the pooled copy)
        bounded(y, r, "bf16x3", ks, "EFD %d at %s" % (C, which))
        eb.check_pair(y.cpu(), taps[dst].cpu(), r, "bf16x3", "EFD %d op vs forward tap (%s)" % (C, which))
