"""CPU: the reference, the bound and the emulation of tests/regress_ref.py hold together before any GPU is asked -- the float32 tap rule is
PyTorch's, the clean float32 emulation sits at a quarter of the bound, and every planted fault is far outside it wherever it can act at all.

What the bound cannot see (regress_ref's docstring): one slice's p off by 2^-18 relative stays under it (test_bound_blind_spot shows it)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regress_ref as R  # noqa: E402


def _worst(cid, got):
    """worst err / E over the heads of a case, with the full bound"""
    return max(float(R.ratio(g, r["d"], E).max()) for g, (r, E) in zip(got, R.case_reference(cid)))


SIZES = [(4, 6, 32, 48), (5, 7, 12, 20), (3, 3, 12, 20), (16, 16, 8, 8), (16, 6, 16, 24), (1, 5, 12, 20), (6, 1, 12, 20), (12, 20, 12, 20), (7, 9, 5, 4),
         (37, 53, 111, 97), (130, 130, 1040, 1040)]


@pytest.mark.parametrize("h,w,H,W", SIZES[:-1] + [(13, 13, 104, 104)])
def test_manual_taps_are_pytorchs(h, w, H, W):
    """The float32 manual-tap upsampling of regress_ref equals F.interpolate(mode="bilinear", align_corners=False) in float32 to 1 ulp of the largest
    tap value, sizes that do not divide and downsampling included.  The input is one plane per source row (ones along the row) and one per source
    column, largest tap value 1: every output element is then a tap weight, or the sum of the two of an axis, so the gate of 2^-23 is on the indices
    and the weights themselves (an index off by one is an error of up to 1, the product rounded before the subtraction ~1e-6 at 37 -> 111)."""
    rows = torch.eye(h).view(1, h, h, 1).expand(1, h, h, w)
    cols = torch.eye(w).view(1, w, 1, w).expand(1, w, h, w)
    s = torch.cat([rows, cols], 1).contiguous()
    v, V = R._interp(s, H, W, torch.float32)
    want = F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False)
    assert float((v - want).abs().max()) <= 2.0 ** -23, float((v - want).abs().max())
    assert torch.equal(v, V)


@pytest.mark.parametrize("h,w,H,W", SIZES)
def test_manual_upsampling_of_random_scores(h, w, H, W):
    """... and on scores in +-30 the two stay within 4 ulp of the largest tap value: each side is a float32 evaluation of the same taps with three
    roundings on the path of every term (PyTorch associates and contracts them its own way; against the exactly evaluated taps its result
    measured up to 1.9 ulp, this file's up to 2.0), so 2 + 2."""
    s = (torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h * 100 + w)) * 2 - 1) * 30
    v, V = R._interp(s, H, W, torch.float32)
    want = F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False)
    ulp = 2.0 ** (torch.floor(torch.log2(s.abs().max())) - 23)
    assert float((v - want).abs().max()) <= 4 * float(ulp), (float((v - want).abs().max()), float(ulp))
    assert bool((V >= v.abs() * (1 - 1e-6)).all())


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_emulation_in_float64_is_the_reference(cid):
    c = R.make_case(cid)
    got = R.emulate(c["scores"], c["fd"], c["H"], c["W"], dtype=torch.float64)
    for g, (r, _) in zip(got, R.case_reference(cid)):
        assert float((g - r["d"]).abs().max()) <= 1e-12 * max(1.0, float(r["f"].abs().max()))


def test_calibration():
    """ALPHA's measurement: the float32 emulation's worst err / E at ALPHA = 1 and EPS_SP = 0 over all cases is CAL (printed per case), and
    ALPHA is four times that, rounded up to a power of two.  With it the clean emulation is at or below E / 4 on every case."""
    worst = {}
    for cid in R.CASE_IDS:
        c = R.make_case(cid)
        got = R.emulate(c["scores"], c["fd"], c["H"], c["W"])
        per = []
        for g, (r, _) in zip(got, R.case_reference(cid)):
            per.append(float(R.ratio(g, r["d"], R.bound(r, alpha=1.0, eps_sp=0.0)).max()))
            assert float(R.ratio(g, r["d"], R.bound(r, eps_sp=0.0)).max()) <= 0.25, cid
        worst[cid] = per
        print("%-20s err/E at alpha=1: %s" % (cid, " ".join("%.3f" % x for x in per)))
    cal = max(max(p) for p in worst.values())
    print("CAL measured %.3f, recorded %.2f; ALPHA %g" % (cal, R.CAL, R.ALPHA))
    assert cal <= R.CAL <= 1.1 * cal + 0.05, (cal, R.CAL)
    alpha = 1.0
    while alpha < 4 * R.CAL:
        alpha *= 2
    assert R.ALPHA == alpha


# where a fault cannot touch a case (regress_ref.can_act):
#   every fault but drop_last   N = 1 (f10_n1_net4): d = f p / p whatever v and p are; without its one term the sum is 0 / 0
#   no_clamp        f16_n16_down: downsampling from 16 to 8 never has its first tap on the last row / column (the last source coordinate is 14.5),
#                   and a head at output resolution has weight 0 on the second tap (a CPU trial of such a head alone gave err / E = 0.7)
#   fd_pixel0       the (B,N,1,1) layouts: every pixel's focus distances are pixel (0, 0)'s
#   single_load_h   the cases without a head that has h == H and w != W (all but the two *_hmatch cases)
@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_exceed_the_bound(fault):
    acted = 0
    for cid in R.CASE_IDS:
        c = R.make_case(cid)
        if not R.can_act(fault, c):
            continue
        acted += 1
        w = _worst(cid, R.emulate(c["scores"], c["fd"], c["H"], c["W"], fault=fault))
        print("%-16s %-20s err/E %.3g" % (fault, cid, w))
        assert w > 4.0, (fault, cid, w)
    assert acted >= 2, fault


def test_faults_that_cannot_act_change_nothing():
    """can_act is not an excuse list: where it says a fault cannot touch a case, the faulty emulation IS the clean one, bit for bit (N = 1: within a
    quarter of the bound, as the clean one is)."""
    for cid in R.CASE_IDS:
        c = R.make_case(cid)
        clean = None
        for fault in R.FAULTS:
            if R.can_act(fault, c):
                continue
            clean = clean or R.emulate(c["scores"], c["fd"], c["H"], c["W"])
            got = R.emulate(c["scores"], c["fd"], c["H"], c["W"], fault=fault)
            if c["N"] > 1:
                assert all(torch.equal(a, b) for a, b in zip(got, clean)), (fault, cid)
            else:       # f p / p rounds differently with another p: still far inside the bound
                assert _worst(cid, got) <= 0.25, (fault, cid)


def test_bound_blind_spot():
    """One slice's p off by 2^-18 relative stays under the bound (it is 4 ulp of p; ALPHA u (1 + V) + EPS_SP is larger at every V): written down
    so that nobody takes the bound for an ulp-exact check of softplus."""
    c = R.make_case("f10_n10_net4")
    H, W = c["H"], c["W"]
    for score, (r, E) in zip(c["scores"], R.case_reference("f10_n10_net4")):
        v, _ = R._interp(score, H, W, torch.float64)
        p = F.softplus(v) + 1e-6
        p[:, 0] *= 1 + 2.0 ** -18
        d = (r["f"] * p).sum(1) / p.sum(1)
        assert float(R.ratio(d, r["d"], E).max()) < 1.0


def test_case_inputs_hold_what_they_promise():
    for cid in R.CASE_IDS:
        c = R.make_case(cid)
        B, N, H, W = c["B"], c["N"], c["H"], c["W"]
        assert c["fd"].expand(B, N, H, W).shape == (B, N, H, W)
        planted = 0
        for k, s in enumerate(c["scores"]):
            if k == c["flat"]:
                assert float(s.abs().max()) <= 1e-3
                continue
            v, _ = R._interp(s, H, W, torch.float64)
            px = v[0, :, 0, 0]
            assert bool((px <= -40).all()) and px.unique().numel() == N
            assert float(s.max()) == 45.0
            planted += 1
        assert planted >= 1
    assert any(bool((R.make_case(cid)["fd"] < 0).any()) and bool((R.make_case(cid)["fd"] > 0).any()) for cid in R.CASE_IDS)
    assert R.make_case("stride_n2")["H"] * R.make_case("stride_n2")["W"] > 4096 * 256


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def test_refusals_without_gpu(eng):
    """Both regression entry points refuse a null pointer, n_heads outside 1..4 and any size below 1 with DFFW_EINVAL and a message, before any
    GPU call (this test runs where there is no GPU: a call that got as far as hipSetDevice would return DFFW_EHIP).  With N = 0 the kernels would
    clamp the slice index to -1 and read in front of the score volume."""
    lib = eng.lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    st = (ctypes.c_int64 * 4)(0, 1, 0, 0)
    ok = dict(B=1, N=2, h=2, w=2, H=4, W=4)

    def one(score=p, fd=p, strides=st, depth=p, **kw):
        a = dict(ok, **kw)
        return lib.dffw_op_regress(0, score, a["B"], a["N"], a["h"], a["w"], a["H"], a["W"], fd, strides, depth, None)

    def many(n=2, scores=(p, p, p, p), depths=(p, p, p, p), hs=(2, 2, 2, 2), ws=(2, 2, 2, 2), fd=p, strides=st, arrays=True, **kw):
        a = dict(ok, **kw)
        sc = (ctypes.c_void_p * 4)(*scores) if arrays else None
        return lib.dffw_op_regress_heads(0, n, sc, (ctypes.c_int * 4)(*hs), (ctypes.c_int * 4)(*ws), (ctypes.c_void_p * 4)(*depths),
                                         a["B"], a["N"], a["H"], a["W"], fd, strides, 1, None)

    def refused(rc, word):
        msg = lib.dffw_last_error()
        assert rc == -1 and word in msg, (rc, msg)

    for kw in (dict(score=None), dict(fd=None), dict(strides=None), dict(depth=None)):
        refused(one(**kw), b"null")
    for key in ("B", "N", "h", "w", "H", "W"):
        for bad in (0, -3):
            refused(one(**{key: bad}), b"bad shape")
    for n in (0, 5, -1):
        refused(many(n=n), b"n_heads")
    refused(many(arrays=False), b"null")
    refused(many(fd=None), b"null")
    refused(many(strides=None), b"null")
    refused(many(scores=(p, None, p, p)), b"null")
    refused(many(depths=(p, None, p, p)), b"null")
    for key in ("B", "N", "H", "W"):
        refused(many(**{key: 0}), b"bad shape")
    refused(many(hs=(2, 0, 2, 2)), b"bad shape")
    refused(many(ws=(2, 2, -1, 2), n=3), b"bad shape")
    assert eng.op_kernels() == []
