"""GPU: the regression heads' three kernel forms -- dffw::regress_fused_kernel<10>, <16> and dffw::regress_kernel with one workgroup row per
head -- called directly through dffw_op_regress_heads, at the shapes where they can go wrong (tests/regress_ref.py CASES: every N at which the
five-slice blocks end differently, the 10 | 11 and 16 | 17 dispatch edges, a head with h == H but w != W, sizes that do not divide,
downsampling, h = 1 / w = 1, four focus-distance layouts, the second trip of the grid-stride loop), every element against the float64
reference within the bound E of regress_ref.

Every depth map is a slice of one 0xFF-filled buffer with 0xFF guards on both sides (as in test_gpu_train_records.py): an element no thread
stores is NaN, a store outside the map breaks a guard.  For every case the fused launch, the launch with fused=False and one dffw_op_regress
call per head must agree bit for bit (DESIGN.md §4.7 and §12 claim it, the training loss depends on it), and two runs must give the same bits.

No test here calls a kernel with a size below 1 or a wrong size: the refusals are asked of the validated entry points only."""
import ctypes
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regress_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, ALIGN = 4096, 256
WORST = {}       # kernel -> worst err / E over the cases


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


@pytest.fixture(scope="module", autouse=True)
def worst_ratio_report():
    """Prints the worst err / E per kernel; with ERROR_BOUND_REPORT=<file> it is merged into that JSON file, as test_gpu_ops.py does."""
    yield
    for k, v in sorted(WORST.items()):
        print("worst err/E %-34s %.4f" % (k, v))
    path = os.environ.get("ERROR_BOUND_REPORT")
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for k, v in WORST.items():
            key = "%s/fp32" % k.replace("dffw::", "")
            old[key] = max(old.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


class GuardedMaps:
    """n float32 (B,H,W) maps as slices of one 0xFF-filled uint8 device tensor: each at an ALIGN-ed offset, GUARD bytes of 0xFF before and after it."""

    def __init__(self, n, B, H, W):
        self.shape, self.nbytes, self.offs, off = (B, H, W), 4 * B * H * W, [], GUARD
        for _ in range(n):
            self.offs.append(off)
            off = -(-(off + self.nbytes + GUARD) // ALIGN) * ALIGN
        self.buf = torch.full((off,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % ALIGN == 0

    def maps(self):
        return [self.buf[o:o + self.nbytes].view(torch.float32).reshape(self.shape) for o in self.offs]

    def check(self):
        """Every byte outside the maps is still 0xFF (call after the stream has drained)."""
        outside = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for o in self.offs:
            outside[o:o + self.nbytes] = False
        bad = int((self.buf[outside] != 0xFF).sum())
        assert bad == 0, "%d guard bytes written" % bad


def device_inputs(c):
    """The case's scores and focus distances on the GPU, the focus distances in the layout the case names (strides are part of what is tested)."""
    B, N, H, W = c["B"], c["N"], c["H"], c["W"]
    fd = c["fd"]
    if c["layout"] == "perm":
        dev = fd.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
        assert dev.stride(3) == N and (N == 1 or dev.stride(1) == 1)
    else:
        dev = fd.contiguous().cuda()
    st = dev.expand(B, N, H, W).stride()
    if c["layout"] == "1n11":
        assert st == (0, 1, 0, 0)
    if c["layout"] == "bn11":
        assert st == (N, 1, 0, 0)
    if c["layout"] in ("dense", "signed"):
        assert st == (N * H * W, H * W, W, 1)
    assert torch.equal(dev.cpu(), fd)
    return [s.cuda() for s in c["scores"]], dev


def run_heads(eng, scores, fd, c, fused):
    """One dffw_op_regress_heads launch into guarded, 0xFF-filled maps: (CPU copies of the maps, the kernel names it reported)."""
    G = GuardedMaps(len(scores), c["B"], c["H"], c["W"])
    out = eng.op_regress_heads(scores, fd, c["H"], c["W"], fused=fused, out=G.maps())
    names = eng.op_kernels()
    torch.cuda.synchronize()
    G.check()
    return [o.cpu() for o in out], names


def same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        diff = x.view(torch.int32) != y.view(torch.int32)
        assert not bool(diff.any()), "%s: head %d differs in %d of %d elements, by up to %.3g" % (
            what, k, int(diff.sum()), diff.numel(), float((x.double() - y.double()).abs().max()))


def within_bound(cid, got, kernel, what):
    per = []
    for k, (g, (r, E)) in enumerate(zip(got, R.case_reference(cid))):
        assert bool(torch.isfinite(g).all()), "%s %s: head %d has %d elements that are not finite" % (cid, what, k, int((~torch.isfinite(g)).sum()))
        per.append(float(R.ratio(g, r["d"], E).max()))
    print("%-20s %-12s %-34s err/E per head: %s" % (cid, what, kernel, " ".join("%.4f" % x for x in per)))
    WORST[kernel] = max(WORST.get(kernel, 0.0), max(per))
    for k, x in enumerate(per):
        assert x <= 1.0, "%s %s (%s): head %d is at %.3f of its bound" % (cid, what, kernel, k, x)


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_heads_within_bound_and_forms_agree(eng, cid):
    c = R.make_case(cid)
    n, N = len(c["scores"]), c["N"]
    scores, fd = device_inputs(c)
    fused, names = run_heads(eng, scores, fd, c, True)
    want = R.expected_kernel(N, n, True)
    assert names == [want], (names, want)
    within_bound(cid, fused, want, "fused")
    again, _ = run_heads(eng, scores, fd, c, True)
    same_bits(fused, again, "%s: two runs of %s" % (cid, want))
    plain, names = run_heads(eng, scores, fd, c, False)
    assert names == ["dffw::regress_kernel"], names
    within_bound(cid, plain, "dffw::regress_kernel", "not fused")
    single = [eng.op_regress(s, fd, c["H"], c["W"]).cpu() for s in scores]
    within_bound(cid, single, "dffw::regress_kernel", "one by one")
    same_bits(plain, single, "%s: regress_kernel with %d heads vs one head per launch" % (cid, n))
    same_bits(fused, plain, "%s: %s vs regress_kernel" % (cid, want))


def test_dispatch_edges_are_covered():
    """The case list reaches each kernel on both sides of its N range, and the fused flag decides alone at N = 10 and 16."""
    by = {}
    for _, B, N, heads, _, _ in R.CASES:
        by.setdefault(R.expected_kernel(N, len(heads), True), set()).add(N)
    assert {1, 10} <= by["dffw::regress_fused_kernel<10>"] and {11, 16} <= by["dffw::regress_fused_kernel<16>"] and 17 in by["dffw::regress_kernel"]
    assert R.expected_kernel(10, 4, False) == R.expected_kernel(16, 2, False) == R.expected_kernel(5, 1, True) == "dffw::regress_kernel"


def test_refusals_leave_the_outputs_alone(eng):
    """With real device buffers: a size below 1, n_heads outside 1..4 and a null entry return DFFW_EINVAL from both entry points, launch nothing
    (dffw_last_op_kernels is empty) and write nothing."""
    B, N, h, w, H, W = 1, 2, 2, 2, 4, 4
    score = torch.zeros(B, N, h, w, device="cuda")
    fd = torch.ones(B, N, 1, 1, device="cuda").expand(B, N, H, W)
    G = GuardedMaps(2, B, H, W)
    maps = G.maps()
    dev = torch.cuda.current_device()
    st = (ctypes.c_int64 * 4)(*fd.stride())
    vp = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in ts])
    i4 = lambda v: (ctypes.c_int * 4)(*v)

    def many(n=2, scores=(score, score), hs=(h, h, 0, 0), ws=(w, w, 0, 0), **kw):
        a = dict(dict(B=B, N=N, H=H, W=W), **kw)
        return eng.lib.dffw_op_regress_heads(dev, n, vp(list(scores) + [None] * (4 - len(scores))), i4(hs), i4(ws), vp(maps + [None, None]),
                                             a["B"], a["N"], a["H"], a["W"], fd.data_ptr(), st, 1, None)

    for rc in (many(N=0), many(N=-1), many(B=0), many(H=0), many(W=0), many(n=0), many(n=5), many(hs=(h, 0, 0, 0)), many(ws=(0, w, 0, 0)),
               many(scores=(score, None)), many(n=3)):
        assert rc == -1, (rc, eng.lib.dffw_last_error())
        assert eng.op_kernels() == []
    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(H=0)):
        a = dict(dict(B=B, N=N, h=h, w=w, H=H, W=W), **kw)
        rc = eng.lib.dffw_op_regress(dev, score.data_ptr(), a["B"], a["N"], a["h"], a["w"], a["H"], a["W"], fd.data_ptr(), st, maps[0].data_ptr(), None)
        assert rc == -1 and b"bad shape" in eng.lib.dffw_last_error()
    with pytest.raises(ValueError):
        eng.op_regress_heads([score] * 5, fd, H, W)
    torch.cuda.synchronize()
    assert bool((G.buf == 0xFF).all())
