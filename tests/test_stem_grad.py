"""CPU: the weight gradient of the stem.  The emulation of the kernel's arithmetic (tests/stem_grad_ref.py) stays inside
the ALPHA * G bound at every shape and regime the GPU test runs, equals float64 autograd bit for bit on small integers, and every planted fault
stands at least 4x over the bound (or breaks the equality), so the GPU test would see it.  The refusals are those of the built library."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_grad_ref as sg  # noqa: E402
from oracle import error_bounds as eb  # noqa: E402

# (B, N, H, W), as tests/test_gpu_stem_grad.py: images smaller than the 17-pixel reach; odd sizes with exactly one in-image position for the
# outermost taps; no multiples of the tile, two samples and three slices; several units per workgroup on a grid of 8
SHAPES = [(1, 1, 1, 1), (1, 1, 4, 6), (1, 2, 17, 19), (2, 3, 20, 36), (2, 3, 32, 40), (1, 2, 128, 160)]
# every workgroup of a grid of 8 sums one full 16 384-pixel partial and starts a second: 131 072 pixels and more (see the GPU test)
FULL = (2, 5, 128, 128)


@functools.lru_cache(maxsize=None)
def case(regime, shape):
    x, gy = sg.make_case(regime, *shape, seed=23 + sum(shape))
    return x, gy, sg.wgrad_ref64(x, gy)


def ratio(got, r, prec):
    return eb.elementwise_ratio(got, r, prec)[0]


@pytest.mark.parametrize("prec", sg.PRECISIONS)
@pytest.mark.parametrize("regime", sg.REGIMES)
def test_emulation_within_the_bound(regime, prec):
    worst = 0.0
    for shape in SHAPES:
        x, gy, r = case(regime, shape)
        for wgs in (0, 8):
            worst = max(worst, eb.check_elementwise(sg.emulate(x, gy, prec, wgs=wgs), r, prec, "emulated grad_w %s %s wgs=%d" % (regime, shape, wgs)))
    # (no margin is asked here: at (1, 1, 1, 1) an element is ONE product, and the roundings of its two operands alone may take 3/4 of 2^-16)
    print("stem_grad emulation %s %s: worst err/bound %.3f" % (prec, regime, worst))


@pytest.mark.parametrize("regime", sg.REGIMES)
def test_emulation_at_full_length_partials(regime):
    """The fp32 accumulation at its full length: every workgroup of the grid of 8 sums 40 units, a whole 32-unit partial and the start of a second."""
    counts = sg.units_per_workgroup(*FULL, wgs=8)
    assert len(counts) == 8 and min(counts) > sg.FLUSH_UNITS, counts
    x, gy, r = case(regime, FULL)
    for prec in sg.PRECISIONS:
        worst = eb.check_elementwise(sg.emulate(x, gy, prec, wgs=8), r, prec, "emulated grad_w at full-length partials")
        print("stem_grad emulation full-length partials %s %s %s: err/bound %.3f" % (prec, regime, FULL, worst))
        assert worst < 0.5


@pytest.mark.parametrize("prec", sg.PRECISIONS)
def test_integers_equal_autograd(prec):
    for shape in SHAPES[1:5]:
        x, gy = sg.int_case(*shape, seed=5)
        ref = sg.wgrad64(x, gy)
        for wgs, flush in ((0, sg.FLUSH_UNITS), (8, 1)):
            assert torch.equal(sg.emulate(x, gy, prec, wgs=wgs, flush_units=flush).double(), ref), (shape, wgs)


# fault -> the regime in which it shows; offset inputs cancel nothing, so a dropped low-order product or a zero read as a neighbour stands out most
FAULT_REGIME = {"dilation1": "zero_mean", "swap_kykx": "zero_mean", "swap_planes": "zero_mean", "pad7": "zero_mean", "wrap_row": "offset",
                "drop_product": "offset", "missing_partial": "offset"}


@pytest.mark.parametrize("fault", sg.FAULTS)
def test_planted_faults_exceed_the_bound(fault):
    assert set(FAULT_REGIME) == set(sg.FAULTS)
    shape = (2, 3, 32, 40)
    x, gy, r = case(FAULT_REGIME[fault], shape)
    for prec in sg.PRECISIONS:
        if fault == "drop_product" and prec != "bf16x3":
            continue
        got = sg.emulate(x, gy, prec, wgs=8, fault=fault)
        assert ratio(got, r, prec) >= 4.0, (fault, prec, ratio(got, r, prec))
        assert ratio(sg.emulate(x, gy, prec, wgs=8), r, prec) < 0.5     # 3 840 pixels: far from the single product above
    xi, gi = sg.int_case(*shape, seed=9)
    if fault != "drop_product":   # (integers have no low part to drop)
        assert not torch.equal(sg.emulate(xi, gi, "bf16x3", wgs=8, fault=fault).double(), sg.wgrad64(xi, gi)), fault


def test_unit_helpers_follow_the_launch():
    assert sg.grid_x_of(1, 1, 1, 1) == 8 and sg.grid_x_of(4, 10, 224, 224) == 512 and sg.grid_x_of(4, 10, 224, 224, wgs=8) == 8
    assert sum(sg.units_per_workgroup(1, 2, 128, 160, wgs=8)) == 80 and sg.units_per_workgroup(2, 3, 20, 36) == [1] * 24


def test_kernel_names_are_symbols_of_the_library(lib_built, tmp_path):
    """What dffw_stem_wgrad reports through dffw_last_op_kernels (asserted on the GPU by tests/test_gpu_stem_grad.py) are the demangled symbols of
    gfx950 kernels in libdffw.so's code objects."""
    import re
    import subprocess
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import isa_compare as ic
    finally:
        sys.path.pop(0)
    mangled = []
    for co in ic.code_objects(lib_built, str(tmp_path)):
        mangled += list(ic.kernel_notes(co))
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    symbols = {re.sub(r"\(.*", "", d).replace("void ", "", 1) for d in demangled}
    for name in ["dffw::stem_wgrad_kernel<%d>" % p for p in range(3)] + ["dffw::stem_wgrad_finish_kernel"]:
        assert name in symbols, name


def test_refusals_without_gpu(lib_built):
    """Everything the stem backward does not serve is DFFW_EINVAL (-1) with a message, from the built library, before any launch and before the
    GPU is touched: this runs on a machine without one (dummy non-null, 16-byte-aligned addresses stand for the operands).  A short workspace
    is DFFW_ENOMEM (-3); dffw_stem_wgrad_workspace_bytes is positive for a served shape and 0 for a refused one."""
    lib = ctypes.CDLL(lib_built)
    lib.dffw_last_error.restype = ctypes.c_char_p
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.dffw_stem_wgrad_workspace_bytes.argtypes = [ci] * 4
    lib.dffw_stem_wgrad_workspace_bytes.restype = i64
    lib.dffw_stem_wgrad.argtypes = [ci, ci, vp, vp] + [ci] * 4 + [vp, vp, i64, vp]
    lib.dffw_op_stem_backward.argtypes = [ci, ci, vp, vp] + [ci] * 4 + [vp, vp]
    P = 4096   # never dereferenced: every call below is refused first
    ok = (1, 2, 17, 19)
    wsb = lib.dffw_stem_wgrad_workspace_bytes(*ok)
    assert wsb == 8 * sg.grid_x_of(*ok) * 8 * 243 and wsb > 0
    assert lib.dffw_stem_wgrad_workspace_bytes(4, 10, 224, 224) == 8 * 512 * 8 * 243

    def record(prec=0, x=P, gy=P, shape=ok, gw=P, ws=P, bytes_=wsb):
        return lib.dffw_stem_wgrad(0, prec, x, gy, *shape, gw, ws, bytes_, None)

    def op(prec=0, x=P, gy=P, shape=ok, gw=P):
        return lib.dffw_op_stem_backward(0, prec, x, gy, *shape, gw, None)

    def refused(rc, what):
        assert rc == -1 and lib.dffw_last_error(), (what, rc)

    too_large = ((32768, 1, 256, 256), (1, 65536, 256, 128), (2, 2, 32768, 16384))   # 2^31 pixels
    for bad in ((0, 2, 17, 19), (1, 0, 17, 19), (1, 2, 0, 19), (1, 2, 17, -3)) + too_large:
        assert lib.dffw_stem_wgrad_workspace_bytes(*bad) == 0, bad
        refused(record(shape=bad), bad)
        refused(op(shape=bad), bad)
    assert lib.dffw_stem_wgrad_workspace_bytes(32767, 1, 256, 256) > 0     # one sample below 2^31 pixels
    for prec in (-1, 3):
        refused(record(prec=prec), "precision %d" % prec)
        refused(op(prec=prec), "precision %d" % prec)
    for name in ("x", "gy", "gw"):
        refused(record(**{name: None}), "null " + name)
        refused(op(**{name: None}), "null " + name)
    refused(record(ws=None), "null workspace")
    refused(record(gy=P + 8), "grad_y off 16 bytes")
    assert record(bytes_=wsb - 8) == -3 and b"too small" in lib.dffw_last_error()
    assert record(bytes_=0) == -3
