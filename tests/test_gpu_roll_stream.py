"""GPU: the slice stream of the rolling conv kernels (dffw_conv_roll.hip, dffw_conv_rollx.hip; schedule: roll_sched / roll_step, dffw_conv_roll.h).

A unit's stream entries are real slices only, a step whose window lacks its front or back slice leaves that slice's contraction chunks out, and the
ring slot at that place holds a NEIGHBOURING unit's slice -- so a wrong chunk list, a wrong step count or a slice read from the wrong ring slot shows
up as a wrong value.  One conv per body through the single-operator entry point (the op's record workspace is poisoned with NaN: a slice no step
wrote fails the finiteness check), rolling kernels forced (DFFW_ROLL_MIN_UNITS=1), eight workgroups (DFFW_ROLL_WGS=8: a workgroup's stream crosses
many unit boundaries), B in {1, 3}, N in {1, 2, 3, 4} on 32 x 32 and 32 x 64 maps of the kernel's column grid, whole slice ranges and two ranges
per sample (DFFW_ROLL_ZSPLIT=2: ranges that start and end inside the volume), the straight-line and the generic epilogue (DFFW_NO_LEAN_ROLL: same
arithmetic, equal bit for bit).  The input is non-zero and carries a per-slice offset.  Held per element to the forward-error bound of
oracle/error_bounds.py against F.conv3d / F.conv_transpose3d in float64.

The two-source forms of these kernels (8 + 8 -> 8, 16 + 16 -> 16, ... over a virtual concat) run on the same slice stream, through
engine.op_conv3d_cat, in tests/test_gpu_conv_cat.py."""
import pytest
import torch

from oracle import error_bounds as eb
from test_gpu_ops import bn_params, bounded, rnd

pytestmark = pytest.mark.gpu

# (name, Cin, Cout, transposed, stride, residual, extra environment, kernel prefix)
CASES = [
    ("roll_16_16", 16, 16, False, 1, False, {}, "dffw::conv_roll<0, 8, 16, 4, 6, false, false,"),
    ("roll_16_16_res", 16, 16, False, 1, True, {}, "dffw::conv_roll<0, 8, 16, 4, 6, true, false,"),
    ("roll_16_8_pair_res", 16, 8, False, 1, True, {}, "dffw::conv_roll<0, 8, 16, 4, 6, true, true,"),
    ("roll_16_8_pair_serial", 16, 8, False, 1, False, {"DFFW_NO_ROLLX": "1"}, "dffw::conv_roll<0, 8, 16, 4, 6, false, true,"),
    ("rollx_pair_16_8", 16, 8, False, 1, False, {}, "dffw::conv_rollx_pair<"),
    ("rollx_k2_32_16", 32, 16, False, 1, False, {}, "dffw::conv_rollx_k2<"),
    ("efd_s2_8_16", 8, 16, False, 2, False, {}, "dffw::conv_roll_efd<0, 5, false,"),
    ("s2_16_16", 16, 16, False, 2, False, {}, "dffw::conv_roll_s2<0, 1, 1, 4,"),
    ("s2_16_32", 16, 32, False, 2, False, {}, "dffw::conv_roll_s2<0, 2, 1, 6,"),
    ("s2_32_64", 32, 64, False, 2, False, {}, "dffw::conv_roll_s2<0, 2, 2, 5,"),
    ("t_16_8", 16, 8, True, 2, False, {}, "dffw::conv_roll_t<0, 8, 16, 4, 6, false,"),
    ("t_16_8_res", 16, 8, True, 2, True, {}, "dffw::conv_roll_t<0, 8, 16, 4, 6, true,"),
    ("t32_32_16", 32, 16, True, 2, False, {"DFFW_NO_ROLLT": "1"}, "dffw::conv_roll_t32<0,"),
    ("t32_32_16_res", 32, 16, True, 2, True, {"DFFW_NO_ROLLT": "1"}, "dffw::conv_roll_t32<0,"),
]
# (B, N, rows, columns) of the kernel's column grid: the output of a stride-1 or strided conv, the input of a transposed one
SHAPES = [(1, 1, 32, 32), (3, 2, 32, 64), (1, 3, 32, 64), (3, 4, 32, 32), (3, 1, 32, 64), (1, 4, 32, 32)]
SWITCHES = ("DFFW_ROLL_MIN_UNITS", "DFFW_ROLL_WGS", "DFFW_ROLL_ZSPLIT", "DFFW_NO_LEAN_ROLL", "DFFW_NO_ROLLX", "DFFW_NO_ROLLT", "DFFW_NO_ROLL", "DFFW_NO_SMALL")


@pytest.fixture(scope="module")
def eng(lib_built):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dffinthewild_amd import engine
    return engine


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_n%d_%dx%d" % s)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_roll_stream(eng, case, shape, monkeypatch):
    name, cin, cout, transposed, stride, residual, extra, kernel = case
    B, N, gh, gw = shape
    H, W = (gh * 2, gw * 2) if (stride == 2 and not transposed) else (gh, gw)
    x = rnd(B, cin, N, H, W, seed=11) + 0.25 * torch.arange(1, N + 1, dtype=torch.float32).reshape(1, 1, N, 1, 1)   # every slice its own level
    w = rnd(*((cin, cout) if transposed else (cout, cin)), 3, 3, 3, seed=12, scale=(2.0 / (cin * 27)) ** 0.5 * 1.7)
    bn = bn_params(cout, 13)
    st = (1, stride, stride)
    oshape = (B, cout, N, 2 * H, 2 * W) if transposed else (B, cout, N, H // stride, W // stride)
    res = rnd(*oshape, seed=14) if residual else None
    r = eb.conv_ref64(x, w, stride=st, pad=1, transposed=transposed, bn=bn, residual=res, relu=1)
    kw = dict(stride=st, pad=1, transposed=transposed, bn=bn, residual=res.cuda() if residual else None, relu=1, precision="bf16x3")
    xd = x.cuda()
    base = dict(extra, DFFW_ROLL_MIN_UNITS="1", DFFW_ROLL_WGS="8")
    lean = None
    for zsplit in (1, 2):
        if zsplit > N:
            continue
        for generic in (False, True):
            _set(monkeypatch, dict(base, DFFW_ROLL_ZSPLIT=str(zsplit), **({"DFFW_NO_LEAN_ROLL": "1"} if generic else {})))
            got = eng.op_conv3d(xd, w, **kw)
            kn = eng.last_conv_kernel()
            assert kn.startswith(kernel), (name, kn)
            if kernel.endswith(","):   # the bodies with a straight-line epilogue: the switch picks the instantiation
                assert kn.endswith("false>" if generic else "true>"), (name, generic, kn)
            assert got.shape == r.ref.shape
            bounded(got, r, "bf16x3", kn, "%s zsplit %d %s" % (name, zsplit, "generic" if generic else "lean"))
            if not generic:
                lean = got
            else:
                assert torch.equal(got, lean), (name, zsplit, "the generic epilogue differs from the straight-line one")
        # a range boundary inside the volume changes which steps are dead, never a value
        if zsplit == 1:
            whole = lean
        else:
            assert torch.equal(lean, whole), (name, "two slice ranges per sample differ from whole ranges")
