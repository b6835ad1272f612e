"""Train-mode BatchNorm3d without a GPU: the library exports and binds the entry points; the CPU restatement of the kernels'
arithmetic (bn_ref.emulate) stays under the per-element bounds of bn_ref for every regime, precision and channel count; with integer data the sums
equal float64 autograd bit for bit; planted faults exceed a bound at least 4x; ALPHA is what the recorded calibration gives."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402

SYMBOLS = ("dffw_bn_train_workspace_bytes", "dffw_bn_train_forward", "dffw_bn_train_backward", "dffw_op_bn_train", "dffw_op_bn_train_backward")


def test_library_exports_and_engine_binds_the_entry_points(lib_built):
    lib = ctypes.CDLL(lib_built)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    from dffinthewild_amd import engine, pipeline
    for name in SYMBOLS:
        assert name in engine.ABI_SYMBOLS and getattr(engine.lib, name).argtypes is not None, name
    assert callable(engine.op_bn_train) and callable(engine.op_bn_train_backward) and engine.BN_EPS == R.BN_EPS
    assert issubclass(pipeline.BatchNorm3d, torch.autograd.Function) and callable(pipeline.batch_norm3d)


def test_workspace_holds_only_the_workgroups_partials(lib_built, monkeypatch):
    """Bytes = grid * 2 * C float64, nothing that scales with M beyond the grid's cap; refused shapes give 0 (decided on the host: no GPU needed)."""
    from dffinthewild_amd import engine
    ws = engine.lib.dffw_bn_train_workspace_bytes
    monkeypatch.delenv("DFFW_BN_WGS", raising=False)
    for C in R.CHANNELS:
        for B, N, H, W in R.SHAPES + [(8, 10, 256, 256)]:
            assert ws(B, C, N, H, W) == R.grid_of(B * N * H * W) * 2 * C * 8
    assert ws(32, 64, 10, 256, 256) == 512 * 2 * 64 * 8
    assert ws(1, 12, 1, 4, 4) == 0 and ws(1, 8, 1, 1, 1) == 0 and ws(1, 256, 1, 4, 4) == 0 and ws(2, 8, 1024, 1024, 1024) == 0
    monkeypatch.setenv("DFFW_BN_WGS", "4")
    assert ws(3, 16, 4, 24, 40) == 8 * 2 * 16 * 8


def test_cpu_tensors_raise(lib_built):
    from dffinthewild_amd import engine, pipeline
    x, v = torch.zeros(1, 8, 1, 2, 2), torch.ones(8)
    with pytest.raises(RuntimeError):
        engine.op_bn_train(x, v, v)
    with pytest.raises(RuntimeError):
        engine.op_bn_train_backward(x, x, x, v, v, v)
    with pytest.raises(RuntimeError):
        pipeline.batch_norm3d(x, v, v)


def test_alpha_is_four_times_the_recorded_calibration():
    assert R.ALPHA == R.alpha_from(R.CALIBRATED_WORST) == 2.0 ** -13


def test_calibration_reproduces():
    """torch's float32 CPU batch_norm over the GPU test's cases: its worst err / bracket is what bn_ref records, within the slack another torch build's
    summation order may cost (a factor 2 either way), and ALPHA covers it."""
    worst = max(v[0] for v in R.calibrate(verbose=True).values())
    print("calibration worst %.3e (recorded %.3e), ALPHA 2^%d" % (worst, R.CALIBRATED_WORST, torch.log2(torch.tensor(R.ALPHA))))
    assert R.CALIBRATED_WORST / 2 <= worst <= R.CALIBRATED_WORST * 2 and worst < R.ALPHA


@functools.lru_cache(maxsize=None)
def case(regime, C, si):
    return R.make_case(regime, C, R.SHAPES[si], R.case_seed(regime, C, si))


def worst_ratios(regime, C, si, prec, relu, residual, **kw):
    c = case(regime, C, si)
    got = R.emulate(c, prec, relu, residual, **kw)
    r = R.reference(c, prec, relu, residual, y_stored=got["y"] if relu else None)
    n, ok = R.mask_disagreements(got["y"], r, prec) if relu else (0, True)
    assert ok, "a ReLU mask differs where |z64| is above the forward bound"
    return R.ratios(got, r, prec), got, r


@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("regime", R.REGIMES)
def test_emulation_stays_under_the_bounds(regime, C, prec):
    worst = {}
    for si in (0, 1, 2):
        for relu, residual in ((False, False), (True, True)) if si else ((False, False), (True, False), (False, True), (True, True)):
            q, _, _ = worst_ratios(regime, C, si, prec, relu, residual)
            for k, v in q.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("bn emulation %s C=%d %s: worst err/bound %s" % (regime, C, prec, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_emulation_on_a_small_grid_walks_many_units(prec):
    """DFFW_BN_WGS=4 at the largest shape: 8 workgroups, 2 or 3 units each; another order of the float64 additions, the same bounds."""
    q, got, _ = worst_ratios("offset", 16, 3, prec, True, True, wgs=4)
    assert R.grid_of(3 * 4 * 24 * 40, 4) == 8 and max(q.values()) <= 1.0, q
    q2, got2, _ = worst_ratios("offset", 16, 3, prec, True, True)
    assert max(q2.values()) <= 1.0, q2


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_constant_channel_gives_the_rounded_beta_exactly(prec):
    for si in (1, 2):
        c = case("constant", 16, si)
        got = R.emulate(c, prec, False, False)
        k = R.const_channel(16)
        want = R.rounded(c["beta"][k], prec)
        assert bool((got["y"][:, k] == want).all()) and float(got["mean"][k]) == R.CONST_VALUE
        assert float(got["invstd"][k]) == float(torch.tensor(1.0 / R.BN_EPS ** 0.5, dtype=torch.float64).float())


def test_integer_data_sums_equal_float64_autograd_bit_for_bit():
    """Integer-valued x and grad_y, gamma = 1, beta = 0: every term of the four sums is an integer or an exact float64 product, so the two-stage sums
    are exact: sum x, sum x^2 (through mean and var) and dbeta equal float64 autograd's bit for bit on any grid."""
    g = torch.Generator().manual_seed(3)
    shape = R.SHAPES[3]
    C = 8
    full = (shape[0], C) + shape[1:]
    c = dict(x=torch.randint(-8, 9, full, generator=g).float(), gy=torch.randint(-4, 5, full, generator=g).float(), gamma=torch.ones(C), beta=torch.zeros(C),
             res=torch.zeros(full), rm0=torch.zeros(C), rv0=torch.ones(C))
    for wgs in (0, 4):
        got = R.emulate(c, "bf16x3", False, False, wgs=wgs)
        r = R.reference(c, "bf16x3", False, False)
        M = r["M"]
        xs = c["x"].double()
        S0, S1 = xs.sum(dim=(0, 2, 3, 4)), (xs * xs).sum(dim=(0, 2, 3, 4))
        mean, var = S0 / M, S1 / M - (S0 / M) ** 2
        assert torch.equal(got["mean"], mean.float()) and torch.equal(got["invstd"], (1.0 / torch.sqrt(var + R.BN_EPS)).float())
        assert torch.equal(got["dbeta"].double(), r["dbeta"])   # integers: exact in float32 and float64
        assert torch.equal(got["rm"], (0.1 * mean).float())


# fault -> (regime, shape index, relu, residual): a case in which the fault acts
FAULTS = {
    "unbiased_invstd": ("zero_mean", 1, False, False),
    "biased_running_var": ("zero_mean", 1, False, False),
    "eps_outside": ("constant", 2, False, False),
    "no_dgamma_term": ("zero_mean", 2, False, False),
    "mask_from_gy": ("zero_mean", 2, True, False),
    "grad_res_unmasked": ("zero_mean", 2, True, True),
    "missing_partial": ("post_relu", 3, False, False),
    "fp32_var": ("offset", 3, False, False),
}


@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_faults_exceed_a_bound(fault, prec):
    regime, si, relu, residual = FAULTS[fault]
    c = case(regime, 16, si)
    got = R.emulate(c, prec, relu, residual, fault=fault)
    # the reference takes the mask an honest forward stored (a planted mask fault must not move the reference with it)
    honest = R.emulate(c, prec, relu, residual)
    r = R.reference(c, prec, relu, residual, y_stored=honest["y"] if relu else None)
    q = R.ratios(got, r, prec)
    print("bn fault %s %s: err/bound %s" % (fault, prec, " ".join("%s %.3g" % kv for kv in q.items())))
    assert max(q.values()) >= 4.0, q
    assert max(R.ratios(honest, r, prec).values()) <= 1.0
