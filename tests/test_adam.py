"""The Adam step without a GPU: the reference, the bounds and the emulation of tests/adam_ref.py against PyTorch's own fp32
Adam; the planted faults; the refusals of dffw_adam_step through ctypes, none of which touches a GPU; pipeline.Adam's refusals and state layout."""
import ctypes

import pytest
import torch

import adam_ref as R

N = 20000


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


def test_emulation_and_torch_adam_within_three_quarters_of_every_bound():
    """The kernel's operation order in fp32 (adam_ref.emulate) and torch.optim.Adam(foreach=False) on the CPU, on all CASES x t x lr: both within 0.75
    of the bounds on p, m and v.  This ties the formulas -- betas (0.9, 0.99), the bias corrections, eps outside the root -- and the state
    layout (step, exp_avg, exp_avg_sq) to PyTorch's."""
    worst = {}
    for case in R.all_cases(N):
        for name, fn in (("emulate", R.emulate), ("torch", R.torch_adam)):
            w = R.check(fn(case), case, name, limit=0.75)
            for k, x in w.items():
                worst[name, case["regime"], k] = max(worst.get((name, case["regime"], k), 0.0), x)
    for name in ("emulate", "torch"):
        for regime in R.CASES:
            print("%-8s %-10s worst err/bound  p %.3f  m %.3f  v %.3f" % ((name, regime) + tuple(worst[name, regime, k] for k in "pmv")))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_far_outside_the_bound(fault):
    """Each fault moves at least half of the elements more than 4x over the bound on p (plain case, t = 10; eps under the root on the zero-state
    case, where sqrt(v') is smallest).  lr = 0.1: at lr = 1e-4 an update is a ten-thousandth of p and most of a fault hides in p's own rounding."""
    case = R.make_case("first_step" if fault == "eps_under_sqrt" else "plain", N, 10, 1e-1)
    over = (R.ratios(R.faulty(case, fault), case)["p"] > 4).double().mean()
    print("%s: %.1f %% of the elements more than 4x over the p bound" % (fault, 100 * float(over)))
    assert float(over) >= 0.5


def _entry(eng, numel, ptrs=(0x1000, 0x2000, 0x3000, 0x4000)):
    return eng.AdamTensor(*ptrs, numel)


def _step(eng, entries, n=None, step=1, lr=1e-3, b1=0.9, b2=0.99, eps=1e-8):
    table = (eng.AdamTensor * max(len(entries), 1))(*entries) if entries is not None else None
    return eng.lib.dffw_adam_step(0, table, len(entries) if n is None else n, step, lr, b1, b2, eps, None)


def test_every_refusal_without_gpu(eng):
    """DFFW_EINVAL (-1) with a message, before any launch and before the GPU is touched (the pointers are not device memory: nothing reads them)."""
    ok = _entry(eng, 8)
    inf, nan = float("inf"), float("nan")
    refused = {
        "null list": dict(entries=None, n=1),
        "empty list": dict(entries=[], n=0),
        "negative count": dict(entries=[ok], n=-1),
        "numel < 0": dict(entries=[ok, _entry(eng, -1)]),
        "numel = 2^31": dict(entries=[_entry(eng, 1 << 31)]),
        "step 0": dict(entries=[ok], step=0),
        "step -3": dict(entries=[ok], step=-3),
        "lr nan": dict(entries=[ok], lr=nan), "lr inf": dict(entries=[ok], lr=inf), "lr < 0": dict(entries=[ok], lr=-1e-3),
        "eps nan": dict(entries=[ok], eps=nan), "eps inf": dict(entries=[ok], eps=inf), "eps < 0": dict(entries=[ok], eps=-1e-8),
        "beta1 nan": dict(entries=[ok], b1=nan), "beta1 = 1": dict(entries=[ok], b1=1.0), "beta1 < 0": dict(entries=[ok], b1=-0.1),
        "beta2 inf": dict(entries=[ok], b2=inf), "beta2 = 1": dict(entries=[ok], b2=1.0), "beta2 < 0": dict(entries=[ok], b2=-0.1),
    }
    for i in range(4):
        null = [0x1000, 0x2000, 0x3000, 0x4000]
        null[i] = 0
        refused["null pointer %d" % i] = dict(entries=[ok, _entry(eng, 8, null)])
        for off in (1, 2, 3):
            odd = [0x1000, 0x2000, 0x3000, 0x4000]
            odd[i] += off
            refused["pointer %d + %d bytes" % (i, off)] = dict(entries=[_entry(eng, 8, odd), ok])
    for what, kw in refused.items():
        entries = kw.pop("entries")
        rc = _step(eng, entries, **kw)
        assert rc == -1 and eng.lib.dffw_last_error(), (what, rc)
        assert eng.lib.dffw_last_op_kernels() == b"", what
    # engine.op_adam_step: the same refusal of an empty list as a ValueError, and no CPU fallback
    with pytest.raises(ValueError):
        eng.op_adam_step([], [], [], [], step=1, lr=1e-3)
    t = [torch.zeros(3)]
    with pytest.raises(eng.DffwError, match="no CPU fallback"):
        eng.op_adam_step(t, t, t, t, step=1, lr=1e-3)
    with pytest.raises(ValueError, match="float32"):
        eng.op_adam_step(t, [torch.zeros(3, dtype=torch.float64)], t, t, step=1, lr=1e-3)
    with pytest.raises(ValueError, match="contiguous"):
        eng.op_adam_step([torch.zeros(3, 2).t()], [torch.zeros(2, 3)], [torch.zeros(2, 3)], [torch.zeros(2, 3)], step=1, lr=1e-3)
    with pytest.raises(ValueError, match="shape"):
        eng.op_adam_step(t, t, [torch.zeros(4)], t, step=1, lr=1e-3)


def test_all_empty_list_is_ok_without_a_launch(eng):
    """Entries with numel == 0 are skipped -- their pointers may be null -- and a list of nothing else returns DFFW_OK without touching the GPU."""
    assert _step(eng, [_entry(eng, 0), _entry(eng, 0, (0, 0, 0, 0))]) == 0
    assert eng.lib.dffw_last_op_kernels() == b""


def test_tensors_per_launch(eng):
    assert eng.lib.dffw_adam_tensors_per_launch() == eng.ADAM_TENSORS_PER_LAUNCH >= 16


def test_pipeline_adam_refuses_what_is_not_built(eng):
    from dffinthewild_amd import pipeline
    p = [torch.nn.Parameter(torch.zeros(3))]
    for name, value in (("weight_decay", 1e-4), ("amsgrad", True), ("maximize", True)):
        with pytest.raises(ValueError, match=name):
            pipeline.Adam(p, lr=1e-3, **{name: value})
    opt = pipeline.Adam(p, lr=1e-3)
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    assert opt.step() is None and len(opt.state) == 0      # no gradient anywhere: nothing to update, nothing reaches the library
    # ... and a checkpoint of torch.optim.Adam that brings one of them is refused at the step
    opt.load_state_dict(torch.optim.Adam(p, lr=1e-3, weight_decay=1e-2).state_dict())
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()
    p[0].grad = torch.ones(3)
    opt = pipeline.Adam(p, lr=1e-3)
    with pytest.raises(eng.DffwError, match="no CPU fallback"):
        opt.step()
    assert float(opt.state[p[0]]["step"]) == 0.0           # a refused step is not counted


def test_pipeline_adam_state_dict_has_torch_adams_keys(eng):
    """A fresh pipeline.Adam over CPU-built parameters: the state_dict of torch.optim.Adam with the same options, key for key and value for value,
    with betas (0.9, 0.99) as its own default; each class loads the other's."""
    from dffinthewild_amd import pipeline
    params = [torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(4, 2, 3))]
    ours = pipeline.Adam([dict(params=params[:1]), dict(params=params[1:], lr=1e-2)], lr=1e-4)
    theirs = torch.optim.Adam([dict(params=params[:1]), dict(params=params[1:], lr=1e-2)], lr=1e-4, betas=(0.9, 0.99))
    a, b = ours.state_dict(), theirs.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"} and a["state"] == b["state"] == {}
    assert len(a["param_groups"]) == len(b["param_groups"]) == 2
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert set(ga) == set(gb) and ga == gb
    assert ours.defaults["betas"] == (0.9, 0.99) and ours.defaults["eps"] == 1e-8
    ours.load_state_dict(b)
    theirs.load_state_dict(a)
