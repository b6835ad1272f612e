"""Reference, bounds and a CPU emulation for the Adam step; shared by tests/test_adam.py and tests/test_gpu_adam.py.

Reference: the formulas in float64, evaluated from the fp32 inputs, with t the step count after the increment:

    m' = b1 m + (1 - b1) g      v' = b2 v + (1 - b2) g^2      d = sqrt(v') / sqrt(1 - b2^t) + eps      p' = p - s m' / d,  s = lr / (1 - b1^t)

Bounds, per element, with u = 2^-24 (fp32 unit roundoff), tiny = 2^-149 (the smallest fp32 subnormal) and A = b1 |m| + (1 - b1) |g|:

    |m_gpu - m'| <= 4 u A + tiny             two products by scalars rounded to fp32 (2 u each), one addition (u), first order; the cancellation
                                             between m and g is measured by A, not by |m'|
    |v_gpu - v'| <= 4 u v' + tiny            b2 v: 2 u; (1 - b2) (g g): 3 u; the sum of two non-negative terms: u; at most 4 u relative
    |p_gpu - p'| <= 2 u |p'| + 16 u s A / d + tiny
                                             the update s m' / d: m' 4 u A / |m'| relative, d half of v's 4 u plus sqrt, the division by the rounded
                                             sqrt(1 - b2^t) (2 u) and the addition of the rounded eps (2 u at most): 7 u; the quotient, the rounded s and
                                             their product 3 u; together 14 u, written 16 u s A / d with |m'| <= A; the final subtraction u (|p'| + |update|)
The constants come from this count and from the CPU runs of tests/test_adam.py (PyTorch's own fp32 Adam and the emulation stay under 0.75 of
each); they are never tuned against what the GPU gives.
"""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
BETAS = (0.9, 0.99)       # the reference training scripts'
EPS = 1e-8
STEPS = (1, 2, 10, 1000, 100000)
LRS = (1e-4, 1e-1)
CASES = ("plain", "cancel", "first_step", "tiny")
FAULTS = ("no_bias_correction_m", "no_bias_correction_v", "t_minus_1", "eps_under_sqrt", "g_for_g2", "betas_swapped")
ZERO_GRAD_SHARE = 0.05


def make_case(regime, n, t, lr, seed=0, betas=BETAS, eps=EPS):
    """{p, g, m, v: fp32 (n,), t, lr, betas, eps}.  plain: p ~ N(0, 1), g ~ 0.1 N, m ~ 0.1 N, v ~ 0.01 N^2.  cancel: b1 m is -(1 - b1) g up to
    a relative 1e-6, so that m' is a millionth of its two terms.  first_step: zero state.  tiny: p, g, m around 1e-24 and v among the fp32
    subnormals (g^2 itself underflows to zero).  In every regime 5 % of the gradients are exactly zero."""
    assert regime in CASES, regime
    gen = torch.Generator().manual_seed(1000 * CASES.index(regime) + seed)
    r = lambda: torch.randn(n, generator=gen, dtype=torch.float64)   # noqa: E731
    p, g, m, v = r(), 0.1 * r(), 0.1 * r(), 0.01 * r() ** 2
    if regime == "cancel":
        m = -(1 - betas[0]) / betas[0] * g * (1 + 1e-6 * r())
    elif regime == "first_step":
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    elif regime == "tiny":
        p, g, m, v = 1e-24 * p, 1e-23 * g, 1e-23 * m, 1e-40 * v
    g = torch.where(torch.rand(n, generator=gen) < ZERO_GRAD_SHARE, torch.zeros(()).double(), g)
    return dict(p=p.float(), g=g.float(), m=m.float(), v=v.float(), t=int(t), lr=float(lr), betas=tuple(betas), eps=float(eps), regime=regime)


def all_cases(n, seed=0):
    for regime in CASES:
        for t in STEPS:
            for lr in LRS:
                yield make_case(regime, n, t, lr, seed)


def _formulas(case, fault=None):
    """(p', m', v', d, s) in float64 from the fp32 inputs; ``fault`` plants one of FAULTS."""
    assert fault in (None,) + FAULTS, fault
    p, g, m, v = (case[k].double() for k in "pgmv")
    (b1, b2), t, lr, eps = case["betas"], case["t"], case["lr"], case["eps"]
    if fault == "betas_swapped":
        b1, b2 = b2, b1
    tt = t - 1 if fault == "t_minus_1" else t
    bc1 = 1.0 if fault == "no_bias_correction_m" else 1.0 - b1 ** tt
    bc2 = 1.0 if fault == "no_bias_correction_v" else 1.0 - b2 ** tt
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * (g.abs() if fault == "g_for_g2" else g * g)
    if fault == "eps_under_sqrt":
        d = torch.sqrt(v1 + eps) / bc2 ** 0.5
    else:
        d = torch.sqrt(v1) / bc2 ** 0.5 + eps
    s = lr / bc1
    return p - s * m1 / d, m1, v1, d, s


def reference(case):
    """{p, m, v}: float64, from the fp32 inputs."""
    p1, m1, v1, _, _ = _formulas(case)
    return dict(p=p1, m=m1, v=v1)


def faulty(case, fault):
    p1, m1, v1, _, _ = _formulas(case, fault)
    return dict(p=p1, m=m1, v=v1)


def bound(case):
    """{p, m, v}: the per-element bounds of the module docstring."""
    p1, _, v1, d, s = _formulas(case)
    b1 = case["betas"][0]
    A = b1 * case["m"].double().abs() + (1 - b1) * case["g"].double().abs()
    return dict(p=2 * U * p1.abs() + 16 * U * s * A / d + TINY, m=4 * U * A + TINY, v=4 * U * v1 + TINY)


def scalars(case):
    """The step's seven fp32 scalars as dffw_adam_step computes them: in double, rounded once."""
    (b1, b2), t, lr, eps = case["betas"], float(case["t"]), case["lr"], case["eps"]
    f = np.float32
    return dict(beta1=f(b1), beta2=f(b2), c1=f(1.0 - b1), c2=f(1.0 - b2), bc2_sqrt=f((1.0 - b2 ** t) ** 0.5), step_size=f(lr / (1.0 - b1 ** t)), eps=f(eps))


def emulate(case):
    """dffw::adam_kernel's adam_one() in NumPy float32, one rounding per operation in the kernel's order.  {p, m, v}: fp32 tensors."""
    k = scalars(case)
    p, g, m, v = (case[x].numpy() for x in "pgmv")
    with np.errstate(all="ignore"):
        mn = k["beta1"] * m + k["c1"] * g
        vn = k["beta2"] * v + k["c2"] * (g * g)
        d = np.sqrt(vn) / k["bc2_sqrt"] + k["eps"]
        pn = p - k["step_size"] * (mn / d)
    assert pn.dtype == mn.dtype == vn.dtype == np.float32
    return dict(p=torch.from_numpy(pn), m=torch.from_numpy(mn), v=torch.from_numpy(vn))


def torch_adam(case, device="cpu", **kw):
    """torch.optim.Adam(foreach=False) for one step from the case's state at step t - 1.  {p, m, v}: fp32 tensors on ``device``."""
    p = torch.nn.Parameter(case["p"].clone().to(device))
    opt = torch.optim.Adam([p], lr=case["lr"], betas=case["betas"], eps=case["eps"], foreach=False, **kw)
    opt.state[p] = dict(step=torch.tensor(float(case["t"] - 1)), exp_avg=case["m"].clone().to(device), exp_avg_sq=case["v"].clone().to(device))
    p.grad = case["g"].clone().to(device)
    opt.step()
    assert float(opt.state[p]["step"]) == case["t"]
    return dict(p=p.detach(), m=opt.state[p]["exp_avg"], v=opt.state[p]["exp_avg_sq"])


def ratios(got, case):
    """{p, m, v}: err / bound per element against the float64 reference (NaN where a result is NaN)."""
    ref, bnd = reference(case), bound(case)
    return {k: (got[k].detach().cpu().double() - ref[k]).abs() / bnd[k] for k in "pmv"}


def worst_ratio(got, case):
    """{p, m, v}: the largest err / bound; a NaN anywhere gives inf."""
    out = {}
    for k, r in ratios(got, case).items():
        out[k] = float("inf") if bool(torch.isnan(r).any()) else float(r.max())
    return out


def check(got, case, what="", limit=1.0):
    """Asserts every element of p, m and v within ``limit`` times its bound; returns the worst ratios."""
    w = worst_ratio(got, case)
    assert all(x <= limit for x in w.values()), "%s (%s t=%d lr=%g): worst err/bound p %.3g m %.3g v %.3g" % (
        what, case.get("regime", "?"), case["t"], case["lr"], w["p"], w["m"], w["v"])
    return w


def same_bits(a, b):
    """fp32 tensors equal bit for bit (so +0 and -0, and two NaN patterns, differ)."""
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))
