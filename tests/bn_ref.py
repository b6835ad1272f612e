"""Reference, bounds and a CPU emulation for train-mode BatchNorm3d; shared by tests/test_bn_train.py and
tests/test_gpu_bn_train.py.

Reference.  float64 ``F.batch_norm(training=True)`` plus the residual add and ReLU, evaluated on the record-rounded tensors
``sum(round_parts(t, prec))`` (x, the residual and grad_y), so input rounding is not charged; the backward is float64 autograd of that graph.
For the backward the ReLU mask may be taken from a stored ``y`` (what the GPU forward wrote) instead of float64 ``z``: a ``z`` within rounding
of 0 may fall either way.  ``mask_disagreements`` lists those elements; each must have ``|z64|`` below the forward bound there.

Bounds, per element, in float64; ``u`` = storage unit of the format (U), ``m`` = momentum, sums per channel over the M pixels:

    |y  - y64 | <= u |y64|  + ALPHA ( |gamma| (|xh| + 1) + |beta| + |res| )
    |gx - gx64| <= u |gx64| + ALPHA |gamma| invstd ( |g| + sum|g| / M + (|xh| + 1) sum|g xh| / M )
    |dbeta - dbeta64| <= ALPHA sum|g|            |dgamma - dgamma64| <= ALPHA sum |g| (|xh| + 1)
    |mean - mean64| <= ALPHA (|mean64| + sigma64)       |invstd - invstd64| <= ALPHA invstd64
    |grad_res - g64| <= u |g64|                  (a masked copy of a record)
    running_mean: m ALPHA (|mean64| + sigma64) + 2^-24 |r64|     running_var: m 2 ALPHA (var64 M/(M-1) + eps) + 2^-24 |r64|

The running statistics' bounds are "the statistic's own bound scaled by m" (a relative ALPHA on invstd is a relative 2 ALPHA on var + eps) plus the
float32 storage of the result: the updated value is rounded to float32 once, half an ulp = 2^-24 of its size, and that is NOT covered by the
m-scaled term when the batch statistic is small against the carried value (a constant channel has var = 0: the m-scaled term is 2 m ALPHA eps,
while rounding (1 - m) running_var costs up to 2^-24 of it -- PyTorch's own float32 update misses the bound without that term).

ALPHA and its calibration (the way loss_ref.py did it).  ``calibrate()`` runs PyTorch's float32 CPU ``F.batch_norm`` forward and autograd backward
over the GPU test's own cases (CASES below: four shapes, five regimes, relu x residual) against the float64 reference and takes, for every
quantity, the worst err divided by the bracketed term.  Measured (torch CPU float32), in units of 2^-24: y 334.7 (the constant channel: PyTorch
folds the shift, and beta - mean gamma invstd cancels against x gamma invstd at invstd = 316), grad_x 11.1, dgamma 8.6, invstd 2.8, mean 2.3,
dbeta 1.0; the worst, CALIBRATED_WORST = 1.995e-5, x 4, rounded up to a power of two: ALPHA = 2^-13.  The running statistics are not part of
the calibration (PyTorch updates them in float32 with several roundings of the carried value, which says nothing about the statistic); they take
the same ALPHA.  The GPU's own worst ratios are recorded in DESIGN.md section 14; they are never used to set ALPHA.
"""
import math

import torch
import torch.nn.functional as F

import conv_grad_ref as cg

BN_EPS = 1e-5
MOMENTUM = 0.1
PRECISIONS = cg.PRECISIONS
U = {"bf16x3": 2.0 ** -16, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
CHANNELS = (8, 16, 32, 64, 128)
# (B, N, H, W): M = 2, the smallest legal; M = 210, a ragged tail in every grouping; several workgroups; (with DFFW_BN_WGS=4) one workgroup walks many units
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 7), (1, 2, 40, 24), (3, 4, 24, 40)]
REGIMES = ("zero_mean", "post_relu", "offset", "constant", "one_sample")
CONST_VALUE = 1.5          # the constant channel's value
UNIT_PIX, DEFAULT_WGS = 512, 512   # what dffw_bn.h fixes

CALIBRATED_WORST = 1.995e-5   # calibrate(): torch CPU float32, y in the constant regime
ALPHA = 2.0 ** -13


def const_channel(C):
    return C // 2 + 1


def make_case(regime, C, shape, seed):
    """float32 CPU tensors of one case: x, gamma, beta, res, gy, rm0, rv0 (the running statistics start from non-trivial values)."""
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    full = (B, C, N, H, W)
    x = torch.randn(*full, generator=g)
    gy = torch.randn(*full, generator=g)
    if regime == "post_relu":
        x = F.relu(x)
    elif regime == "offset":          # mean = 100 sigma in every channel at every M (M = 2 included): the cancellation case of the variance
        mu = x.mean(dim=(0, 2, 3, 4), keepdim=True)
        x = 0.5 * (x - mu) / (x - mu).pow(2).mean(dim=(0, 2, 3, 4), keepdim=True).sqrt() + 50.0
    elif regime == "constant":
        x[:, const_channel(C)] = CONST_VALUE
    elif regime == "one_sample":      # every other sample of the batch contributes exact zeros to the backward sums
        gy[:B - 1] = 0.0
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.rand(C, generator=g) - 0.5
    res = torch.randn(*full, generator=g)
    rm0 = torch.randn(C, generator=g) * 0.5
    rv0 = 0.5 + torch.rand(C, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, res=res, gy=gy, rm0=rm0, rv0=rv0, regime=regime, C=C, shape=shape)


def rounded(t, prec):
    return sum(cg.round_parts(t, prec))


def _ch(v):
    return v.reshape(1, -1, 1, 1, 1)


def _csum(t):
    return t.sum(dim=(0, 2, 3, 4))


def reference(case, prec, relu, residual, y_stored=None, eps=BN_EPS, momentum=MOMENTUM):
    """The float64 reference and everything the bounds need, as a dict of float64 CPU tensors.  ``prec`` None: the tensors as they are."""
    rd = (lambda t: t.double()) if prec is None else (lambda t: rounded(t, prec).double())
    x = rd(case["x"]).requires_grad_(True)
    gy = rd(case["gy"])
    res = rd(case["res"]).requires_grad_(True) if residual else None
    gamma = case["gamma"].double().requires_grad_(True)
    beta = case["beta"].double().requires_grad_(True)
    rm, rv = case["rm0"].double().clone(), case["rv0"].double().clone()
    M = x.numel() // x.shape[1]
    z = F.batch_norm(x, rm, rv, gamma, beta, True, momentum, eps)
    if residual:
        z = z + res
    y = F.relu(z) if relu else z
    xd = x.detach()
    mean = _csum(xd) / M
    var = _csum((xd - _ch(mean)) ** 2) / M
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (xd - _ch(mean)) * _ch(invstd)
    if relu:
        mask = (y_stored.detach().cpu().double() > 0) if y_stored is not None else (z.detach() > 0)
        g = gy * mask
    else:
        g = gy
    ins = (x, gamma, beta) + ((res,) if residual else ())
    grads = torch.autograd.grad(z, ins, g)
    return dict(y=y.detach(), z=z.detach(), mean=mean, var=var, sigma=var.sqrt(), invstd=invstd, xh=xh, g=g, gx=grads[0], dgamma=grads[1], dbeta=grads[2],
                gres=grads[3] if residual else None, rm=rm, rv=rv, gamma=gamma.detach(), beta=beta.detach(), res=res.detach() if residual else None,
                M=M, eps=eps, momentum=momentum, relu=relu)


def brackets(r):
    """The bracketed terms of the bounds (what ALPHA multiplies), per quantity."""
    M, ga = r["M"], _ch(r["gamma"].abs())
    sg, sgx = _csum(r["g"].abs()), _csum((r["g"] * r["xh"]).abs())
    y = ga * (r["xh"].abs() + 1) + _ch(r["beta"].abs()) + (r["res"].abs() if r["res"] is not None else 0.0)
    gx = ga * _ch(r["invstd"]) * (r["g"].abs() + _ch(sg) / M + (r["xh"].abs() + 1) * _ch(sgx) / M)
    return dict(y=y, gx=gx, dbeta=sg, dgamma=_csum(r["g"].abs() * (r["xh"].abs() + 1)), mean=r["mean"].abs() + r["sigma"], invstd=r["invstd"],
                rm=r["momentum"] * (r["mean"].abs() + r["sigma"]), rv=r["momentum"] * 2 * (r["var"] * M / (M - 1) + r["eps"]))


def bounds(r, prec, alpha=ALPHA):
    u, b = U[prec], brackets(r)
    out = {k: alpha * v for k, v in b.items()}
    out["y"] = out["y"] + u * r["y"].abs()
    out["gx"] = out["gx"] + u * r["gx"].abs()
    out["rm"] = out["rm"] + 2.0 ** -24 * r["rm"].abs()
    out["rv"] = out["rv"] + 2.0 ** -24 * r["rv"].abs()
    if r["gres"] is not None:
        out["gres"] = u * r["g"].abs()
    return out


QUANTITIES = ("y", "mean", "invstd", "rm", "rv", "gx", "gres", "dgamma", "dbeta")


def ratios(got, r, prec, alpha=ALPHA):
    """Worst err / bound of every quantity in ``got`` (a dict keyed like QUANTITIES; missing or None entries are skipped).  0 / 0 counts as 0; a NaN
    or an error against a zero bound as inf."""
    bd, out = bounds(r, prec, alpha), {}
    for k in QUANTITIES:
        if got.get(k) is None or r.get(k) is None:
            continue
        err = (got[k].detach().cpu().double() - r[k]).abs()
        q = torch.where(err == 0, torch.zeros_like(err), err / bd[k])
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        out[k] = float(q.max())
    return out


def mask_disagreements(y_stored, r, prec, alpha=ALPHA):
    """(count, ok): the elements where the stored y's ReLU mask differs from float64 z's, and whether each has |z64| under the forward bound."""
    differ = (y_stored.detach().cpu().double() > 0) != (r["z"] > 0)
    ok = bool((r["z"].abs()[differ] <= (bounds(r, prec, alpha)["y"])[differ]).all())
    return int(differ.sum()), ok


# ---- calibration of ALPHA: PyTorch's float32 CPU batch_norm against the float64 reference ---------------------------------------------------------
# the GPU test's cases: (regime, C, shape index); every regime at every shape, the channel counts spread over them
CASES = [(regime, CHANNELS[(i + j) % 5], j) for i, regime in enumerate(REGIMES) for j in range(len(SHAPES))]


def case_seed(regime, C, si):
    return 101 + 7 * REGIMES.index(regime) + 31 * C + 1009 * si


def torch_f32(case, relu, residual, eps=BN_EPS, momentum=MOMENTUM):
    """PyTorch's own float32 CPU forward and autograd backward on the (bf16x3-rounded, i.e. float32-exact) tensors."""
    x = rounded(case["x"], "bf16x3").requires_grad_(True)
    gy = rounded(case["gy"], "bf16x3")
    res = rounded(case["res"], "bf16x3").requires_grad_(True) if residual else None
    gamma, beta = case["gamma"].clone().requires_grad_(True), case["beta"].clone().requires_grad_(True)
    rm, rv = case["rm0"].clone(), case["rv0"].clone()
    z = F.batch_norm(x, rm, rv, gamma, beta, True, momentum, eps)
    if residual:
        z = z + res
    y = F.relu(z) if relu else z
    grads = torch.autograd.grad(y, (x, gamma, beta) + ((res,) if residual else ()), gy)
    M = x.numel() // x.shape[1]
    xd = x.detach()
    mean = _csum(xd) / M     # PyTorch does not hand out save_mean / save_invstd; the float32 statistics a user would compute
    invstd = 1.0 / torch.sqrt(_csum((xd - _ch(mean)) ** 2) / M + eps)
    return dict(y=y.detach(), gx=grads[0], dgamma=grads[1], dbeta=grads[2], gres=grads[3] if residual else None, rm=rm, rv=rv, mean=mean, invstd=invstd)


def calibrate(verbose=False):
    """Worst err / bracket of torch CPU float32 per quantity over CASES x relu x residual (float32 results: no storage term; the running
    statistics against their m-scaled bracket plus the float32 storage of the value)."""
    worst = {}
    for regime, C, si in CASES:
        case = make_case(regime, C, SHAPES[si], case_seed(regime, C, si))
        for relu in (False, True):
            for residual in (False, True):
                got = torch_f32(case, relu, residual)
                r = reference(case, "bf16x3", relu, residual, y_stored=got["y"] if relu else None)
                b = brackets(r)
                for k in ("y", "gx", "dgamma", "dbeta", "mean", "invstd"):
                    err = (got[k].double() - r[k]).abs()
                    q = torch.where(err == 0, torch.zeros_like(err), err / b[k])
                    q = float(q.max())
                    if q > worst.get(k, (0.0,))[0]:
                        worst[k] = (q, regime, C, SHAPES[si], relu, residual)
    if verbose:
        for k, v in worst.items():
            print("calibration %-7s worst err/bracket %.3e = %.2f * 2^-24  at %s" % (k, v[0], v[0] * 2 ** 24, v[1:]))
    return worst


def alpha_from(worst):
    return 2.0 ** math.ceil(math.log2(4 * worst))


# ---- CPU emulation of the kernels of dffw_bn.hip ----------------------------------------------------------------------------------------------
def grid_of(M, wgs=0):
    """persistent_grid of dffw_persist.h for the BatchNorm launches."""
    units = -(-M // UNIT_PIX)
    return 8 * min(-(-units // 8), max(1, (wgs if wgs > 0 else DEFAULT_WGS) // 8))


def _pixels(t):
    """(B, C, N, H, W) -> (M, C), pixels in record order."""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def _two_stage(terms0, terms1, M, grid_x, drop_largest=False):
    """The float64 sums of two (M, C) term arrays: per workgroup over the pixels of its units (persistent_range), then over the workgroups in order."""
    units = -(-M // UNIT_PIX)
    per_wg = cg.persistent_units(units, grid_x)
    slots = []
    for us in per_wg:
        idx = torch.cat([torch.arange(u * UNIT_PIX, min(M, (u + 1) * UNIT_PIX)) for u in us]) if us else torch.zeros(0, dtype=torch.long)
        slots.append((terms0[idx].sum(0), terms1[idx].sum(0)))
    if drop_largest:
        slots[max(range(len(per_wg)), key=lambda i: len(per_wg[i]))] = (torch.zeros_like(slots[0][0]), torch.zeros_like(slots[0][1]))
    S0, S1 = torch.zeros_like(slots[0][0]), torch.zeros_like(slots[0][1])
    for a, b in slots:
        S0, S1 = S0 + a, S1 + b
    return S0, S1


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate(case, prec, relu, residual, *, wgs=0, eps=BN_EPS, momentum=MOMENTUM, fault=None):
    """Forward and backward in the kernels' arithmetic: records rounded to ``prec``; float64 sums of x and x^2 (exact terms) per workgroup, added in
    workgroup order; float32 save_mean / save_invstd; float32 channel constant gamma * invstd, y = fma(x - mean, const, beta) (+ res), split into
    the parts of ``prec``; the backward sums of g and g (x - mean) the same way, float32 constants dbeta / M and dgamma invstd / M, grad_x split
    into parts.  ``fault`` plants one of the errors tests/test_bn_train.py names.  Returns a dict keyed like QUANTITIES (NCDHW float32)."""
    full = case["x"].shape
    C = full[1]
    back = lambda t: t.reshape(full[0], full[2], full[3], full[4], C).permute(0, 4, 1, 2, 3).contiguous()
    x = _pixels(rounded(case["x"], prec))
    gy = _pixels(rounded(case["gy"], prec))
    M = x.shape[0]
    grid_x = grid_of(M, wgs)
    xd = x.double()
    S0, S1 = _two_stage(xd, xd * xd, M, grid_x, drop_largest=fault == "missing_partial")
    mean = S0 / M
    var = (S1 / M - mean * mean).clamp_min(0.0)
    if fault == "fp32_var":
        s1, s2 = torch.zeros(C), torch.zeros(C)       # float32 running sums, one pixel after the other, and E[x^2] - mean^2 in float32
        for row in x:
            s1, s2 = s1 + row, s2 + row * row
        var = (s2 / M - (s1 / M) * (s1 / M)).clamp_min(0.0).double()
    vi = var * M / (M - 1) if fault == "unbiased_invstd" else var
    invstd = 1.0 / (vi.sqrt() + eps) if fault == "eps_outside" else 1.0 / torch.sqrt(vi + eps)
    out = dict(mean=mean.float(), invstd=invstd.float())
    out["rm"] = ((1 - momentum) * case["rm0"].double() + momentum * mean).float()
    out["rv"] = ((1 - momentum) * case["rv0"].double() + momentum * (var if fault == "biased_running_var" else var * M / (M - 1))).float()
    mu, istd, gamma, beta = out["mean"], out["invstd"], case["gamma"], case["beta"]
    sc = gamma * istd
    t = x - mu
    z = _fma32(t, sc, beta)
    if residual:
        z = z + _pixels(rounded(case["res"], prec))
    if relu:
        z = torch.where(z < 0, torch.zeros_like(z), z)
    y = rounded(z, prec)
    out["y"] = back(y)
    g = gy
    if relu:
        g = torch.where((gy if fault == "mask_from_gy" else y) > 0, gy, torch.zeros_like(gy))
    T0, T1 = _two_stage(g.double(), g.double() * t.double(), M, grid_x)
    out["dbeta"], out["dgamma"] = T0.float(), (T1 * istd.double()).float()
    k1 = (out["dbeta"].double() / M).float()
    k2 = (out["dgamma"].double() * istd.double() / M).float()
    if fault == "no_dgamma_term":
        k2 = torch.zeros_like(k2)
    out["gx"] = back(rounded(_fma32(-t, k2, g - k1) * sc, prec))
    if residual:
        out["gres"] = back(gy if fault == "grad_res_unmasked" else g)
    return out
