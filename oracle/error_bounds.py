"""ORACLE — test infrastructure, not product code.

Per-element forward-error bounds for the conv and pool kernels of libdffw.so.

A global relative L2 gate (``rel(got, ref) <= 5e-5``) lets one element out of ``n`` be off by about ``5e-5 * sqrt(n)`` times the
output's rms: at 1e5 ... 3e6 elements that is 2 % ... 9 % of a typical value, enough to hide a wrong edge tile, one phase of a
transposed conv or a fragment whose low half went astray.  The helpers below check every element against the standard
forward-error bound of a dot product instead, which is per element and proportional to the sum of the absolute products.

Arithmetic of the op path.  BatchNorm is folded into the weights on the host in fp32,
``w' = s_c * w``, ``s_c = gamma / sqrt(var + eps)``, ``t_c = beta - mean * s_c``; then

* ``bf16x3``: both operands split ``hi = bf16(v)``, ``lo = bf16(v - hi)`` (bf16 keeps 8 significant bits, unit roundoff 2^-8, round to
  nearest even), so one hi + lo pair carries ``|v - hi - lo| <= 2^-8 |v - hi| <= 2^-16 |v|``; products ``hi*hi + hi*lo + lo*hi`` (the
  dropped ``lo*lo`` is ``<= 2^-16 |x w'|``), fp32 accumulation, the result stored as a hi + lo pair again (``<= 2^-16 |y|``).
* ``fp16`` / ``bf16``: one rounding of each operand to the 16-bit format (unit roundoff ``u`` = 2^-11 / 2^-8), one exact product, fp32
  accumulation, one rounding of the stored result: per product ``|err| <= (2u + u^2) |x w'|``, storage ``u |y|``.

Summed over the ``K`` products and the epilogue (shift, residual, ReLU: ReLU is 1-Lipschitz and cannot grow an error), with
``S = conv(|x|, |w|)`` and the per-element scale

    D = |s_c| S + |BN(conv(x, w))| + |t_c| + |res|

every element satisfies ``|got - ref| <= alpha * D`` with ``alpha`` = fp16 2^-10, bf16 2^-7 (``2u``: the worst case of the two operand
roundings, the storage rounding is covered by the ``|BN(conv)|`` and ``|res|`` terms) and bf16x3 2^-16.  For bf16x3 the worst case
of one product is three times that, but it needs both residues ``v - hi`` at half an ulp and ``lo`` rounded the full half ulp: the
residues are spread evenly, their errors are as likely up as down, and over a sum of products the error is about a quarter of
``2^-16 |s_c| S``.  The fp32 accumulation adds at worst ``K * 2^-24 * S`` (2^-11.7 S at K = 27 * 192) and in fact ``~sqrt(K) * 2^-24 * S``,
under 2^-17.8 S at K = 5184.  Emulated on the CPU (tests/test_error_bounds.py) the worst ratio ``err / (alpha D)`` stays under 0.5 (0.46) for all
three formats, K from 24 to 5184, zero-mean, constant, shifted and post-ReLU inputs, unit impulses and wide BN scales (gamma 0 and
negative, var down to 1e-4); on the MI355X every kernel family of tests/test_gpu_ops.py stays under 0.6.  A missed product, a term computed from ``hi`` halves only, or a wrong tap is a local error of order
``|x w'|`` to ``2^-8 |x w'|`` and exceeds the bound by far more than that headroom; at K = 5184 one missed product of average size is
``S / 5184 = 2^-12.3 S``, still 14x over the bf16x3 bound.  (An impulse input is exact in every format, so there only the weight and
the storage roundings act: at most ``2^-16 (|s_c| S + |y|)``, within the bound even in the worst case.)

fp16 subnormals: the fold happens before the cast, so a small ``s_c`` (gamma near zero) makes folded weights subnormal in fp16, where
the rounding error is absolute, at most half the subnormal spacing 2^-24 per weight: ``2^-25 conv(|x|, 1)``.  A subnormal stored
result adds at most 2^-25 as well.  Both terms are added to the fp16 bound only.

Nothing here imports the reference; only torch.
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5

# alpha = 2u of the operand and storage format (derivation above)
ALPHA = {"bf16x3": 2.0 ** -16, "fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
FP16_SUB = 2.0 ** -25   # half the fp16 subnormal spacing


class Ref64:
    """Float64 reference of one conv op: ``ref`` (the op's output), ``pre`` (BN(conv) before residual and ReLU, what the op's
    ``want_pre`` returns), ``D`` (the per-element scale of the bound) and ``sub`` (the fp16 subnormal term, absolute)."""

    def __init__(self, ref, pre, D, sub):
        self.ref, self.pre, self.D, self.sub = ref, pre, D, sub

    def squeeze1(self):
        """The one-output-channel form the op returns for Cout == 1 (B, N, H, W)."""
        return Ref64(self.ref.squeeze(1), self.pre.squeeze(1), self.D.squeeze(1), self.sub.squeeze(1))

    def bound(self, prec):
        b = ALPHA[prec] * self.D
        if prec == "fp16":
            b = b + self.sub
        return b


def _conv64(x, w, stride, pad, dilation, transposed):
    if transposed:
        return F.conv_transpose3d(x, w, None, stride, pad, (0, 1, 1))
    return F.conv3d(x, w, None, stride, pad, dilation)


def fold_bn(bn, cout):
    """(s_c, t_c) in float64 of eval-mode BatchNorm (gamma, beta, mean, var); identity without BN."""
    if bn is None:
        return torch.ones(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
    g, b, m, v = (t.detach().cpu().double().reshape(-1) for t in bn)
    s = g / torch.sqrt(v + BN_EPS)
    return s, b - m * s


def conv_ref64(x, w, *, stride=1, pad=0, dilation=1, transposed=False, bn=None, residual=None, relu=0):
    """The op ``y = [relu](BN(conv(x, w)) [+ res])`` in float64 on the CPU, in the order the op applies it: ``relu=1`` is
    ``relu(BN(conv) + res)``, ``relu=2`` is ``relu(BN(conv)) + res``, ``relu=0`` no ReLU.  Returns a Ref64."""
    x = x.detach().cpu().double()
    w = w.detach().cpu().double()
    cout = w.shape[1] if transposed else w.shape[0]
    acc = _conv64(x, w, stride, pad, dilation, transposed)
    S = _conv64(x.abs(), w.abs(), stride, pad, dilation, transposed)
    ones = torch.ones_like(w[:1] if not transposed else w[:, :1])
    X1 = _conv64(x.abs(), ones, stride, pad, dilation, transposed)
    s, t = fold_bn(bn, cout)
    s5, t5 = s.reshape(1, -1, 1, 1, 1), t.reshape(1, -1, 1, 1, 1)
    pre = acc * s5 + t5
    D = s5.abs() * S + pre.abs() + t5.abs()
    if residual is not None:
        res = residual.detach().cpu().double()
        D = D + res.abs()
        y = (F.relu(pre) + res) if relu == 2 else (pre + res)
        if relu == 1:
            y = F.relu(y)
    else:
        y = F.relu(pre) if relu else pre
    sub = FP16_SUB * (X1 + 1.0)
    return Ref64(y, pre, D, sub.expand_as(D))


def score_ref64(r, cw):
    """Reference and scale of the fused 1x1x1 Cout -> 1 classifier (conv_rollt<.., 2>) applied to the op's final value ``r.ref``:
    the classifier weights are rounded like any weight and each ``y_c`` carries its own bound, so
    ``|err| <= alpha * sum_c |cw_c| (D_c + |y_c|)``.  Returns a Ref64 of shape (B, N, H, W)."""
    cw = cw.detach().cpu().double().reshape(1, -1, 1, 1, 1)
    ref = (r.ref * cw).sum(1)
    D = ((r.D + r.ref.abs()) * cw.abs()).sum(1)
    sub = (r.sub * cw.abs()).sum(1) + FP16_SUB * (r.ref.abs().sum(1) + 1.0)
    return Ref64(ref, ref, D, sub)


def pool_ref64(x, k, mode):
    """Max / average pool (1,k,k) of the stored inputs: max selects one stored value (its storage rounding: ``alpha * |ref|``), avg sums
    k^2 stored values and stores the mean (input roundings ``alpha * mean|x|``, output rounding ``alpha * |ref|``)."""
    x = x.detach().cpu().double()
    if mode == "max":
        ref = F.max_pool3d(x, (1, k, k), (1, k, k))
        D = ref.abs()
    else:
        ref = F.avg_pool3d(x, (1, k, k), (1, k, k))
        D = F.avg_pool3d(x.abs(), (1, k, k), (1, k, k)) + ref.abs()
    return Ref64(ref, ref, D, torch.full_like(D, FP16_SUB))


def _ratio(err, bound):
    """err / bound per element: 0 where both are 0, inf where only the bound is (or err is NaN)."""
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))


def _report(ratio, what):
    flat = int(torch.argmax(ratio.reshape(-1)))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    nbad = int((ratio > 1).sum())
    return "%s: %d of %d elements over the bound; worst at %s (b, c, z, y, x), err/bound %.3g" % (
        what, nbad, ratio.numel(), idx, float(ratio.reshape(-1)[flat]))


def elementwise_ratio(got, r, prec, factor=1.0, alt=None):
    """max(|got - ref| / bound) over all elements, and the ratio tensor; with ``alt`` the pair |got - alt| against factor * bound."""
    got = got.detach().cpu().double()
    other = r.ref if alt is None else alt.detach().cpu().double()
    assert got.shape == other.shape == r.D.shape, (tuple(got.shape), tuple(other.shape), tuple(r.D.shape))
    ratio = _ratio((got - other).abs(), factor * r.bound(prec))
    return float(ratio.max()) if ratio.numel() else 0.0, ratio


def check_elementwise(got, r, prec, what="output"):
    """Assert ``|got - ref| <= alpha_prec * D (+ fp16 subnormal term)`` for every element (exactly 0 where D == 0, NaN fails);
    returns max(err / bound) so tests can log it."""
    worst, ratio = elementwise_ratio(got, r, prec)
    assert worst <= 1.0, _report(ratio, "%s (%s)" % (what, prec))
    return worst


def check_pair(got, alt, r, prec, what="kernel vs kernel"):
    """Two kernels' results of one op: ``|got - alt| <= 2 * bound`` elementwise (each is within one bound of the reference)."""
    worst, ratio = elementwise_ratio(got, r, prec, factor=2.0, alt=alt)
    assert worst <= 1.0, _report(ratio, "%s (%s)" % (what, prec))
    return worst


# ---- input and BatchNorm regimes where kernels go wrong (shared by the CPU self-test and the GPU wide-regime test) ----------
REGIMES = ("impulse", "constant", "post_relu", "offset", "trained_bn")


def _uniform(shape, g):
    return torch.rand(*shape, generator=g) * 2 - 1


def impulse_input(B, C, N, H, W):
    """Zero except unit impulses at the four corners, on tile boundaries (rows / columns 7, 8, 15, 16, 31, 32 where they exist),
    in the first and last slice and in the first and last channel."""
    x = torch.zeros(B, C, N, H, W)
    rows = sorted({0, H - 1} | {r for r in (7, 8, 15, 16, 31, 32) if r < H})
    cols = sorted({0, W - 1} | {c for c in (7, 8, 15, 16, 31, 32) if c < W})
    for b in range(B):
        for i, (z, c) in enumerate(((0, 0), (N - 1, C - 1), (N // 2, C // 2))):
            for y in (0, H - 1):                       # the four corners
                for xx in (0, W - 1):
                    x[b, c, z, y, xx] = 1.0
            for j, r in enumerate(rows):               # tile boundaries, spread over rows and columns so footprints rarely overlap
                x[b, c, z, r, cols[(j + i + b) % len(cols)]] = 1.0
            for j, cc in enumerate(cols):
                x[b, (c + j) % C, z, rows[(j + 2 * i + b) % len(rows)], cc] = 1.0
    return x


def regime_input(kind, shape, seed):
    """The input volume (B, C, N, H, W) of a regime (see REGIMES)."""
    B, C, N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if kind == "impulse":
        return impulse_input(B, C, N, H, W)
    if kind == "constant":       # one constant per (sample, channel, slice) plane: only the border differs from the interior
        return _uniform((B, C, N, 1, 1), g).expand(B, C, N, H, W).contiguous()
    if kind == "post_relu":      # half of the input exact zeros
        return F.relu(_uniform(shape, g))
    if kind == "offset":         # large common offset: heavy cancellation against the BN mean
        return 3 + 0.5 * _uniform(shape, g)
    return _uniform(shape, g)    # "trained_bn" and the plain case: zero-mean uniform


def bn_regime(kind, c, seed, conv_mean=0.0):
    """(gamma, beta, mean, var) of a regime.  ``trained_bn`` / ``offset``: gamma with zeros, negatives and up to +-2, var log-uniform in
    [1e-4, 1e2], mean and beta in +-3 (``offset`` centres mean on ``conv_mean`` so the BN cancels the offset); ``impulse``: the same
    scales with zero shift (t_c = 0); otherwise the mild synthetic regime (gamma, var in [0.5, 1.5])."""
    g = torch.Generator().manual_seed(seed)
    if kind in ("trained_bn", "offset", "impulse"):
        gamma = (torch.rand(c, generator=g) * 4 - 2)
        gamma[0] = 0.0
        if c > 2:
            gamma[1] = -2.0
            gamma[2] = 2.0
        var = 10.0 ** (torch.rand(c, generator=g) * 6 - 4)
        mean = (torch.rand(c, generator=g) * 6 - 3) + conv_mean
        beta = torch.rand(c, generator=g) * 6 - 3
        if kind == "impulse":
            mean = torch.zeros(c)
            beta = torch.zeros(c)
        return gamma, beta, mean, var
    return (0.5 + torch.rand(c, generator=g), torch.rand(c, generator=g) - 0.5,
            torch.rand(c, generator=g) - 0.5, 0.5 + torch.rand(c, generator=g))
