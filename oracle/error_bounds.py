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

Fused blocks (srd_ref64, efd_ref64).  The SRD and EFD kernels compute several convs of a block in one launch, keep intermediates in
LDS (in fp32 or in the storage format) and only the block's output is observable, so their bound composes the per-conv ones.  To
first order an error ``e`` in a conv's input adds ``|s_c| conv(|e|, |w|)`` to its output (the conv is linear, its folded weights are
``s_c w``), and ReLU, the residual add and max are 1-Lipschitz, so they pass an error on without growing it.  With every operand
error bounded by ``alpha`` times its D, the block's D is the sum of each conv's own D (the roundings inside it) and the previous D
carried through ``|s_c| |w|``:

    SRD  t = relu(BN0(conv(x, w0)))                     D_t    = D(conv0)
         feat = relu(BN2(conv(t, w2)) + x)              D_feat = D(conv2) + |s2| conv(D_t, |w2|)
         a = relu(conv(feat, w3))      (3x1x1)          D_a    = D(conv3) + conv(D_feat, |w3|)
         y = relu(conv(a, w1)) + feat  (1x1x1)          D_y    = D(conv1) + conv(D_a, |w1|) + D_feat
         pooled = max_pool(1,2,2)(y)                    D_p    = max_pool(D_y) + |pooled|
    EFD  a = BN_s(conv_s(1,2,2)(x, ws))                 D_a    = D(conv_s)
         y = relu(BN_p(conv(max_pool(x), wp)) + a)      D_y    = D(conv_p) + D_a

where each ``D(conv)`` is the single-conv scale above evaluated on the float64 reference of its input (its ``|res|`` term holds the
stored residual's rounding).  Max selects one stored value, so the pooled input of the EFD carries only x's own rounding, which the
operand term of ``D(conv_p)`` already holds, and ``|max(a) - max(b)| <= max|a - b|`` gives ``max_pool(D_y)`` for the pooled copy (``+ |pooled|``
for a copy that is rounded once more).  The bound stays ``alpha * D`` with the same alpha: it is linear in the per-conv bounds,
second-order terms (an error times a rounding) are below 2^-32 for split-bf16 and covered by the margin of the worst-case alpha for
the 16-bit formats.  The fp16 subnormal term composes the same way.

The carried terms grow by the L1 norm of each filter (``|s_c| sum|w|`` ~ 3 ... 10 at He scale), so through the SRD block's four convs the
scale reaches some 600 |y|, and a lost lo half of ``feat`` (2^-9 |feat|) would stay under it.  ``srd_ref64(..., prec)`` therefore resolves
the ReLUs for one arithmetic: where a ReLU's reference input lies below minus that arithmetic's bound of it, the kernel's input is
negative as well, both outputs are exactly 0 and no error passes; elsewhere the full D passes.  That bound holds for ``prec`` only
(``Ref64.prec``) and is no longer linear in alpha; without ``prec`` every ReLU passes its input's error on.  Emulated through both blocks (tests/test_error_bounds.py) the worst
ratio stays under 0.5 in all three arithmetics, slice counts 1, 2, 3 and every regime below (0.44 EFD, 0.35 SRD); a missed residual in one column, a slice
padding read from the neighbour, ``feat`` kept as hi halves in one strip, a wrong pixel of the pooled window or a pooled branch one
row off at a tile seam each exceed the bound at least 4x.

Alignment feature blocks (of_ref64).  resnet_block_2d_OF (End_to_End.py:135-145) is two 1x3x3 convbn and a bias-free 1x1x1 shortcut,
both first convs with the block's (1,s,s) stride:

         t = relu(BN0(conv_s(x, w0)))                   D_t = D(conv0)
         f = conv1x1_s(x, wf)                           D_f = conv(|x|, |wf|) + |f|
         y = relu(BN2(conv(t, w2)) + f)                 D_y = D(conv2) + |s2| conv(D_t, |w2|) + D_f

A stride-1 block folds the shortcut into conv.2's contraction over [t | x] (its products are then rounded like conv.2's own; the
``conv(|x|, |wf|)`` term covers them and ``|f|`` a stored copy), a stride-2 block adds a stored ``f`` as a residual: one D serves both.
``of_ref64(..., prec)`` resolves both ReLUs as srd_ref64 does.  The 3 -> 8 first block reads the fp32 stack, rounded once to the
operand format (the ``|s_c| S`` term).  Emulated through the block (tests/test_error_bounds.py) the worst ratio stays under 0.5 in all
three arithmetics, every regime and slice counts 1, 2, 3 and 10; the stride-2 shortcut reading the odd pixel, a missed shortcut in one
column and ``t`` kept as hi halves in one strip each exceed the bound at least 4x.

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

    prec = None   # the one arithmetic D holds for (a block's bound with its ReLUs resolved, srd_ref64), or None: every one

    def __init__(self, ref, pre, D, sub):
        self.ref, self.pre, self.D, self.sub = ref, pre, D, sub

    def squeeze1(self):
        """The one-output-channel form the op returns for Cout == 1 (B, N, H, W)."""
        return Ref64(self.ref.squeeze(1), self.pre.squeeze(1), self.D.squeeze(1), self.sub.squeeze(1))

    def bound(self, prec):
        assert self.prec in (None, prec), "this bound was composed for %s, not %s" % (self.prec, prec)
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


# ---- the fused front-end blocks: composed bounds (derivation in the module docstring) ------------------------------------------
def _carry(D, w, scale=None, pad=0):
    """``|s_c| conv(D, |w|)``: an input error bounded by D, carried through a conv (its folded weights are s_c * w)."""
    out = F.conv3d(D, w.detach().cpu().double().abs(), None, 1, pad)
    return out if scale is None else out * scale.abs().reshape(1, -1, 1, 1, 1)


def maxpool_ref64(r):
    """max_pool(1,2,2) of a block's output (its Ref64): the maximum moves by at most the largest error in the window, and a copy
    rounded once more adds ``|pooled|``."""
    ref = F.max_pool3d(r.ref, (1, 2, 2), (1, 2, 2))
    return Ref64(ref, ref, F.max_pool3d(r.D, (1, 2, 2), (1, 2, 2)) + ref.abs(), F.max_pool3d(r.sub, (1, 2, 2), (1, 2, 2)) + FP16_SUB)


def _relu_passes(pre, D, sub, prec):
    """1 where a ReLU can pass its input's error on, 0 where it cannot: with ``prec`` given, an input whose reference lies below
    minus that arithmetic's bound is negative in the kernel as well, so both results are exactly 0 there."""
    if prec is None:
        return torch.ones_like(pre)
    return (pre > -Ref64(pre, pre, D, sub).bound(prec)).to(pre.dtype)


def srd_ref64(x, w0, bn0, w2, bn2, w3, w1, prec=None):
    """The SRD block (DEN.py:317-330) in float64: (Ref64 of its output, Ref64 of the max-pooled copy).  ``pre`` of the output is the
    attention's 1x1x1 conv before its ReLU.  With ``prec`` the four ReLUs pass no error where they are off for certain in that
    arithmetic (the bound is then that arithmetic's only); without it every ReLU passes its input's error on."""
    x = x.detach().cpu().double()
    C = x.shape[1]
    p2, pa = (0, 1, 1), (1, 0, 0)
    rt = conv_ref64(x, w0, pad=p2, bn=bn0, relu=1)
    on = _relu_passes(rt.pre, rt.D, rt.sub, prec)
    D_t, sub_t = rt.D * on, rt.sub * on
    s2, _ = fold_bn(bn2, C)
    rf = conv_ref64(rt.ref, w2, pad=p2, bn=bn2, residual=x, relu=1)
    D_feat = rf.D + _carry(D_t, w2, s2, p2)
    sub_feat = rf.sub + _carry(sub_t, w2, s2, p2)
    on = _relu_passes(rf.pre + x, D_feat, sub_feat, prec)
    D_feat, sub_feat = D_feat * on, sub_feat * on
    ra = conv_ref64(rf.ref, w3, pad=pa, relu=1)
    D_a = ra.D + _carry(D_feat, w3, pad=pa)
    sub_a = ra.sub + _carry(sub_feat, w3, pad=pa)
    on = _relu_passes(ra.pre, D_a, sub_a, prec)
    D_a, sub_a = D_a * on, sub_a * on
    ro = conv_ref64(ra.ref, w1, residual=rf.ref, relu=2)
    D_1, sub_1 = ro.D - rf.ref.abs() + _carry(D_a, w1), ro.sub + _carry(sub_a, w1)   # the 1x1x1 conv before its ReLU ...
    on = _relu_passes(ro.pre, D_1, sub_1, prec)
    # ... then + feat (its storage rounding: |feat|), and the sum stored once more (|y| <= |relu(pre)| + |feat|; a subnormal: FP16_SUB)
    out = Ref64(ro.ref, ro.pre, D_1 * on + rf.ref.abs() + D_feat, sub_1 * on + sub_feat + FP16_SUB)
    out.prec = prec
    pooled = maxpool_ref64(out)
    pooled.prec = prec
    return out, pooled


def efd_ref64(x, ws, bns, wp, bnp):
    """The EFD block (DEN.py:306-315) in float64: relu(BN_s(conv s(1,2,2)(x)) + BN_p(conv(max_pool(x)))), a Ref64 whose ``pre`` is
    the pooled branch's BN(conv)."""
    x = x.detach().cpu().double()
    ra = conv_ref64(x, ws, stride=(1, 2, 2), pad=1, bn=bns)
    rb = conv_ref64(F.max_pool3d(x, (1, 2, 2), (1, 2, 2)), wp, pad=1, bn=bnp, residual=ra.ref, relu=1)
    return Ref64(rb.ref, rb.pre, rb.D + ra.D, rb.sub + ra.sub)


def _block_weight(shape, K, g, bn):
    """Uniform weights of rms ~ sqrt(2 / K) * 1.7 / sqrt(3); with a BatchNorm whose scale |s_c| exceeds 4 (var down to 1e-4) the
    weights are divided by max|s_c| / 4, so that two such convs in a row stay well inside the fp16 range while the per-channel
    scales keep their spread (folded weights of the small-scale channels then land in the fp16 subnormals)."""
    w = (torch.rand(*shape, generator=g) * 2 - 1) * (2.0 / K) ** 0.5 * 1.7
    if bn is not None:
        s, _ = fold_bn(bn, shape[0])
        w = w / max(1.0, float(s.abs().max()) / 4)
    return w


def srd_params(kind, C, seed):
    """Weights of one SRD block in a regime (see REGIMES): (w0, bn0, w2, bn2, w3, w1); both BatchNorms from bn_regime."""
    g = torch.Generator().manual_seed(seed)
    bn0, bn2 = bn_regime(kind, C, seed + 1), bn_regime(kind, C, seed + 2)
    w0 = _block_weight((C, C, 1, 3, 3), 9 * C, g, bn0)
    w2 = _block_weight((C, C, 1, 3, 3), 9 * C, g, bn2)
    w3 = _block_weight((C, C, 3, 1, 1), 3 * C, g, None)
    w1 = _block_weight((C, C, 1, 1, 1), C, g, None)
    if kind == "offset":    # the first BN centred on what the input's common offset 3 gives (heavy cancellation, as in make_case)
        bn0 = bn_regime(kind, C, seed + 1, conv_mean=3.0 * float(w0.double().sum() / C))
    return w0, bn0, w2, bn2, w3, w1


def efd_params(kind, cin, seed):
    """Weights of one EFD block cin -> 2 cin in a regime: (ws, bns, wp, bnp)."""
    g = torch.Generator().manual_seed(seed)
    cout = 2 * cin
    bns, bnp = bn_regime(kind, cout, seed + 1), bn_regime(kind, cout, seed + 2)
    ws = _block_weight((cout, cin, 3, 3, 3), 27 * cin, g, bns)
    wp = _block_weight((cout, cin, 3, 3, 3), 27 * cin, g, bnp)
    if kind == "offset":    # both branches centred: their sum then cancels twice
        bns = bn_regime(kind, cout, seed + 1, conv_mean=3.0 * float(ws.double().sum() / cout))
        bnp = bn_regime(kind, cout, seed + 2, conv_mean=3.0 * float(wp.double().sum() / cout))
    return ws, bns, wp, bnp


# ---- the alignment network's feature blocks ----------------------------------------------------------------------------------------
def of_ref64(x, w0, bn0, w2, bn2, wf, stride, prec=None):
    """resnet_block_2d_OF (End_to_End.py:135-145) in float64: relu(conv1x1_s(x, wf) + BN2(conv(relu(BN0(conv_s(x, w0))), w2))), a Ref64
    whose ``pre`` is BN2(conv) + shortcut before the last ReLU.  With ``prec`` both ReLUs pass no error where they are off for certain
    in that arithmetic (see srd_ref64)."""
    x = x.detach().cpu().double()
    Cout = w0.shape[0]
    s, p2 = (1, stride, stride), (0, 1, 1)
    rt = conv_ref64(x, w0, stride=s, pad=p2, bn=bn0, relu=1)
    on = _relu_passes(rt.pre, rt.D, rt.sub, prec)
    D_t, sub_t = rt.D * on, rt.sub * on
    rf = conv_ref64(x, wf, stride=s)
    ry = conv_ref64(rt.ref, w2, pad=p2, bn=bn2, residual=rf.ref, relu=1)
    s2, _ = fold_bn(bn2, Cout)
    pre = ry.pre + rf.ref
    D = ry.D + _carry(D_t, w2, s2, p2) + rf.D - rf.ref.abs()   # (ry.D holds |f| already: its residual term)
    sub = ry.sub + _carry(sub_t, w2, s2, p2) + rf.sub
    on = _relu_passes(pre, D, sub, prec)
    out = Ref64(ry.ref, pre, D * on, sub * on)
    out.prec = prec
    return out


OF_BLOCKS = ((3, 8, 1), (8, 8, 1), (8, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1))   # (Cin, Cout, stride): OF_feature.0 ... OF_feature2.1


def of_params(kind, cin, cout, seed):
    """Weights of one alignment feature block in a regime (see REGIMES): (w0, bn0, w2, bn2, wf)."""
    g = torch.Generator().manual_seed(seed)
    bn0, bn2 = bn_regime(kind, cout, seed + 1), bn_regime(kind, cout, seed + 2)
    w0 = _block_weight((cout, cin, 1, 3, 3), 9 * cin, g, bn0)
    w2 = _block_weight((cout, cout, 1, 3, 3), 9 * cout, g, bn2)
    wf = _block_weight((cout, cin, 1, 1, 1), cin, g, None)
    if kind == "offset":    # the first BN centred on what the input's common offset 3 gives
        bn0 = bn_regime(kind, cout, seed + 1, conv_mean=3.0 * float(w0.double().sum() / cout))
    return w0, bn0, w2, bn2, wf
