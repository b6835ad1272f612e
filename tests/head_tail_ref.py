"""Reference, per-element bound and CPU emulation of the back half of an alpha head (``head_tail()`` in csrc/dffw_align.cpp, tested through
``dffw_op_head_tail``): from the first conv's output y0 through convs .2 and .4 (1x3x3, BatchNorm, ReLU), the biased conv .6 (C -> 3) and the
plane mean to ``raw = m`` and ``alpha += (0.001 m if c == 0 else m)`` (End_to_End.py:37-69, 86-103).  A plain module like regress_ref.py.

Reference (``reference``).  Float64 on the record-rounded x: y1 = relu(BN(conv(x, w2))), y2 = relu(BN(conv(y1, w4))),
m[b,c,n] = bias6[c] + mean_{y,x} conv(y2, w6)[b,c,n]; with ``start = 2`` x is y2.

Forms.  "tiles": of_roll_kernel<P, false, true> + head_tail_tiles_reduce/finish (y2 stays fp32); "rows": conv .4 as a row-sums conv +
head_tail_rows_reduce/finish (y2 stays fp32); "planes": stored y2, plane_sums_kernel + head_tail_finish_kernel; "mean": stored y2, conv .6
into three fp32 planes + alpha_mean_kernel.

Bound E, per output number, arithmetic and form; u = 2^-24, a = eb.ALPHA[prec]:

* Carried term  (1/HW) sum_{y,x} conv(a D2 [+ sub2], |w6|).  D2 is the composed scale of y2: D1 = D(conv .2) on the exact records of x (ReLU
  resolved with eb._relu_passes), D2 = D(conv .4) + |s4| conv(D1, |w4|) (eb._carry), ReLU resolved again; an unresolved ReLU passes the whole
  scale, no output is left out.  D(conv .4) holds |BN(conv)|, the storage rounding of y2: the tiles and rows forms keep y2 in fp32, so the
  stored-y2 scale is an upper bound for them.  With start = 2 the term is zero: x is y2 exactly, as records.
* Summation term.  The kernels form, per channel, the plane total T, the two border rows R, the two border columns C (and read the corners),
  in fp32 up to a point and in double from there; a tap's window sum is T - R - C + corner.  T, R and C are rounded separately in the planes
  form, so the term is not k u (1/HW) sum conv(|y2|, |w6|) (which vanishes where the window is empty, e.g. tap row 0 at H = 1) but the same
  with the subtracted lines ADDED:  u (1/HW) sum_{c,ci,dy,dx} |w6| (kT |T| + kR |R_dy| + kC |C_dx|), |.| the sums of |y2|.  k is the longest
  chain of fp32 additions before the doubles:
    planes  kT = ceil(ppc PR / 256) (a thread's fp32 partial of its piece position over a chunk of ppc pixels, PR = parts C / 8 pieces a
            pixel), kR / kC = ceil(len / (4 nph)) + 5 (four accumulators over a thread's phase of the line, nph = 256 / C, the remainder
            loop into the first, two adds to combine); the corners are exact.
    tiles   kT = kR = 5 (the DPP tree over a row of 16 pixels is 4 additions deep, + 1 for the wave's second row; a border row alone: 4),
            kC = 1 (the wave's two border pixels).
    rows    kT = kR = 4 (the DPP tree over a row segment of 16 pixels), kC = 0 (single pixels).
    mean    the conv's fp32 planes, then alpha_mean_kernel: k = ceil(HW / 1024) + 3 (a thread's accumulator, the remainder loop into the
            first) + 2 (combining the four) + 6 (shuffle tree) + 2 (part[]) + 1 (the division), on (1/HW) sum |conv(y2, w6) + bias| <= A + |bias|.
  Every form adds 2^-40 of the same sums for the double additions (chains under 2^12 at 2^-53 each).
* Weights of conv .6: exact fp32 (whead) in the three plane-sum forms; in the mean form the conv runs in the arithmetic:
  a (1/HW) sum conv(|y2|, |w6|) (+ eb.FP16_SUB (1/HW) sum conv(|y2|, 1) for fp16 weights in the subnormals) and u |bias| for the fp32 shift.
* Last steps: one fp32 rounding of m (u |m|); alpha: the step 0.001f m in fp32 (|0.001f - 0.001| |m| + u 0.001 |m|, c = 0 only), one fp32 add
  (u |alpha_out|).

E_raw = CAL_FACTOR (carried + summation + weights + u |m|);  E_alpha = damp E_raw + CAL_FACTOR (step terms + u |alpha_out|).

Calibration.  CAL_FACTOR is set from the clean emulation's worst err / E (with CAL_FACTOR = 1) over the cases at the end of this module
(every case of the GPU test, in every form and arithmetic): CAL_WORST, re-measured by tests/test_head_tail.py::test_calibration, times 4,
rounded up to a power of two -- never from a GPU result.  The last steps are single roundings, so err / E comes close to 1 where they are
all there is (start = 2, a handful of exact values); the clean emulation then sits at or under E / 4.

Emulation (``emulate``).  float32 / split records on the CPU.  Convs .2, .4 (and .6 in the mean form): operands split to the format, fp32
accumulation (torch's order, not the MFMA's: stated equivalent), the shift in fp32, ReLU, the result stored (or kept fp32).  planes: a
thread's chunk partial and the line accumulators in the kernel's order; tiles / rows: the balanced 16-pixel tree, the two-row add; mean: the
four accumulators, tree and part[] in the kernel's order.  Everything the kernels do in double is done in double here, in torch's order
(differences at 2^-53).  FAULTS are arguments of the emulation."""
import math

import torch
import torch.nn.functional as F

from oracle import error_bounds as eb

U = 2.0 ** -24
DBL = 2.0 ** -40
DAMP32 = float(torch.tensor(0.001, dtype=torch.float32))   # 0.001f
CAL_WORST = 0.98      # worst err / E (CAL_FACTOR = 1) of the clean emulation over the cases below; test_calibration re-measures it
CAL_FACTOR = 4.0      # 4 * CAL_WORST = 3.9, rounded up to a power of two
PAD = (0, 1, 1)
FORMS = ("tiles", "rows", "planes", "mean")
HEADS = {16: "conv3", 32: "conv2", 64: "conv1"}
FAULTS = ("corner_missing", "corners_swapped", "row_swapped", "col_swapped", "remainder_dropped", "lo_dropped", "interior_as_left",
          "divisor", "damp_c1", "raw_damped", "alpha_overwritten", "idx_order")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def head_params(kind, C, seed):
    """(w2, bn2, w4, bn4, w6, bias6) of one head in a regime of eb.REGIMES, eb-style."""
    g = torch.Generator().manual_seed(seed)
    bn2, bn4 = eb.bn_regime(kind, C, seed + 1), eb.bn_regime(kind, C, seed + 2)
    w2 = eb._block_weight((C, C, 1, 3, 3), 9 * C, g, bn2)
    w4 = eb._block_weight((C, C, 1, 3, 3), 9 * C, g, bn4)
    w6 = eb._block_weight((3, C, 1, 3, 3), 9 * C, g, None)
    bias6 = torch.rand(3, generator=g) - 0.5
    if kind == "offset":
        bn2 = eb.bn_regime(kind, C, seed + 1, conv_mean=3.0 * float(w2.double().sum() / C))
    return w2, bn2, w4, bn4, w6, bias6


def centre_params(C, seed):
    """Centre-tap w2, w4 with a positive BatchNorm scale and no shift: y2 is a positive multiple of y0 (powers of two: exact in every format)."""
    w = torch.zeros(C, C, 1, 3, 3)
    for c in range(C):
        w[c, c, 0, 1, 1] = 1.0
    var = torch.full((C,), 1.0 - eb.BN_EPS)
    bn = lambda s: (torch.full((C,), s), torch.zeros(C), torch.zeros(C), var)
    g = torch.Generator().manual_seed(seed)
    return w, bn(2.0), w.clone(), bn(0.5), torch.rand(3, C, 1, 3, 3, generator=g) * 2 - 1, torch.rand(3, generator=g) - 0.5


def places(H, W):
    """The four corners, a pixel of each border line, an interior pixel (those that exist, without repeats)."""
    p = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)]
    return list(dict.fromkeys(p))


def placed_input(B, C, N, H, W, value=1.0):
    """Zero except one ``value`` per plane (b, n), every plane at a different place (cycling) and channel."""
    x = torch.zeros(B, C, N, H, W)
    pl = places(H, W)
    for b in range(B):
        for n in range(N):
            k = b * N + n
            y, xx = pl[k % len(pl)]
            x[b, (5 * k + 3) % C, n, y, xx] = value
    return x


def smooth_input(B, C, N, H, W):
    """A smooth positive feature map (what the whole-network test feeds the heads): low-frequency waves, a different phase per channel and slice."""
    yy = torch.arange(H, dtype=torch.float64).reshape(1, 1, 1, H, 1) / H
    xx = torch.arange(W, dtype=torch.float64).reshape(1, 1, 1, 1, W) / W
    c = torch.arange(C, dtype=torch.float64).reshape(1, C, 1, 1, 1)
    n = torch.arange(N, dtype=torch.float64).reshape(1, 1, N, 1, 1)
    b = torch.arange(B, dtype=torch.float64).reshape(B, 1, 1, 1, 1)
    v = 0.6 + 0.4 * torch.sin(2 * math.pi * (yy * (1 + c % 3) + 0.37 * c + 0.11 * n + 0.23 * b)) * torch.cos(2 * math.pi * (xx * (1 + c % 2) + 0.19 * c))
    return v.float()


def alpha_input(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, 3, N, generator=g) * 2 - 1) * 0.7
    return torch.where(a.abs() < 0.05, torch.full_like(a, 0.3), a)


def records(x, prec):
    """x as the activation records hold it (float32: hi + lo is exact in fp32 for split-bf16)."""
    hi, lo = _split(x.float(), prec)
    return hi + lo


# ---- reference and bound -----------------------------------------------------------------------------------------------------------------
def _plane_mean(t):
    return t.mean(dim=(3, 4))


def _line_sums(a):
    """|y2| (B,C,N,H,W) float64 -> T, R[dy], C[dx] per (B,C,N): the lines a tap row / column subtracts (zero for the centre)."""
    T = a.sum(dim=(3, 4))
    z = torch.zeros_like(T)
    R = [a[:, :, :, -1, :].sum(-1), z, a[:, :, :, 0, :].sum(-1)]
    Cc = [a[:, :, :, :, -1].sum(-1), z, a[:, :, :, :, 0].sum(-1)]
    return T, R, Cc


def chunking(B, N, hw):
    """(chunks, pixels per chunk) of launch_head_tail."""
    n0 = max(1, -(-2560 // (B * N)))
    if n0 * 256 > hw:
        n0 = (hw + 255) // 256
    ppc = -(-hw // n0)
    return -(-hw // ppc), ppc


def sum_chains(form, prec, B, C, N, H, W):
    """(kT, kR, kC) of a form (module docstring); the mean form's single k is returned as kT."""
    if form == "tiles":
        return 5, 5, 1
    if form == "rows":
        return 4, 4, 0
    if form == "planes":
        PR = (2 if prec == "bf16x3" else 1) * C // 8
        _, ppc = chunking(B, N, H * W)
        nph = 256 // C
        return -(-ppc * PR // 256), -(-W // (4 * nph)) + 5, -(-H // (4 * nph)) + 5
    return -(-H * W // 1024) + 14, 0, 0


class HeadRef:
    """raw / alpha: float64 (B,3,N) references; E(form) -> (E_raw, E_alpha), the bounds of one form; shares: per ReLU, the share of its inputs
    that lie within the bound of zero (the kernel's ReLU may differ from the reference's there: the whole scale passes)."""

    def E(self, form):
        return self.bounds[form]


def reference(x, w2, bn2, w4, bn4, w6, bias6, alpha_in, prec, start, forms=FORMS, factor=CAL_FACTOR):
    forms = (forms,) if isinstance(forms, str) else tuple(forms)
    xr = records(x, prec).double()
    B, C, N, H, W = xr.shape
    a = eb.ALPHA[prec]
    out = HeadRef()
    out.shares = []
    if start == 0:
        r1 = eb.conv_ref64(xr, w2, pad=PAD, bn=bn2, relu=1)
        on = eb._relu_passes(r1.pre, r1.D, r1.sub, prec)
        out.shares.append(float(((r1.pre.abs() <= eb.Ref64(r1.pre, r1.pre, r1.D, r1.sub).bound(prec)) & (r1.D > 0)).double().mean()))
        D1, sub1 = r1.D * on, r1.sub * on
        s4, _ = eb.fold_bn(bn4, C)
        r2 = eb.conv_ref64(r1.ref, w4, pad=PAD, bn=bn4, relu=1)
        D2, sub2 = r2.D + eb._carry(D1, w4, s4, PAD), r2.sub + eb._carry(sub1, w4, s4, PAD)
        on = eb._relu_passes(r2.pre, D2, sub2, prec)
        out.shares.append(float(((r2.pre.abs() <= eb.Ref64(r2.pre, r2.pre, D2, sub2).bound(prec)) & (D2 > 0)).double().mean()))
        y2 = r2.ref
        e2 = a * D2 * on + (sub2 * on if prec == "fp16" else 0.0)
    else:
        assert start == 2 and set(forms) <= {"planes", "mean"}, (start, forms)
        y2, e2 = xr, torch.zeros_like(xr)
    w6d, b6 = w6.double(), bias6.double().reshape(1, 3, 1)
    out.y2 = y2
    m = b6 + _plane_mean(F.conv3d(y2, w6d, None, 1, PAD))
    carried = _plane_mean(F.conv3d(e2, w6d.abs(), None, 1, PAD))
    y2a, hw = y2.abs(), H * W
    A = _plane_mean(F.conv3d(y2a, w6d.abs(), None, 1, PAD))
    T, R, Cc = _line_sums(y2a)
    wa = w6d.abs()[:, :, 0]                                        # (3, C, 3, 3)
    lines = lambda kt, kr, kc: sum(torch.einsum("oc,bcn->bon", wa[:, :, dy, dx], kt * T + kr * R[dy] + kc * Cc[dx]) for dy in range(3) for dx in range(3)) / hw
    damp = torch.tensor([0.001, 1.0, 1.0], dtype=torch.float64).reshape(1, 3, 1)
    out.raw = m
    out.alpha = alpha_in.double() + damp * m
    step = (abs(DAMP32 - 0.001) + U * 0.001) * m.abs() * (damp < 1)
    out.bounds, out.terms = {}, {}
    for form in forms:
        kT, kR, kC = sum_chains(form, prec, B, C, N, H, W)
        if form == "mean":
            summ = kT * U * (A + b6.abs()) + DBL * A
            wts = a * A + U * b6.abs()
            if prec == "fp16":
                wts = wts + eb.FP16_SUB * _plane_mean(F.conv3d(y2a, torch.ones_like(w6d), None, 1, PAD))
        else:
            summ = U * lines(kT, kR, kC) + DBL * lines(1, 1, 1)
            wts = torch.zeros_like(A)
        out.terms[form] = {"carried": carried, "summation": summ, "weights": wts}
        E_raw = factor * (carried + summ + wts + U * m.abs())
        out.bounds[form] = (E_raw, damp * E_raw + factor * (step + U * out.alpha.abs()))
    return out


def literal(x, w2, bn2, w4, bn4, w6, bias6, alpha_in, prec, start):
    """The same numbers from a literal float64 composition: F.conv3d, eval-mode batch norm, relu, mean."""
    v = records(x, prec).double()
    if start == 0:
        for w, bn in ((w2, bn2), (w4, bn4)):
            g, b, mu, var = (t.double() for t in bn)
            v = F.relu(F.batch_norm(F.conv3d(v, w.double(), None, 1, PAD), mu, var, g, b, False, 0.0, eb.BN_EPS))
    m = F.conv3d(v, w6.double(), bias6.double(), 1, PAD).mean(dim=(3, 4))
    al = alpha_in.double().clone()
    al[:, 0] += 0.001 * m[:, 0]
    al[:, 1:] += m[:, 1:]
    return m, al


def ratio(got, ref, E):
    """err / E per number: 0 where both are 0, inf where only E is (or got is not finite)."""
    err = (got.detach().cpu().double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))


def worst(got_raw, got_alpha, r, form):
    """The largest err / E over the 2 * 3 * B * N numbers of a result."""
    E_raw, E_alpha = r.E(form)
    return max(float(ratio(got_raw, r.raw, E_raw).max()), float(ratio(got_alpha, r.alpha, E_alpha).max()))


# ---- emulation ----------------------------------------------------------------------------------------------------------------------------
def _split(v, prec):
    if prec == "fp16":
        hi = v.half().float()
        return hi, torch.zeros_like(hi)
    hi = v.bfloat16().float()
    return hi, ((v - hi).bfloat16().float() if prec == "bf16x3" else torch.zeros_like(hi))


def _conv_emu(x, w, bn, shift, prec, relu, store):
    """One 1x3x3 conv in the arithmetic: BN folded in fp32, operands split, fp32 accumulation, fp32 shift, ReLU, stored or fp32."""
    s, t = eb.fold_bn(bn, w.shape[0])
    ws = (w.double() * s.reshape(-1, 1, 1, 1, 1)).float()
    t = t.float() if shift is None else shift.float()
    xh, xl = _split(x, prec)
    wh, wl = _split(ws, prec)
    acc = F.conv3d(xh, wh, None, 1, PAD)
    if prec == "bf16x3":
        acc = acc + (F.conv3d(xh, wl, None, 1, PAD) + F.conv3d(xl, wh, None, 1, PAD))
    y = acc + t.reshape(1, -1, 1, 1, 1)
    if relu:
        y = F.relu(y)
    return records(y, prec) if store else y


def emulate_y2(x, w2, bn2, w4, bn4, prec, store):
    """y2 from y0 in the arithmetic (float32): y1 is always stored (LDS or memory, in the format), y2 stored or kept fp32."""
    y1 = _conv_emu(records(x, prec), w2, bn2, None, prec, True, True)
    return _conv_emu(y1, w4, bn4, None, prec, True, store)


def _seq32(v, dim):
    """Sequential float32 sum along ``dim`` (a thread's accumulator)."""
    acc = torch.zeros_like(v.select(dim, 0))
    for j in range(v.shape[dim]):
        acc = acc + v.select(dim, j)
    return acc


def _tree16(v):
    """The balanced float32 tree over the last dimension of 16 (the DPP row sum)."""
    for _ in range(4):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _acc4(v, nph):
    """plane_sums_kernel's border line / alpha_mean_kernel's accumulators: v (..., len) float32, thread ph takes ph, ph + nph, ...: four
    accumulators in turn while four more elements remain, the rest into the first; (t0 + t1) + (t2 + t3).  Returns (..., nph)."""
    L = v.shape[-1]
    J = -(-L // nph)
    v = F.pad(v, (0, J * nph - L)).reshape(*v.shape[:-1], J, nph)            # [j][ph]
    ph = torch.arange(nph)
    cnt = (L - ph + nph - 1) // nph                                          # elements thread ph owns
    G = cnt // 4                                                             # full rounds: while p + 3 nph < len
    t = [torch.zeros_like(v[..., 0, :]) for _ in range(4)]
    for j in range(J):
        in_round = j < 4 * G
        k = j % 4
        for q in range(4):
            use = (in_round & (k == q)) | (~in_round & (q == 0))
            t[q] = t[q] + v[..., j, :] * use.to(v.dtype)
    return (t[0] + t[1]) + (t[2] + t[3])


def _sums_planes(y2, prec, fault):
    """sums[9] (each (B,C,N) float64) as plane_sums_kernel + head_tail_finish_kernel form them from stored y2 (float32, exact records)."""
    B, C, N, H, W = y2.shape
    hw = H * W
    parts = _split(y2, prec) if prec == "bf16x3" else (y2,)
    if fault == "lo_dropped":
        parts = parts[:1]
    PR = (2 if prec == "bf16x3" else 1) * C // 8
    nphp = 256 // PR                                              # pixels in flight per round of a workgroup
    nchunk, ppc = chunking(B, N, hw)
    T = torch.zeros(B, C, N, dtype=torch.float64)
    for p in parts:
        flat = p.reshape(B, C, N, hw)
        for k in range(nchunk):
            ch = flat[..., k * ppc:min(hw, (k + 1) * ppc)]
            L = ch.shape[-1]
            if fault == "remainder_dropped" and k == nchunk - 1:
                L = L // nphp * nphp
                ch = ch[..., :L]
            J = -(-L // nphp) if L else 0
            if not J:
                continue
            ch = F.pad(ch, (0, J * nphp - L)).reshape(B, C, N, J, nphp)
            T = T + _seq32(ch, 3).double().sum(-1)
    nph = 256 // C
    line = lambda v: _acc4(v, nph).double().sum(-1)
    return [T, line(y2[:, :, :, 0, :]), line(y2[:, :, :, -1, :]), line(y2[:, :, :, :, 0]), line(y2[:, :, :, :, -1]),
            y2[:, :, :, 0, 0].double(), y2[:, :, :, 0, -1].double(), y2[:, :, :, -1, 0].double(), y2[:, :, :, -1, -1].double()]


def _sums_segments(y2, th, fault):
    """sums[9] from fp32 y2 as the tiles (th = 8: of_roll SUMS, two rows per wave) or rows (th = 1) forms leave and reduce them: the 16-pixel
    tree, the two-row add, flags per tile / row segment."""
    B, C, N, H, W = y2.shape
    tx = W // 16
    seg = y2.reshape(B, C, N, H, tx, 16)
    rs = _tree16(seg)                                              # (B,C,N,H,tx) float32
    first, last = seg[..., 0], seg[..., 15]
    if th == 8:                                                    # a wave's two rows in fp32
        tot = rs[:, :, :, 0::2] + rs[:, :, :, 1::2]
        fc, lc = first[:, :, :, 0::2] + first[:, :, :, 1::2], last[:, :, :, 0::2] + last[:, :, :, 1::2]
    else:
        tot, fc, lc = rs, first, last
    lef = torch.zeros(tx, dtype=torch.bool)
    lef[0] = True
    if fault == "interior_as_left" and tx > 2:
        lef[1] = True
    d = lambda t: t.double()
    col0 = (d(fc) * lef).sum(dim=(3, 4))
    return [d(tot).sum(dim=(3, 4)), d(rs[:, :, :, 0]).sum(-1), d(rs[:, :, :, -1]).sum(-1), col0, d(lc[..., -1]).sum(-1),
            (d(first[:, :, :, 0]) * lef).sum(-1), d(last[:, :, :, 0, -1]), (d(first[:, :, :, -1]) * lef).sum(-1), d(last[:, :, :, -1, -1])]


def _apply(sums, w6, bias6, hw, H, W, fault):
    """head_tail_apply in double: the 27 x C multiply-adds, the mean."""
    T, R0, RL, C0, CL, c00, c0w, ch0, chw = sums
    if fault == "corners_swapped":
        c0w, ch0 = ch0, c0w
    wd = w6.double()[:, :, 0]
    acc = torch.zeros(T.shape[0], 3, T.shape[2], dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            rsub = (R0 if fault == "row_swapped" else RL) if dy == 0 else (R0 if dy == 2 else 0.0)
            csub = (C0 if fault == "col_swapped" else CL) if dx == 0 else (C0 if dx == 2 else 0.0)
            S = T - rsub - csub
            if dy == 0 and dx == 0 and fault != "corner_missing":
                S = S + chw
            if dy == 0 and dx == 2:
                S = S + ch0
            if dy == 2 and dx == 0:
                S = S + c0w
            if dy == 2 and dx == 2:
                S = S + c00
            acc = acc + torch.einsum("oc,bcn->bon", wd[:, :, dy, dx], S)
    div = float((H - 1) * (W - 1)) if fault == "divisor" else float(hw)
    return (bias6.double().reshape(1, 3, 1) + acc / div).float()


def _mean_form(y2, w6, bias6, prec, fault):
    """conv .6 in the arithmetic into fp32 planes, then alpha_mean_kernel: four accumulators per thread, the shuffle tree, part[]."""
    B, C, N, H, W = y2.shape
    hw = H * W
    head = _conv_emu(y2, w6, None, bias6, prec, False, False).reshape(B, 3, N, hw)
    t = _acc4(head, 256)                                           # (B,3,N,256): a thread's sum
    waves = t.reshape(B, 3, N, 4, 64)
    for _ in range(6):
        waves = waves[..., 0::2] + waves[..., 1::2]
    part = waves[..., 0]
    div = float((H - 1) * (W - 1)) if fault == "divisor" else float(hw)
    return ((part[..., 0] + part[..., 1]) + (part[..., 2] + part[..., 3])) / torch.tensor(div, dtype=torch.float32)


def emulate(x, w2, bn2, w4, bn4, w6, bias6, alpha_in, prec, start, form, fault=None, y2=None):
    """(raw, alpha_out) float32 (B,3,N) as the form's kernels give them; ``fault``: one of FAULTS; ``y2``: a precomputed emulate_y2."""
    stored = form in ("planes", "mean")
    if y2 is None:
        y2 = emulate_y2(x, w2, bn2, w4, bn4, prec, stored) if start == 0 else records(x, prec)
    B, C, N, H, W = y2.shape
    if form == "mean":
        m = _mean_form(y2, w6, bias6, prec, fault)
    else:
        sums = _sums_planes(y2, prec, fault) if form == "planes" else _sums_segments(y2, 8 if form == "tiles" else 1, fault)
        m = _apply(sums, w6, bias6, H * W, H, W, fault)
    damp_c = 1 if fault == "damp_c1" else 0
    step = m.clone()
    step[:, damp_c] = torch.tensor(DAMP32) * m[:, damp_c]
    raw = step.clone() if fault == "raw_damped" else m
    alpha = step.clone() if fault == "alpha_overwritten" else alpha_in.float() + step
    if fault == "idx_order":   # idx = (b N + n) 3 + c instead of (b 3 + c) N + n: the same values at other places of the (B,3,N) block
        alpha = alpha_in.float().clone()
        fa, fr, fs, fm = alpha.reshape(B, -1), torch.zeros(B, 3 * N), step.reshape(B, 3, N), m.reshape(B, 3, N)
        for c in range(3):
            for n in range(N):
                fa[:, n * 3 + c] += fs[:, c, n]
                fr[:, n * 3 + c] = fm[:, c, n]
        raw = fr.reshape(B, 3, N)
    return raw, alpha


def can_act(fault, form, prec, B, N, H, W, C):
    """Whether a fault changes anything in a form at a shape (the CPU test names a case for every fault)."""
    if fault == "remainder_dropped":
        PR = (2 if prec == "bf16x3" else 1) * C // 8
        nchunk, ppc = chunking(B, N, H * W)
        return form == "planes" and (H * W - (nchunk - 1) * ppc) % (256 // PR) != 0
    if fault == "lo_dropped":
        return form == "planes" and prec == "bf16x3"
    if fault == "interior_as_left":
        return form in ("tiles", "rows") and W // 16 > 2
    if fault in ("corner_missing", "corners_swapped", "row_swapped", "col_swapped"):
        return form != "mean" and H > 1 and W > 1
    if fault == "divisor":
        return H > 1 and W > 1
    if fault == "idx_order":
        return N > 1
    return True


def gate_rel_l2(bad, good):
    """What the whole-network gate sees: the largest relative L2 over a sample's (3, N) tap."""
    b, g = bad.double(), good.double()
    return float(((b - g).flatten(1).norm(dim=1) / g.flatten(1).norm(dim=1).clamp_min(1e-300)).max())


GATE = 2e-5   # test_hip_e2e_head_tail_as_plane_sums: relative L2 over the 30 numbers of a head / alpha tap


def old_gate_table(H, W, prec="bf16x3", C=16, N=10):
    """fault -> (form, the larger of the raw and alpha taps' relative L2 against the clean emulation) on a smooth y0 of one sample: what the
    whole-network gate would have seen of each planted fault.  The form is the first of tiles, planes in which the fault can act (None, 0.0: in
    neither at this size)."""
    x = smooth_input(1, C, N, H, W)
    p = head_params("post_relu", C, seed=11)
    a = alpha_input(1, N, 5)
    y2 = {f: emulate_y2(x, *p[:4], prec, f == "planes") for f in ("tiles", "planes")}
    clean = {f: emulate(x, *p, a, prec, 0, f, y2=y2[f]) for f in y2}
    out = {}
    for fault in FAULTS:
        form = next((f for f in ("tiles", "planes") if can_act(fault, f, prec, 1, N, H, W, C)), None)
        if form is None:      # (a last chunk without remainder: the fault cannot act at this size at all)
            out[fault] = (None, 0.0)
            continue
        bad = emulate(x, *p, a, prec, 0, form, fault=fault, y2=y2[form])
        out[fault] = (form, max(gate_rel_l2(bad[0], clean[form][0]), gate_rel_l2(bad[1], clean[form][1])))
    return out


# ---- the cases of tests/test_gpu_head_tail.py; the CPU test calibrates the bound on them and checks their unresolved-ReLU shares -------------
PRECISIONS = ("bf16x3", "fp16", "bf16")
# start = 0, C = 16, whole 8 x 16 columns (B, N, H, W, DFFW_SRD_WGS): one tile; two tiles along one axis; an interior tile, B > 1; ten slices;
# 18 tiles on 8 workgroups (over HT_SEG and under 2 HT_SEG: at two tiles a segment the tenth segment starts past the last tile)
PAIR_SHAPES = [(1, 1, 8, 16, 0), (1, 2, 8, 32, 0), (1, 2, 16, 16, 0), (2, 3, 24, 48, 0), (1, 10, 32, 64, 0), (3, 1, 16, 96, 8)]
# start = 0 without the pair, at conv_sums_ok's floor of 256 tiles of 5 x 4 x 16: (C, (B, N, H, W)).  H = 68 is no multiple of the streaming
# kernels' 8-row columns, so split-bf16 takes conv_tile's row-sums variant there as the 16-bit arithmetics do everywhere
ROWS_CASES = [(32, (1, 1, 64, 256)), (64, (1, 1, 64, 256)), (32, (1, 1, 68, 256)), (64, (1, 1, 68, 256)), (32, (2, 6, 64, 64))]
# start = 2 (module docstring of the GPU test)
S2_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 7), (1, 2, 5, 1), (2, 3, 2, 2), (1, 2, 3, 37), (2, 3, 12, 20), (1, 1, 40, 52), (1, 1, 33, 128), (4, 10, 16, 24)]
S2_KINDS = ("random", "placed", "constant", "zero")
SHARE_CAP = {"bf16x3": 2.0 ** -7, "fp16": 0.5, "bf16": 1.0}   # ALPHA * 2^9, see test_head_tail.py::test_unresolved_relu_shares


def pair_case(i, kind="random"):
    """(x, params, alpha_in) of PAIR_SHAPES[i]: an eb regime (cycling) with eb-style parameters, or ("placed") impulses through centre-tap convs."""
    B, N, H, W, _ = PAIR_SHAPES[i]
    if kind == "placed":
        x = placed_input(B, 16, N, H, W)
        if W > 16:
            x[:, 1, :, H // 2, 16] = 1.0        # the first column of the second tile
        if H > 8:
            x[:, 2, :, 8, W // 2] = 1.0         # the first row of the second tile row
        return x, centre_params(16, 70 + i), alpha_input(B, N, 90 + i)
    regime = eb.REGIMES[i % len(eb.REGIMES)]
    return eb.regime_input(regime, (B, 16, N, H, W), seed=40 + i), head_params(regime, 16, 300 + i), alpha_input(B, N, 90 + i)


def rows_case(j, kind="random"):
    C, (B, N, H, W) = ROWS_CASES[j]
    if kind == "placed":
        x = placed_input(B, C, N, H, W)
        x[:, 1, :, H // 2, 16] = 1.0
        x[:, 2, :, 4, W // 2] = 1.0
        return x, centre_params(C, 170 + j), alpha_input(B, N, 190 + j)
    return eb.regime_input("post_relu", (B, C, N, H, W), seed=140 + j), head_params("post_relu", C, 400 + j), alpha_input(B, N, 190 + j)


def s2_case(C, shape, kind):
    """(y2, params, alpha_in): y2 random (post-ReLU: non-negative, half zeros), one 1.0 per plane, all ones, or all zeros with alpha_in = 0."""
    B, N, H, W = shape
    k = S2_SHAPES.index(shape)
    g = torch.Generator().manual_seed(500 + C + k)
    x = {"random": lambda: F.relu(torch.rand(B, C, N, H, W, generator=g) * 2 - 1), "placed": lambda: placed_input(B, C, N, H, W),
         "constant": lambda: torch.ones(B, C, N, H, W), "zero": lambda: torch.zeros(B, C, N, H, W)}[kind]()
    alpha = torch.zeros(B, 3, N) if kind == "zero" else alpha_input(B, N, 600 + k)
    return x, head_params("post_relu", C, 700 + C + k), alpha


# start = 0 below every fused form: 32 / 64 channels under conv_sums_ok's floor, 16 channels off the 8 x 16 columns: stored y2
STORED_CASES = [(32, (1, 2, 16, 32)), (64, (2, 1, 12, 20)), (16, (1, 3, 12, 20))]


def stored_case(j):
    C, (B, N, H, W) = STORED_CASES[j]
    regime = eb.REGIMES[(j + 2) % len(eb.REGIMES)]
    return eb.regime_input(regime, (B, C, N, H, W), seed=240 + j), head_params(regime, C, 800 + j), alpha_input(B, N, 290 + j)
