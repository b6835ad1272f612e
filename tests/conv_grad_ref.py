"""Reference, bounds and a CPU emulation for the conv backward; shared by tests/test_conv_grad.py,
tests/test_gpu_conv_grad.py and tests/test_gpu_train_records.py (which also takes the record layout helpers from here).

Reference: float64 ``torch.autograd.grad`` of ``F.conv3d`` / ``F.conv_transpose3d`` on the CPU.

Bounds.  grad_x is the adjoint conv of grad_y run by the forward's own kernels, so its bound is ``oracle.error_bounds.conv_ref64`` applied to
that adjoint conv: ``ALPHA[prec] * D``, unchanged.  grad_w is one dot product over the pixels per element, its operands rounded to the
activation records exactly like a forward conv's, so the same per-product derivation gives

    |dW - dW64| <= ALPHA[prec] * G,        G = sum |grad_y| * |x| over the same contraction

(plus, for fp16, the subnormal term: an operand below the normal range is off by at most 2^-25 absolutely, ``FP16_SUB * (sum |grad_y| + sum |x|)``
over the contraction).  The result is fp32 and not rounded to a record, so there is no storage term.  The only new term against the forward is
the fp32 accumulation over pixels, which the kernel keeps short: its accumulators are flushed into float64 sums after at most PARTIAL_PIXELS
pixels (``emulate_wgrad`` runs exactly that arithmetic; tests/test_conv_grad.py holds its worst err / bound under 0.5).
"""
import torch
import torch.nn.functional as F

from oracle import error_bounds as eb

GEOMETRIES = {          # name: (kernel, stride, pad, transposed)
    "k333": ((3, 3, 3), (1, 1, 1), (1, 1, 1), False),
    "k133": ((1, 3, 3), (1, 1, 1), (0, 1, 1), False),
    "k333s2": ((3, 3, 3), (1, 2, 2), (1, 1, 1), False),
    "k333t": ((3, 3, 3), (1, 2, 2), (1, 1, 1), True),
}
PRECISIONS = ("bf16x3", "fp16", "bf16")
# what dffw_conv_wgrad.h fixes: a unit is TY x TX grid points, the fp32 accumulators are flushed after FLUSH_UNITS units
TY, TX, FLUSH_UNITS = 4, 16, 256
PARTIAL_PIXELS = TY * TX * FLUSH_UNITS   # 16 384


def weight_shape(geom, cin, cout):
    k, _, _, transposed = GEOMETRIES[geom]
    return (cin, cout) + k if transposed else (cout, cin) + k


def out_shape(geom, B, cin, cout, N, H, W):
    _, s, _, transposed = GEOMETRIES[geom]
    return (B, cout, N, 2 * H, 2 * W) if transposed else (B, cout, N, H // s[1], W // s[2])


def conv64(x, w, geom):
    k, s, p, transposed = GEOMETRIES[geom]
    if transposed:
        return F.conv_transpose3d(x, w, None, s, p, (0, 1, 1))
    return F.conv3d(x, w, None, s, p)


def grads64(x, w, gy, geom):
    """(grad_x, grad_w) of <gy, conv(x, w)> by float64 autograd."""
    x = x.detach().cpu().double().requires_grad_(True)
    w = w.detach().cpu().double().requires_grad_(True)
    return torch.autograd.grad(conv64(x, w, geom), (x, w), gy.detach().cpu().double())


def adjoint_conv(w, geom):
    """The data gradient as a conv of grad_y: (filter, kwargs of oracle.error_bounds.conv_ref64).  Stride 1: filter flipped, in / out swapped,
    padding k - 1 - p; stride (1,2,2): the transposed form on the same filter, and the other way round."""
    k, s, p, transposed = GEOMETRIES[geom]
    if s == (1, 1, 1):
        return w.flip(2, 3, 4).transpose(0, 1).contiguous(), dict(stride=1, pad=tuple(k[i] - 1 - p[i] for i in range(3)))
    return w, dict(stride=s, pad=p, transposed=not transposed)


def dgrad_ref64(w, gy, geom):
    """Ref64 (reference and per-element scale D) of grad_x."""
    wa, kw = adjoint_conv(w, geom)
    return eb.conv_ref64(gy, wa, **kw)


def _wgrad_of(x, gy, geom, wshape):
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(conv64(x, w, geom), w, gy)[0]


def wgrad_ref64(x, gy, geom, wshape):
    """Ref64 of grad_w: reference, G = sum |gy| |x| as D, and the fp16 subnormal term."""
    x, gy = x.detach().cpu().double(), gy.detach().cpu().double()
    ref = _wgrad_of(x, gy, geom, wshape)
    G = _wgrad_of(x.abs(), gy.abs(), geom, wshape)
    sub = eb.FP16_SUB * (_wgrad_of(torch.ones_like(x), gy.abs(), geom, wshape) + _wgrad_of(x.abs(), torch.ones_like(gy), geom, wshape))
    return eb.Ref64(ref, ref, G, sub)


# ---- CPU emulation of dffw::conv_wgrad_kernel + conv_wgrad_finish_kernel ---------------------------------------------------------------------
def round_parts(v, prec):
    """The parts of an activation record as float32 tensors: (hi, lo) for bf16x3, (hi,) otherwise."""
    v = v.float()
    if prec == "fp16":
        return (v.half().float(),)
    hi = v.bfloat16().float()
    if prec == "bf16":
        return (hi,)
    return hi, (v - hi).bfloat16().float()


_BITS = {"bf16x3": torch.bfloat16, "bf16": torch.bfloat16, "fp16": torch.float16}


def to_records(t, prec):
    """(B, C, N, H, W) float32 -> the activation records the library reads, an int16 tensor [B, N, H, W, parts, C]: ``[pixel][part][channel]``,
    part 0 = hi, part 1 = lo (split-bf16 only), each the bit pattern of ``round_parts``' value.  The device's split (Fmt::split, dffw_device.h)
    is the same round-to-nearest-even hi = bf16(v), lo = bf16(v - hi), or half(v)."""
    parts = [p.to(_BITS[prec]).view(torch.int16).permute(0, 2, 3, 4, 1) for p in round_parts(t.detach().cpu(), prec)]
    return torch.stack(parts, dim=4).contiguous()


def from_records(r, prec, C):
    """The inverse of ``to_records``: int16 records [B, N, H, W, parts, C] -> (B, C, N, H, W) float32, hi + lo."""
    nparts = 2 if prec == "bf16x3" else 1
    assert r.dtype == torch.int16 and r.dim() == 6 and r.shape[4] == nparts and r.shape[5] == C, (r.dtype, tuple(r.shape), prec, C)
    v = r.detach().cpu().contiguous().view(_BITS[prec]).float()
    v = v[..., 0, :] + v[..., 1, :] if nparts == 2 else v[..., 0, :]
    return v.permute(0, 4, 1, 2, 3).contiguous()


def persistent_units(total, grid_x):
    """Units of every workgroup under the rule of dffw_persist.h (persistent_range): workgroup b serves XCD b % 8, a contiguous range of the units."""
    per_xcd = grid_x // 8
    q, rem = divmod(total, 8)
    out = []
    for b in range(grid_x):
        xcd, widx = b % 8, b // 8
        xs = xcd * (q + 1) if xcd < rem else rem * (q + 1) + (xcd - rem) * q
        end = xs + q + (1 if xcd < rem else 0)
        out.append(list(range(xs + widx, end, per_xcd)))
    return out


def counted_units(geom, B, N, Hg, Wg, grid_x):
    """[slice tap][workgroup] -> the units that workgroup really sums on the grid-side volume (B, N, Hg, Wg): its persistent range without the
    units whose slice tap falls into the slice padding.  More than FLUSH_UNITS of them: the workgroup flushes a full-length fp32 partial."""
    k, _, p, _ = GEOMETRIES[geom]
    per_slice = -(-Hg // TY) * -(-Wg // TX)
    upw = persistent_units(B * N * per_slice, grid_x)
    return [[sum(0 <= (u // per_slice) % N + kz - p[0] < N for u in units) for units in upw] for kz in range(k[0])]


def _units(t, Hg, Wg):
    """(B, C, N, Hg, Wg) -> (units, 2 chunks, 32 pixels, C): units numbered x fastest, then y, slice, sample; a chunk is two tile rows."""
    B, C, N = t.shape[:3]
    ty, tx = -(-Hg // TY), -(-Wg // TX)
    t = F.pad(t, (0, tx * TX - Wg, 0, ty * TY - Hg))
    t = t.reshape(B, C, N, ty, TY // 2, 2, tx, TX).permute(0, 2, 3, 6, 4, 5, 7, 1)
    return t.reshape(B * N * ty * tx, TY // 2, 2 * TX, C)


def emulate_wgrad(x, gy, geom, prec, *, grid_x=8, flush_units=FLUSH_UNITS, fault=None):
    """grad_w in the kernel's arithmetic: operands rounded to the records of ``prec``; per 32-pixel chunk one fp32 MFMA step per product (for
    bf16x3 lo*hi, hi*lo, hi*hi, in that order) added to an fp32 accumulator; the accumulator added to a float64 sum every ``flush_units`` units and
    at the end; the workgroups' sums added in float64 in workgroup order.  ``fault`` plants one of the errors tests/test_conv_grad.py names."""
    k, s, p, transposed = GEOMETRIES[geom]
    S = s[1]
    g, f = (x, gy) if transposed else (gy, x)      # the transposed conv's weight gradient: the stride-2 kernel with the roles swapped
    if fault == "no_swap":
        g, f = f, g
    B, Cg, N, Hg, Wg = g.shape
    Cf = f.shape[1]
    gp = [_units(t, Hg, Wg) for t in round_parts(g, prec)]
    fparts = round_parts(f, prec)
    nu = gp[0].shape[0]
    upw = persistent_units(nu, grid_x)
    per_slice = nu // (B * N)
    dw = torch.zeros(Cg, Cf, k[0], 3, 3, dtype=torch.float64)
    for kz in range(k[0]):
        dz = kz - p[0]
        taps = []
        for ky in range(3):
            for kx in range(3):
                oy, ox = ky - 1, kx - 1
                if fault == "odd_pixel" and S == 2 and (ky, kx) == (0, 0):
                    oy, ox = oy + 1, ox + 1
                parts = []
                for t in fparts:
                    tp = F.pad(t, (1, S, 1, S, 1, 1))
                    if fault == "z_neighbour":     # the slice padding read from the neighbouring slice instead of zeros
                        tp[:, :, 0], tp[:, :, -1] = tp[:, :, 1], tp[:, :, -2]
                    tp = tp[:, :, 1 + dz:1 + dz + N, 1 + oy:1 + oy + S * Hg:S, 1 + ox:1 + ox + S * Wg:S]
                    parts.append(_units(tp, Hg, Wg))
                taps.append(parts)
        nparts = len(gp)
        blocks = []
        for wg, units in enumerate(upw):
            total = torch.zeros(Cg, Cf, 9, dtype=torch.float64)
            acc = torch.zeros(Cg, Cf, 9, dtype=torch.float32)
            since = 0
            for u in units:
                nf = (u // per_slice) % N + dz
                if (nf < 0 or nf >= N) and fault != "z_neighbour":
                    continue
                for c in range(TY // 2):
                    A = [gp[i][u, c].t().contiguous() for i in range(nparts)]                    # (Cg, 32)
                    Bm = [torch.stack([taps[t][i][u, c] for t in range(9)], 0) for i in range(nparts)]   # (9, 32, Cf)
                    if fault == "hi_only" and nparts == 2 and u % 2 == 0:
                        Bm[1] = torch.zeros_like(Bm[1])
                    order = ((1, 0), (0, 1), (0, 0)) if nparts == 2 else ((0, 0),)
                    for ia, ib in order:
                        acc = acc + torch.matmul(A[ia].unsqueeze(0), Bm[ib]).permute(1, 2, 0)
                since += 1
                if since >= flush_units:
                    total, acc, since = total + acc.double(), torch.zeros_like(acc), 0
            blocks.append(total + acc.double())
        if fault == "missing_partial":
            blocks[max(range(len(upw)), key=lambda i: len(upw[i]))] *= 0
        for blk in blocks:
            dw[:, :, kz] += blk.reshape(Cg, Cf, 3, 3)
    if fault == "drop_product":                    # one product of one pixel never summed: the largest one of element [0, 0, centre tap]
        kc = k[0] // 2
        prod = (g.double()[:, 0] * f.double()[:, 0, :, ::S, ::S]).reshape(-1)
        dw[0, 0, kc, 1, 1] -= prod[prod.abs().argmax()]
    return dw.float()


def make_case(regime, geom, B, cin, cout, N, H, W, seed, impulse_channel=None):
    """(x, w, gy) float32 CPU tensors of a regime: zero_mean, post_relu (x), offset (both), impulse (a unit-impulse gy, in channel
    ``impulse_channel``; None: cout // 2), one_sample (gy zero except in the last sample of the batch)."""
    g = torch.Generator().manual_seed(seed)
    xs, ys = (B, cin, N, H, W), out_shape(geom, B, cin, cout, N, H, W)
    u = lambda shape: torch.rand(*shape, generator=g) * 2 - 1
    x, gy = u(xs), u(ys)
    if regime == "post_relu":
        x = F.relu(x)
    elif regime == "offset":
        x, gy = 3 + 0.5 * x, 1 + 0.25 * gy
    elif regime == "impulse":
        gy = torch.zeros(ys)
        gy[B - 1, cout // 2 if impulse_channel is None else impulse_channel, N // 2, ys[3] // 2, ys[4] - 2] = 1.0
    elif regime == "one_sample":   # every other sample of the batch contributes exact zeros
        gy[:B - 1] = 0.0
    kk = GEOMETRIES[geom][0]
    w = u(weight_shape(geom, cin, cout)) * (2.0 / (cin * kk[0] * 9)) ** 0.5 * 1.7
    return x, w, gy
