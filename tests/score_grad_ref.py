"""Reference, bounds and a CPU emulation for the backward of the score convs, Cin -> 1; shared by
tests/test_score_grad.py and tests/test_gpu_score_grad.py.

    grad_x[b,c,n,y,x]  = sum_{kz,ky,kx} w[c,kz,ky,kx] g[b, n+1-kz, y+1-ky, x+1-kx]  (+ b[b,c,n,y,x])      taps outside the volume contribute 0
    grad_w[c,kz,ky,kx] = sum_{b,n,y,x}  g[b,n,y,x] x[b,c, n+kz-1, y+ky-1, x+kx-1]

Reference: both formulas in float64 from the RECORD-ROUNDED x and b and the fp32 g and w (test_score_grad.py holds them against float64
autograd of F.conv3d).

Bounds, derived from the arithmetic (u = section 14's unit roundoff of one stored record, pw_grad_ref.U):

    grad_x, k111   (u + 2^-23) |ref64|: one fp32 rounding (w * g, or fmaf(w, g, b)), one split -- section 15's grad_combine bound
    grad_x, k333   gamma A + u (|ref64| + gamma A), gamma = 28 * 2^-24, A = sum |w| |g| + |b| at that element: 27 fmaf and one addition, each
                   rounding a partial sum of at most A by 2^-24; then one split of a value of at most |ref64| + gamma A
    grad_w         2^-24 |dW64| + L 2^-53 G, G = sum |g| |x|: the products are exact in float64, every term passes through at most L float64
                   additions (its thread's chain, the workgroup's tree or part sum, the ordered finish), then one rounding to fp32.
                   wgrad_chain() computes L from the volume and the grid (+ 2: the second-order terms of both roundings).

Data.  The bounds have no absolute term, so the test data keeps every product clear of the subnormal range of the format it is stored in:
magnitudes in [0.25, 1].  The one result that could still fall there is fp16's k111 sum w g + b under cancellation; for that case b takes the
sign of w g (make_case's ``aligned_b``), for the bf16 formats b's signs are free.
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_grad_ref as cg
from oracle import error_bounds as eb
from pw_grad_ref import U, rounded  # noqa: F401

PRECISIONS = cg.PRECISIONS
GEOMETRIES = {"k111": (1, 0), "k333": (3, 1)}     # name: (kernel, pad) on all three axes
# what dffw_score_grad.h fixes
UNIT_PIX, TY, TX, DEFAULT_WGS, SMALL_WGS = 512, 8, 8, 512, 8
TILE_PIX = TY * TX
GAMMA = 28 * 2.0 ** -24
TAPS3 = [(kz, ky, kx) for kz in range(3) for ky in range(3) for kx in range(3)]

# (B, N, h, w) and the channel counts of tests/test_gpu_score_grad.py.  k111: one pixel; less than a unit; exactly one unit; one unit and one
# pixel; two units and a ragged third.  k333: only the centre tap inside; a 2x2 plane of ten slices; odd sizes below a tile; several ragged
# tiles; whole tiles of several samples and slices
SHAPES = {
    "k111": [(1, 1, 1, 1), (2, 3, 8, 8), (2, 1, 16, 16), (1, 1, 19, 27), (1, 2, 23, 23)],
    "k333": [(1, 1, 1, 1), (1, 10, 2, 2), (2, 3, 5, 7), (1, 2, 9, 35), (2, 4, 16, 16)],
}
CHANNELS = {"k111": [8, 16, 32, 24, 128], "k333": [8, 32, 40]}
FAULTS = ("octets_swapped", "g_neighbour", "ragged_dropped", "slot_missing", "hi_only",
          "not_flipped", "next_sample", "row_wrap", "kykx_swapped", "ragged_summed")


def weight_shape(geom, C):
    k = GEOMETRIES[geom][0]
    return (1, C, k, k, k)


def units_of(geom, shape):
    B, N, H, W = shape
    if geom == "k111":
        return -(-(B * N * H * W) // UNIT_PIX)
    return B * N * -(-H // TY) * -(-W // TX)


def grid_of(geom, shape, wgs=DEFAULT_WGS):
    """persistent_grid: ``wgs`` workgroups rounded down to a multiple of 8, at least 8, never more per XCD than it has units."""
    return 8 * min(-(-units_of(geom, shape) // 8), max(1, wgs // 8))


def grids_of(geom, shape):
    """The grids a shape is tested on: the default, and with more than one unit also DFFW_SCORE_WGS=8."""
    return [DEFAULT_WGS, SMALL_WGS] if units_of(geom, shape) > 1 else [DEFAULT_WGS]


def make_case(geom, shape, C, seed, aligned_b=False):
    """(x, w, g, b): x, b (B,C,N,h,w), w (1,C,k,k,k), g (B,N,h,w), float32 CPU, magnitudes in [0.25, 1], signs random -- except b's with
    ``aligned_b`` (k111 only), which are those of w g."""
    B, N, H, W = shape
    gen = torch.Generator().manual_seed(seed)

    def mag(*s):
        return 0.25 + 0.75 * torch.rand(*s, generator=gen)

    def sgn(*s):
        return torch.randint(0, 2, s, generator=gen).float() * 2 - 1
    x = mag(B, C, N, H, W) * sgn(B, C, N, H, W)
    w = mag(*weight_shape(geom, C)) * sgn(*weight_shape(geom, C))
    g = mag(B, N, H, W) * sgn(B, N, H, W)
    b = mag(B, C, N, H, W)
    if aligned_b:
        assert geom == "k111"
        b = b * torch.sign(w.reshape(1, C, 1, 1, 1) * g[:, None])
    else:
        b = b * sgn(B, C, N, H, W)
    return x, w, g, b


def int_case(geom, shape, C, seed):
    """Small integers: exact in every format and in every order of summation."""
    B, N, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randint(-3, 4, s, generator=gen).float()
    return r(B, C, N, H, W), r(*weight_shape(geom, C)), r(B, N, H, W), r(B, C, N, H, W)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------------------
def shifts(g, k, fault=None):
    """[tap] -> g[b, n+1-kz, y+1-ky, x+1-kx] (zero outside the volume), taps in row-major (kz, ky, kx) order; k = 1: [g].  Faults: ``next_sample``
    takes the slice offset on the flat (sample, slice) axis, so the tap past a sample's last slice reads the next sample's first; ``row_wrap``
    takes the column offset on the flat (row, column) axis, so the halo column at a row end reads the next row's first pixel; ``not_flipped``
    reads g[p + k - 1]."""
    if k == 1:
        return [g]
    B, N, H, W = g.shape
    out = []
    for kz, ky, kx in TAPS3:
        dz, dy, dx = (kz - 1, ky - 1, kx - 1) if fault == "not_flipped" else (1 - kz, 1 - ky, 1 - kx)
        t = g
        if fault == "next_sample":
            t = F.pad(t.reshape(1, B * N, H, W), (0, 0, 0, 0, 1, 1))[:, 1 + dz:1 + dz + B * N].reshape(B, N, H, W)
        else:
            t = F.pad(t, (0, 0, 0, 0, 1, 1))[:, 1 + dz:1 + dz + N]
        if fault == "row_wrap":
            t = F.pad(t, (0, 0, 1, 1))[:, :, 1 + dy:1 + dy + H]
            t = F.pad(t.reshape(B, N, H * W), (1, 1))[:, :, 1 + dx:1 + dx + H * W].reshape(B, N, H, W)
        else:
            t = F.pad(t, (1, 1, 1, 1))[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        out.append(t)
    return out


def dgrad_of(w, g, b, geom):
    """grad_x in the dtype of its arguments."""
    k = GEOMETRIES[geom][0]
    S = torch.stack(shifts(g, k))
    out = torch.einsum("ct,tbnhw->bcnhw", w.reshape(w.shape[1], -1), S)
    return out if b is None else out + b


def wgrad_of(x, g, geom):
    """grad_w (1,C,k,k,k) in the dtype of its arguments."""
    k = GEOMETRIES[geom][0]
    S = torch.stack(shifts(g, k))
    return torch.einsum("tbnhw,bcnhw->ct", S, x).reshape(1, x.shape[1], k, k, k)


def dgrad_ref64(w, g, b, geom, prec):
    """(ref64, bound) of grad_x from the fp32 w and g and the record-rounded b."""
    w64, g64 = w.double(), g.double()
    b64 = None if b is None else rounded(b, prec).double()
    ref = dgrad_of(w64, g64, b64, geom)
    if geom == "k111":
        return ref, (U[prec] + 2.0 ** -23) * ref.abs()
    A = dgrad_of(w64.abs(), g64.abs(), None if b is None else b64.abs(), geom)
    return ref, GAMMA * A + U[prec] * (ref.abs() + GAMMA * A)


def wgrad_ref64(x, g, geom, prec, L):
    """(ref64, bound) of grad_w from the record-rounded x and the fp32 g; L: wgrad_chain()."""
    x64, g64 = rounded(x, prec).double(), g.double()
    ref = wgrad_of(x64, g64, geom)
    G = wgrad_of(x64.abs(), g64.abs(), geom)
    return ref, 2.0 ** -24 * ref.abs() + L * 2.0 ** -53 * G


def grads64(x, w, g, geom):
    """(grad_x, grad_w) of <g, conv(x, w)> by float64 autograd of F.conv3d: what the two formulas are held against."""
    x = x.detach().cpu().double().requires_grad_(True)
    w = w.detach().cpu().double().requires_grad_(True)
    y = F.conv3d(x, w, None, 1, GEOMETRIES[geom][1])[:, 0]
    return torch.autograd.grad(y, (x, w), g.detach().cpu().double())


# ---- the kernels' decomposition ------------------------------------------------------------------------------------------------------------------
def k111_lanes(C):
    """(octets, pixel lanes): a thread owns octet tid % (C/8) and pixel lane tid / (C/8) of the 256 / (C/8) a pass covers."""
    no = C // 8
    return no, 256 // no


def k333_parts(C):
    """(pairs, S): 27 * C/8 (tap, octet) pairs; up to 256 of them, S = 256 / pairs threads share a pair and split the tile's 64 pixels."""
    pairs = 27 * (C // 8)
    return pairs, (256 // pairs if pairs <= 256 else 1)


def tree_steps(pp):
    h, n = 1, 1
    while 2 * h < pp:
        h, n = 2 * h, n + 1
    return h, n


def wgrad_chain(geom, shape, C, wgs=DEFAULT_WGS):
    """L: the longest chain of float64 additions a term of grad_w passes through on the grid ``wgs`` gives, plus 2."""
    grid = grid_of(geom, shape, wgs)
    most = max(len(u) for u in cg.persistent_units(units_of(geom, shape), grid))
    if geom == "k111":
        _, pp = k111_lanes(C)
        return most * -(-UNIT_PIX // pp) + tree_steps(pp)[1] + grid + 2
    _, S = k333_parts(C)
    return most * -(-TILE_PIX // S) + (S - 1) + grid + 2


# ---- the kernels' arithmetic ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product is exact in float64; the float64 sum is rounded to odd (its residual
    from TwoSum decides), and a value rounded to odd at 53 bits rounds to nearest at 24 bits as the exact one does."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def emulate_dgrad(w, g, b, geom, prec, *, fault=None):
    """grad_x in the kernels' arithmetic.  k111: w * g or fmaf(w, g, b), then the split.  k333: 27 fmaf in row-major tap order from 0, then + b
    in fp32, then the split."""
    assert fault in (None,) + FAULTS, fault
    B, N, H, W = g.shape
    C = w.shape[1]
    br = None if b is None else rounded(b, prec).numpy()
    wn = w.reshape(C, -1).numpy()
    if geom == "k111":
        gv = g
        if fault == "g_neighbour":
            gv = torch.roll(g.reshape(-1), -1).reshape(g.shape)
        gn = gv.numpy()[:, None]                       # (B, 1, N, H, W)
        wv = wn[:, 0].copy()
        if fault == "octets_swapped":
            wv[8:16], wv[16:24] = wn[16:24, 0], wn[8:16, 0]
        wv = np.broadcast_to(wv.reshape(1, C, 1, 1, 1), (B, C, N, H, W))
        gb = np.broadcast_to(gn, (B, C, N, H, W))
        v = wv * gb if br is None else fma32(wv, gb, br)
        out = rounded(torch.from_numpy(np.ascontiguousarray(v)), prec)
        if fault == "ragged_dropped":
            M = B * N * H * W
            flat = out.permute(0, 2, 3, 4, 1).reshape(M, C).clone()
            flat[(M // UNIT_PIX) * UNIT_PIX:] = 0 if M % UNIT_PIX else flat[(M // UNIT_PIX) * UNIT_PIX:]
            out = flat.reshape(B, N, H, W, C).permute(0, 4, 1, 2, 3).contiguous()
        return out
    S = shifts(g, 3, fault)
    acc = np.zeros((B, C, N, H, W), dtype=np.float32)
    for t, sh in enumerate(S):
        acc = fma32(np.broadcast_to(wn[:, t].reshape(1, C, 1, 1, 1), acc.shape), np.broadcast_to(sh.numpy()[:, None], acc.shape), acc)
    if br is not None:
        acc = acc + br
    return rounded(torch.from_numpy(acc), prec)


def _ordered_sum(terms):
    """terms (steps, ...) float64: s = 0; s += terms[0]; s += terms[1]; ..."""
    s = np.zeros(terms.shape[1:], dtype=np.float64)
    for t in terms:
        s = s + t
    return s


def emulate_wgrad(x, g, geom, prec, *, wgs=DEFAULT_WGS, fault=None):
    """grad_w in the kernels' arithmetic: the record values of x (hi + lo) and the fp32 g as float64, their exact products added in float64
    -- per thread over its pixels in its order under persistent_range, over the workgroup (k111: the fixed tree; k333: the parts of a pair in
    order), over the workgroups' slots in workgroup order -- and rounded to fp32 once."""
    assert fault in (None,) + FAULTS, fault
    B, N, H, W = g.shape
    C = x.shape[1]
    shape = (B, N, H, W)
    xr = cg.round_parts(x, prec)[0] if fault == "hi_only" else rounded(x, prec)
    grid = grid_of(geom, shape, wgs)
    upw = cg.persistent_units(units_of(geom, shape), grid)
    most = max(1, max(len(u) for u in upw))
    if geom == "k111":
        M = B * N * H * W
        no, pp = k111_lanes(C)
        gv = g.reshape(-1)
        if fault == "g_neighbour":
            gv = torch.roll(gv, -1)
        prod = gv.double().numpy()[:, None] * xr.permute(0, 2, 3, 4, 1).reshape(M, C).double().numpy()      # exact
        prod = np.concatenate([prod, np.zeros((1, C))])                                                      # index M: nothing
        per_unit = -(-UNIT_PIX // pp)
        idx = np.full((grid, most * per_unit, pp), M, dtype=np.int64)
        full = M // UNIT_PIX
        for wg, units in enumerate(upw):
            for i, u in enumerate(units):
                if fault == "ragged_dropped" and u == full:
                    continue
                p = u * UNIT_PIX + np.arange(per_unit)[:, None] * pp + np.arange(pp)[None, :]
                p[(p >= min(M, (u + 1) * UNIT_PIX))] = M
                idx[wg, i * per_unit:(i + 1) * per_unit] = p
        red = _ordered_sum(np.moveaxis(prod[idx], 1, 0))          # (grid, pp, C): the threads' sums
        h, _ = tree_steps(pp)
        while h >= 1:
            n = min(h, pp - h)
            red[:, :n] = red[:, :n] + red[:, h:h + n]
            h //= 2
        slots = red[:, 0]                                         # (grid, C)
        if fault == "slot_missing":
            slots[int(np.abs(slots).sum(1).argmax())] = 0
        dw = _ordered_sum(slots)
        if fault == "octets_swapped":
            dw[8:16], dw[16:24] = dw[16:24].copy(), dw[8:16].copy()
        return torch.from_numpy(dw).float().reshape(1, C, 1, 1, 1)
    # k333: everything on the canvas of whole tiles
    ty, tx = -(-H // TY), -(-W // TX)
    Hc, Wc = ty * TY, tx * TX
    x64 = xr.double()
    if fault == "ragged_summed":      # the pixels outside a ragged tile's extent hold what follows in memory: the next rows' pixels
        flat = F.pad(x64.reshape(B, C, N * H * W), (0, Hc * Wc))
        rows = (torch.arange(Hc) * W)[:, None] + torch.arange(Wc)[None, :]
        idx = (torch.arange(N) * H * W)[:, None, None] + rows[None]
        xc = flat[:, :, idx]
    else:
        xc = F.pad(x64, (0, Wc - W, 0, Hc - H))
    if fault == "ragged_summed":      # ... and meet the halo's g of their real neighbours
        S = torch.stack(shifts(F.pad(g.double(), (0, Wc - W, 0, Hc - H)), 3))
    else:
        S = torch.stack([F.pad(t.double(), (0, Wc - W, 0, Hc - H)) for t in shifts(g, 3, fault)])            # (27, B, N, Hc, Wc)
    tiles = lambda t, lead: t.reshape(*lead, B, N, ty, TY, tx, TX)
    St = tiles(S, (27,)).permute(1, 2, 3, 5, 0, 4, 6).reshape(B * N * ty * tx, 27, TILE_PIX)                # (unit, tap, q)
    Xt = tiles(xc.permute(1, 0, 2, 3, 4), (C,)).permute(1, 2, 3, 5, 4, 6, 0).reshape(B * N * ty * tx, TILE_PIX, C)   # (unit, q, c)
    prod = (St[:, :, :, None] * Xt[:, None, :, :]).numpy()        # (unit, tap, q, c), exact
    prod = np.concatenate([prod, np.zeros((1,) + prod.shape[1:])])
    nil = prod.shape[0] - 1
    _, Sp = k333_parts(C)
    bounds = [(p * TILE_PIX // Sp, (p + 1) * TILE_PIX // Sp) for p in range(Sp)]
    plen = max(q1 - q0 for q0, q1 in bounds)
    acc = np.zeros((grid, Sp, 27, C))
    for i in range(most):
        unit = np.array([units[i] if i < len(units) else nil for units in upw])
        P = prod[unit]                                            # (grid, tap, q, c)
        for j in range(plen):
            for p, (q0, q1) in enumerate(bounds):
                if q0 + j < q1:
                    acc[:, p] = acc[:, p] + P[:, :, q0 + j]
    slots = _ordered_sum(np.moveaxis(acc, 1, 0))                  # the parts of a pair, in order: (grid, tap, c)
    dw = _ordered_sum(slots).T.reshape(C, 3, 3, 3)                # the finish, in workgroup order
    if fault == "kykx_swapped":
        dw = dw.transpose(0, 1, 3, 2)
    return torch.from_numpy(np.ascontiguousarray(dw)).float().reshape(1, C, 3, 3, 3)


def check(got, ref, bound, what=""):
    """max err / bound over every element (0 / 0 = 0); asserts that none exceeds 1.  NaN fails."""
    err = (got.detach().cpu().double() - ref).abs()
    ratio = eb._ratio(err, bound)
    worst = float(ratio.max())
    assert worst <= 1.0, "%s: %d of %d elements over the bound, worst err/bound %.3g" % (what, int((ratio > 1).sum()), ratio.numel(), worst)
    return worst


def worst_ratio(got, ref, bound):
    return float(eb._ratio((got.detach().cpu().double() - ref).abs(), bound).max())


def same_bits(a, b):
    """fp32 tensors equal bit for bit (so +0 and -0 differ)."""
    return torch.equal(a.detach().cpu().float().contiguous().view(torch.int32), b.detach().cpu().float().contiguous().view(torch.int32))
