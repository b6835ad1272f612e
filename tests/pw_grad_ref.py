"""Reference, bounds and a CPU emulation for the backward of the convs without in-plane taps and for the gradient mask-and-add (DESIGN.md
section 15); shared by tests/test_pw_grad.py and tests/test_gpu_pw_grad.py.  The record helpers, persistent_units and make_case's regimes
are those of tests/conv_grad_ref.py.

Reference: float64 ``torch.autograd.grad`` of ``F.conv3d`` on the CPU.

Bounds.  Section 13's, with oracle.error_bounds.ALPHA unchanged.  grad_x is the adjoint conv run by the forward's own kernels:
``ALPHA[prec] * D`` of ``eb.conv_ref64`` on that conv.  grad_w is one dot product over the pixels per element with both operands rounded to
activation records:

    |dW - dW64| <= ALPHA[prec] * G,        G = sum |grad_y| * |x| over the same contraction

plus, for fp16, ``FP16_SUB * (sum |grad_y| + sum |x|)``.  The fp32 accumulation over pixels is kept short by the kernel (PARTIAL_PIXELS per
accumulator, then float64); ``emulate_pw_wgrad`` runs exactly that arithmetic and tests/test_pw_grad.py holds its worst err / bound under 0.5.

grad_combine ``out = [y > 0] a (+ b)``.  Without b the result is a's record or +0: exact.  With b the two record values (each exact in fp32)
are added in fp32 (one rounding, 2^-24 relative) and the sum is split into a record (u relative, section 14's u):
``|out - ref64| <= (u + 2^-23) |ref64|`` with ref64 formed from the record-rounded operands and the stored mask.  (fp16: every fp16 value is a
multiple of 2^-24, so a sum below the normal range is a subnormal exactly: no absolute term.)
"""
import torch
import torch.nn.functional as F

import conv_grad_ref as cg
from oracle import error_bounds as eb

GEOMETRIES = {          # name: (kernel, pad); stride 1, dilation 1, no bias
    "k311": ((3, 1, 1), (1, 0, 0)),
    "k111": ((1, 1, 1), (0, 0, 0)),
}
PRECISIONS = cg.PRECISIONS
# what dffw_conv_pw_wgrad.h fixes: a unit is a column of P flat pixels, a wave contracts WAVE_PIX of them per step (slice), the fp32
# accumulators are flushed after FLUSH_STEPS steps
P, WAVE_PIX, WAVES, FLUSH_STEPS = 128, 32, 4, 512
PARTIAL_PIXELS = WAVE_PIX * FLUSH_STEPS   # 16 384
U = {"bf16x3": 2.0 ** -16, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}   # unit roundoff of one stored record (section 14)


def weight_shape(geom, cin, cout):
    return (cout, cin) + GEOMETRIES[geom][0]


def conv64(x, w, geom):
    return F.conv3d(x, w, None, 1, GEOMETRIES[geom][1])


def grads64(x, w, gy, geom):
    """(grad_x, grad_w) of <gy, conv(x, w)> by float64 autograd."""
    x = x.detach().cpu().double().requires_grad_(True)
    w = w.detach().cpu().double().requires_grad_(True)
    return torch.autograd.grad(conv64(x, w, geom), (x, w), gy.detach().cpu().double())


def adjoint_conv(w, geom):
    """The data gradient as a conv of grad_y: the filter flipped along the slice axis, in / out channels swapped, the same padding."""
    return w.flip(2).transpose(0, 1).contiguous(), dict(stride=1, pad=GEOMETRIES[geom][1])


def dgrad_ref64(w, gy, geom):
    wa, kw = adjoint_conv(w, geom)
    return eb.conv_ref64(gy, wa, **kw)


def _wgrad_of(x, gy, geom):
    """dW[co][ci][kz] = sum_{b,n,p} gy[b,co,n,p] x[b,ci,n+kz-pz,p] in the dtype of its arguments (float64: the reference), shape (Cout,Cin,kd,1,1)."""
    k, p = GEOMETRIES[geom]
    N = x.shape[2]
    xp = F.pad(x, (0, 0, 0, 0, p[0], p[0]))
    taps = [torch.einsum("bonhw,binhw->oi", gy, xp[:, :, kz:kz + N]) for kz in range(k[0])]
    return torch.stack(taps, 2)[..., None, None]


def wgrad_ref64(x, gy, geom):
    """Ref64 of grad_w: reference, G = sum |gy| |x| as D, and the fp16 subnormal term."""
    x, gy = x.detach().cpu().double(), gy.detach().cpu().double()
    ref = _wgrad_of(x, gy, geom)
    G = _wgrad_of(x.abs(), gy.abs(), geom)
    sub = eb.FP16_SUB * (_wgrad_of(torch.ones_like(x), gy.abs(), geom) + _wgrad_of(x.abs(), torch.ones_like(gy), geom))
    return eb.Ref64(ref, ref, G, sub)


def make_case(regime, geom, B, cin, cout, N, H, W, seed):
    """(x, w, gy) float32 CPU tensors: conv_grad_ref.make_case's regimes zero_mean, post_relu (x) and offset (both) with this family's filter."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape: torch.rand(*shape, generator=g) * 2 - 1
    x, gy = u((B, cin, N, H, W)), u((B, cout, N, H, W))
    if regime == "post_relu":
        x = F.relu(x)
    elif regime == "offset":
        x, gy = 3 + 0.5 * x, 1 + 0.25 * gy
    else:
        assert regime == "zero_mean", regime
    kd = GEOMETRIES[geom][0][0]
    w = u(weight_shape(geom, cin, cout)) * (2.0 / (cin * kd)) ** 0.5 * 1.7
    return x, w, gy


def int_case(geom, B, cin, cout, N, H, W, seed):
    """Small integers: exact in every format and in every order of summation."""
    g = torch.Generator().manual_seed(seed)
    r = lambda shape: torch.randint(-3, 4, shape, generator=g).float()
    return r((B, cin, N, H, W)), r(weight_shape(geom, cin, cout)), r((B, cout, N, H, W))


# ---- the kernel's decomposition -----------------------------------------------------------------------------------------------------------------
def chunks_of(H, W):
    return -(-(H * W) // P)


def grid_x_of(B, H, W, cin, cout, wgs=512):
    """conv_pw_wgrad_grid_x: ``wgs`` workgroups over grid.x * grid.y, at least 8, a multiple of 8, never more per XCD than it has units."""
    ny = -(-cout // 16) * -(-cin // 32)
    total = B * chunks_of(H, W)
    return 8 * min(-(-total // 8), max(1, max(8, wgs // ny) // 8))


def steps_per_workgroup(B, N, H, W, grid_x):
    """Steps (one slice of one column: WAVE_PIX pixels per accumulator) every workgroup walks under persistent_range.  More than FLUSH_STEPS of
    them: each of its waves flushes a full-length fp32 partial and starts another."""
    return [len(units) * N for units in cg.persistent_units(B * chunks_of(H, W), grid_x)]


def _columns(t):
    """(B, C, N, H, W) -> (B, C, N, chunks * P): the flat plane, zero-filled to whole chunks."""
    B, C, N, H, W = t.shape
    return F.pad(t.reshape(B, C, N, H * W), (0, chunks_of(H, W) * P - H * W))


def _columns_running_on(t):
    """The planted fault: the ragged chunk filled with what follows the plane in memory (the next slice's, then the next sample's first pixels)."""
    B, C, N, H, W = t.shape
    hw, hwp = H * W, chunks_of(H, W) * P
    flat = F.pad(t.permute(1, 0, 2, 3, 4).reshape(C, B * N * hw), (0, hwp))
    idx = (torch.arange(B * N) * hw)[:, None] + torch.arange(hwp)[None, :]
    return flat[:, idx].reshape(C, B, N, hwp).permute(1, 0, 2, 3).contiguous()


def emulate_pw_wgrad(x, gy, geom, prec, *, grid_x=8, flush_steps=FLUSH_STEPS, fault=None):
    """grad_w in the kernel's arithmetic: operands rounded to the records of ``prec``; a workgroup walks its columns (persistent_range) slice by
    slice; per step each of its 4 waves adds, per slice tap inside the sample, one 32-pixel fp32 MFMA step per product (bf16x3: lo*hi, hi*lo,
    hi*hi, in that order) to its own fp32 accumulator; every ``flush_steps`` steps and at the end the accumulator goes into the wave's float64
    block; the blocks are added in float64 in (workgroup, wave) order.  A tap outside the sample adds nothing (the kernel skips it; here it
    multiplies a zero slice, which leaves an fp32 accumulator unchanged).  ``fault`` plants one of the errors tests/test_pw_grad.py names."""
    k, p = GEOMETRIES[geom]
    kd, pz = k[0], p[0]
    B, Cg, N, H, W = gy.shape
    Cf = x.shape[1]
    cols = _columns_running_on if fault == "ragged_runs_on" else _columns
    gp = [cols(t) for t in cg.round_parts(gy, prec)]
    fp = [F.pad(cols(t), (0, 0, pz, pz)) for t in cg.round_parts(x, prec)]       # slices -1 and N: zeros
    if fault == "next_sample" and pz:     # the tap past a sample's last slice reads the next sample's first slice
        for t in fp:
            t[:-1, :, N + pz] = t[1:, :, pz]
    nparts, chunks = len(gp), chunks_of(H, W)
    order = ((1, 0), (0, 1), (0, 0)) if nparts == 2 else ((0, 0),)
    blocks = []
    for units in cg.persistent_units(B * chunks, grid_x):
        total = torch.zeros(WAVES, kd, Cg, Cf, dtype=torch.float64)
        acc = torch.zeros(WAVES, kd, Cg, Cf, dtype=torch.float32)
        since = 0
        for u in units:
            b, c = divmod(u, chunks)
            px = slice(c * P, (c + 1) * P)
            for n in range(N):
                A = [t[b, :, n, px].reshape(Cg, WAVES, WAVE_PIX).permute(1, 0, 2) for t in gp]                                  # (wave, Cg, 32)
                Bm = [t[b, :, n:n + kd, px].reshape(Cf, kd, WAVES, WAVE_PIX).permute(2, 1, 3, 0) for t in fp]                  # (wave, kd, 32, Cf)
                if fault == "hi_only" and nparts == 2 and u % 2 == 0:
                    Bm[1] = torch.zeros_like(Bm[1])
                for ia, ib in order:
                    acc = acc + torch.matmul(A[ia].unsqueeze(1), Bm[ib])
                since += 1
                if since >= flush_steps:
                    total, acc, since = total + acc.double(), torch.zeros_like(acc), 0
        blocks.append(total + acc.double())
    if fault == "missing_wave":
        blocks[max(range(len(blocks)), key=lambda i: float(blocks[i][1].abs().sum()))][1] = 0
    dw = torch.zeros(kd, Cg, Cf, dtype=torch.float64)
    for blk in blocks:
        for wv in range(WAVES):
            dw = dw + blk[wv]
    dw = dw.permute(1, 2, 0).contiguous()
    if fault == "taps_reversed":
        dw = dw.flip(2)
    if fault == "swapped_octets":
        a, b = dw[Cg - 16:Cg - 8].clone(), dw[Cg - 8:].clone()
        dw[Cg - 16:Cg - 8], dw[Cg - 8:] = b, a
    return dw.float()[..., None, None]


# ---- grad_combine -------------------------------------------------------------------------------------------------------------------------------
def rounded(t, prec):
    """The value of t's activation record (hi + lo, exact in fp32)."""
    return sum(cg.round_parts(t, prec))


def combine_ref64(a, y, b, prec):
    """(ref64, bound) of out = [y > 0] a (+ b): formed in float64 from the record-rounded operands and the stored mask."""
    ref = rounded(a, prec).double()
    if y is not None:
        ref = torch.where(rounded(y, prec) > 0, ref, torch.zeros_like(ref))
    if b is None:
        return ref, torch.zeros_like(ref)
    ref = ref + rounded(b, prec).double()
    return ref, (U[prec] + 2.0 ** -23) * ref.abs()


def emulate_combine(a, y, b, prec, fault=None):
    """The kernel's arithmetic: the mask from the stored y; without b the record of a or +0; with b one fp32 addition, then the split."""
    v = rounded(a, prec)
    if y is not None:
        v = torch.where(rounded(a if fault == "mask_from_a" else y, prec) > 0, v, torch.zeros_like(v))
    if b is None or fault == "add_dropped":
        return v
    return rounded(v + rounded(b, prec), prec)
