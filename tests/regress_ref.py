"""Reference, per-element bound and fault-planting emulation of the regression heads, shared by tests/test_regress.py (CPU) and
tests/test_gpu_regress.py (GPU: dffw::regress_fused_kernel<10|16> and dffw::regress_kernel through dffw_op_regress_heads).

    v_n = bilinear(score[:, n], align_corners=False)    p_n = softplus(v_n) + 1e-6    q_n = p_n / sum_m p_m    d = sum_n f_n q_n

`reference` takes the tap indices and the weights ly, lx from PyTorch's float32 index rule -- scale = (float)h / (float)H,
s = (i + 0.5) * scale - 0.5 as ONE fused multiply-subtract, clamped at 0, second index clamped at h - 1 -- because the kernels copy that rule:
with sizes that do not divide, float64 weights differ from the float32 ones by ~2^-24 * s, which times a tap difference of up to 60 is far more
than the arithmetic under test.  The single rounding is part of the rule as PyTorch evaluates it (its CPU build contracts the expression, so do
its GPU kernels, and hipcc does in all three kernels here: v_fma_f32 .., -0.5); rounding the product first moves s by an ulp wherever
(i + 0.5) * scale is inexact -- never when h / H is a power of two, as in every head the network produces, but by up to 27 ulp of the result at
37 -> 111.  tests/test_regress.py::test_manual_taps_are_pytorchs holds `taps` to F.interpolate.  Everything after the weights is float64.

The bound, per output pixel (u = 2^-24):

    E = sum_n |f_n - d| q_n (EPS_SP + ALPHA u (1 + V_n))  +  ALPHA u (N + 2) sum_n |f_n| q_n

term by term:
  * d is a ratio of sums of p, so a RELATIVE error e_n of p_n moves it by sum_n (f_n - d) q_n e_n / (1 + sum q e): to first order
    sum_n |f_n - d| q_n |e_n|.  A common factor on all p cancels, and a slice whose focus distance is d does not matter.
  * e_n from softplus itself: EPS_SP = 0.75e-6, half of the 1.5e-6 that test_gpu_ops.py::test_softplus_pointwise_sweep allows on a ratio of two
    softplus_fast values (hardware exp2 / log / rcp).  The project's own number; the margin ALPHA does not scale it.
  * e_n from the error of v_n: d ln(p)/dv = sigmoid(v) / (softplus(v) + 1e-6) <= 1 (log(1 + x) >= x / (1 + x)), so an absolute error of v_n is at
    most the same relative error of p_n.  v_n = hy (hx s00 + lx s01) + ly (hx s10 + lx s11) with hy = 1 - ly, hx = 1 - lx rounded: four
    roundings on the path of every tap, each relative to a partial sum bounded by V_n = the same taps applied to |s|: c u V_n.
  * the "1 +": the rounding of softplus's result and of the addition of 1e-6 (float32(1e-6) is 2.5e-9 off), relative to p_n.
  * the sums: num = sum f_n p_n carries N roundings of additions and one per product, den = sum p_n N, the division one:
    at worst u ((N + 1) sum |f_n| q_n + (N + 1) |d|) <= u (2N + 2) sum |f_n| q_n.  The form keeps (N + 2); ALPHA >= 2 covers the rest.
  * ALPHA is measured, not chosen: four times the worst err / E of the float32 CPU emulation below (`emulate`, libm softplus) over CASES,
    taken with EPS_SP = 0 and ALPHA = 1, rounded up to a power of two -- the rule loss_ref.ALPHA follows.  The factor 4 is for what the GPU
    does differently: contracted multiply-adds in another association, exp2 / log / rcp at ~1 ulp each.
    tests/test_regress.py::test_calibration re-measures CAL.

What the bound cannot see: an error that stays relative to p and small against ALPHA u (1 + V_n) + EPS_SP = 4.8e-7 (1 + V_n) + 7.5e-7 per slice
plus the sums' term: one slice's p off by 2^-18 (3.8e-6 relative, 64 ulp) stays under it (tests/test_regress.py::test_bound_blind_spot).  A
softplus that is a few 1e-6 off is the sweep test's to find, not this one's."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS_SP = 0.75e-6
CAL = 1.47            # worst err / E (ALPHA = 1, EPS_SP = 0) of emulate(float32) over CASES: 1.465 at stride_n2, head (130, 130); test_calibration re-measures it
ALPHA = 8.0           # 4 * CAL = 5.9, rounded up to a power of two

FAULTS = ("no_clamp", "swap_lx", "drop_last", "last_twice", "fd_shift", "fd_pixel0", "no_floor", "single_load_h", "next_head_size")

NET4 = lambda H, W: [(H // 8, W // 8), (H // 4, W // 4), (H // 2, W // 2), (H, W)]
# (id, B, N, heads [(h, w)...], (H, W), focus-distance layout).  Every case runs in three forms: fused (regress_fused_kernel<10> for N <= 10,
# <16> for N <= 16, regress_kernel above), not fused (regress_kernel, blockIdx.y = head) and one dffw_op_regress call per head.
# Layouts: "dense" (B,N,H,W) varying per pixel; "bn11" (B,N,1,1); "1n11" (1,N,1,1) expanded over the batch (batch stride 0); "perm" a (B,H,W,N)
# buffer permuted to (B,N,H,W) (slice stride 1); "signed": dense with focus distances of both signs.
CASES = [
    # fused <10>: N on both sides of the five-slice blocks (1, 2: a tail of 4 and 3 clamped loads; 5: none; 9: a tail of one; 10: the last N)
    ("f10_n1_net4", 2, 1, NET4(32, 48), (32, 48), "bn11"),
    ("f10_n2_full_first", 1, 2, [(32, 48), (8, 12)], (32, 48), "dense"),
    ("f10_n5_net4", 2, 5, NET4(32, 48), (32, 48), "1n11"),
    ("f10_n5_thin", 1, 5, [(1, 5), (6, 1), (12, 20)], (12, 20), "perm"),          # h = 1 and w = 1: both taps of an axis are the one element
    ("f10_n9_full_first", 1, 9, [(32, 48), (16, 24), (4, 6)], (32, 48), "perm"),
    ("f10_n10_net4", 2, 10, NET4(32, 48), (32, 48), "signed"),
    # fused <16>: the first N past <10>, a tail of 4 (14), 15 (the only N a golden has) and 16 (the last block holds ONE slice)
    ("f16_n11_hmatch", 1, 11, [(16, 6), (16, 24)], (16, 24), "bn11"),             # h == H, w != W next to a head at output size
    ("f16_n14_net4", 2, 14, NET4(32, 48), (32, 48), "dense"),
    ("f16_n15_odd", 2, 15, [(5, 7), (3, 3), (12, 20)], (12, 20), "1n11"),         # sizes that do not divide
    ("f16_n16_down", 2, 16, [(16, 16), (8, 8)], (8, 8), "perm"),                  # downsampling
    # regress_kernel with several heads (N > 16)
    ("rk_n17_hmatch", 2, 17, [(16, 6), (16, 24)], (16, 24), "dense"),
    ("rk_n17_odd", 2, 17, [(5, 7), (3, 3), (12, 20)], (12, 20), "1n11"),
    ("rk_n20_net4", 1, 20, NET4(32, 48), (32, 48), "bn11"),
    ("rk_n20_thin", 2, 20, [(1, 5), (6, 1), (12, 20)], (12, 20), "perm"),
    # the second trip of the grid-stride loop: 1 081 600 pixels, 4096 workgroups of 256 cover 1 048 576
    ("stride_n2", 1, 2, [(130, 130), (1040, 1040)], (1040, 1040), "bn11"),
]
CASE_IDS = [c[0] for c in CASES]


def expected_kernel(N, n_heads, fused):
    if fused and n_heads > 1 and N <= 16:
        return "dffw::regress_fused_kernel<10>" if N <= 10 else "dffw::regress_fused_kernel<16>"
    return "dffw::regress_kernel"


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """CPU tensors of one case, built once: dict(id, B, N, H, W, scores [float32 (B,N,h,w)], fd (float32, broadcastable view, NOT contiguous
    where the layout says so), flat (index of the head whose scores are within +-1e-3)).
    Scores are uniform in +-30; in every other head the 2x2 corner block of sample 0 holds distinct values at or below -40 in every slice (output pixel
    (0, 0) then sees only the 1e-6 floor) and the last element of slice 0 of the last sample is 45 (softplus's linear branch)."""
    _, B, N, heads, (H, W), layout = CASES[CASE_IDS.index(cid)]
    g = torch.Generator().manual_seed(4000 + sum(map(ord, cid)))
    flat = len(heads) - 1 if heads[-1] != (H, W) or len(heads) == 2 else 1     # not always the full-resolution head
    scores = []
    for k, (h, w) in enumerate(heads):
        s = (torch.rand(B, N, h, w, generator=g) * 2 - 1) * (1e-3 if k == flat else 30.0)
        if k != flat:
            hh, ww = min(h, 2), min(w, 2)
            s[0, :, :hh, :ww] = -40.0 - 0.5 * torch.arange(N, dtype=torch.float32).view(N, 1, 1) \
                - 0.125 * torch.arange(hh * ww, dtype=torch.float32).view(1, hh, ww)
            s[B - 1, 0, h - 1, w - 1] = 45.0
        scores.append(s)
    base = torch.linspace(0.1, 1.5, N)
    if layout == "signed":
        base = torch.linspace(-0.7, 1.5, N)
    if layout in ("dense", "signed"):
        fd = base.view(1, N, 1, 1) * (1 + 0.3 * torch.rand(B, 1, H, W, generator=g)) + 0.05 * torch.rand(B, N, H, W, generator=g)
    elif layout == "perm":
        fd = (base.view(1, 1, 1, N) * (1 + 0.3 * torch.rand(B, H, W, 1, generator=g)) + 0.05 * torch.rand(B, H, W, N, generator=g)).permute(0, 3, 1, 2)
        assert fd.stride(1) == 1 or N == 1
    elif layout == "bn11":
        fd = base.view(1, N, 1, 1) * (1 + torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1))
    else:
        fd = (base * 1.25).view(1, N, 1, 1)
    return dict(id=cid, B=B, N=N, H=H, W=W, scores=scores, fd=fd, flat=flat, layout=layout)


def taps(n_out, n_in):
    """The float32 index rule along one axis: i0, i1 (clamped), i1 not clamped, l (float32 weight of i1).  The source coordinate is one fused
    multiply-subtract: the product is exact in float64, so the float64 expression rounded to float32 is that fma."""
    sc = (torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)).double()
    s = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * sc - 0.5).float().clamp(min=0)
    i0 = s.floor().long()
    i1 = i0 + 1
    return i0, i1.clamp(max=n_in - 1), i1, s - i0.float()


def _gather(flat, B, N, hu, wu, yi, xi):
    """flat[((b N + n) hu + y) wu + x] for all b, n, y in yi, x in xi, modulo the buffer's length (an emulated fault may index past it)."""
    b = torch.arange(B).view(B, 1, 1, 1)
    n = torch.arange(N).view(1, N, 1, 1)
    idx = ((b * N + n) * hu + yi.view(1, 1, -1, 1)) * wu + xi.view(1, 1, 1, -1)
    return flat[idx % flat.numel()]


def _interp(score, H, W, dtype, fault=None, size=None):
    """(v, V): the four-tap value in the kernels' formulation, every operation in `dtype`, and the same taps applied to |score|."""
    B, N, h, w = score.shape
    hu, wu = size if size is not None else (h, w)
    flat = score.to(dtype).reshape(-1)
    if fault == "single_load":
        yi, xi = torch.arange(H), torch.arange(W)
        v = _gather(flat, B, N, hu, wu, yi, xi)
        return v, v.abs()
    y0, y1, y1u, ly = taps(H, hu)
    x0, x1, x1u, lx = taps(W, wu)
    if fault == "no_clamp":
        y1, x1 = y1u, x1u
    ly, lx = ly.to(dtype).view(1, 1, H, 1), lx.to(dtype).view(1, 1, 1, W)
    hy, hx = 1 - ly, 1 - lx
    if fault == "swap_lx":
        lx, hx = hx, lx
    s00, s01, s10, s11 = (_gather(flat, B, N, hu, wu, yi, xi) for yi in (y0, y1) for xi in (x0, x1))
    v = hy * (hx * s00 + lx * s01) + ly * (hx * s10 + lx * s11)
    V = hy * (hx * s00.abs() + lx * s01.abs()) + ly * (hx * s10.abs() + lx * s11.abs())
    return v, V


def reference(score, fd, H, W):
    """One head in float64 on the float32 tap rule: dict(d (B,H,W), q, V, f (B,N,H,W))."""
    B, N = score.shape[:2]
    v, V = _interp(score, H, W, torch.float64)
    p = F.softplus(v) + 1e-6            # float64, torch's threshold 20
    q = p / p.sum(1, keepdim=True)
    f = fd.double().expand(B, N, H, W)
    return dict(d=(f * q).sum(1), q=q, V=V, f=f)


def bound(ref, alpha=ALPHA, eps_sp=EPS_SP):
    """E (B,H,W) float64 of the module docstring."""
    N = ref["q"].shape[1]
    d, q, f = ref["d"].unsqueeze(1), ref["q"], ref["f"]
    return ((f - d).abs() * q * (eps_sp + alpha * U * (1 + ref["V"]))).sum(1) + alpha * U * (N + 2) * (f.abs() * q).sum(1)


def emulate(scores, fd, H, W, dtype=torch.float32, fault=None):
    """All heads in the kernels' formulation, every step in `dtype`: hy*(hx*s00 + lx*s01) + ly*(hx*s10 + lx*s11), then den += p, num += f*p over the
    slices in order.  `fault` plants one defect:
      no_clamp        the second tap is not clamped at the right / bottom edge (it reads the next row / plane)
      swap_lx         lx and hx exchanged
      drop_last       the last slice left out of the sums
      last_twice      the last slice added twice (the tail of a five-slice block not masked)
      fd_shift        the focus distance of slice n - 1 used for slice n
      fd_pixel0       pixel (0, 0)'s focus distances used for every pixel of the sample
      no_floor        the 1e-6 left out
      single_load_h   the single-load branch (score[Y * w + X]) taken for a head with h == H but w != W
      next_head_size  head k read with head k + 1's h, w (the last with the first's)"""
    assert fault is None or fault in FAULTS, fault
    out = []
    n = len(scores)
    for k, score in enumerate(scores):
        B, N, h, w = score.shape
        size, f_int = None, fault if fault in ("no_clamp", "swap_lx") else None
        if fault == "next_head_size":
            size = tuple(scores[(k + 1) % n].shape[2:])
        if fault == "single_load_h" and h == H and w != W:
            f_int = "single_load"
        v, _ = _interp(score, H, W, dtype, fault=f_int, size=size)
        p = F.softplus(v) + (0.0 if fault == "no_floor" else 1e-6)
        f = fd.to(dtype).expand(B, N, H, W)
        if fault == "fd_shift":
            f = f[:, [max(i - 1, 0) for i in range(N)]]
        if fault == "fd_pixel0":
            f = f[:, :, :1, :1].expand(B, N, H, W)
        num, den = torch.zeros(B, H, W, dtype=dtype), torch.zeros(B, H, W, dtype=dtype)
        for i in list(range(N - 1 if fault == "drop_last" else N)) + ([N - 1] if fault == "last_twice" else []):
            den = den + p[:, i]
            num = num + f[:, i] * p[:, i]
        out.append(num / den)
    return out


def can_act(fault, case):
    """Whether a planted fault changes any operation of this case at all (tests/test_regress.py says why not, fault by fault)."""
    N, H, W = case["N"], case["H"], case["W"]
    sizes = [tuple(s.shape[2:]) for s in case["scores"]]
    if N == 1:      # d = f p / p: only a sum without its one term (0 / 0) shows
        return fault == "drop_last"
    if fault == "no_clamp":
        # the clamp engages where the first tap is the last row / column with a non-zero weight on the second: upsampling only
        def axis(n_out, n_in):
            i0, _, _, l = taps(n_out, n_in)
            return bool(((i0 == n_in - 1) & (l > 0)).any())
        return any(axis(H, h) or axis(W, w) for h, w in sizes)
    if fault == "fd_pixel0":
        return case["layout"] in ("dense", "signed", "perm")
    if fault == "single_load_h":
        return any(h == H and w != W for h, w in sizes)
    if fault == "next_head_size":
        return len(set(sizes)) > 1
    return True


def ratio(got, ref_d, E):
    """err / E per element, inf where got is not finite; 0 where both agree exactly."""
    err = (got.double() - ref_d).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(err == 0, torch.zeros_like(err), err / E)


@functools.lru_cache(maxsize=None)
def case_reference(cid):
    """[(reference dict, E)] per head of a case, computed once and shared; treat as read-only."""
    c = make_case(cid)
    refs = [reference(s, c["fd"], c["H"], c["W"]) for s in c["scores"]]
    return [(r, bound(r)) for r in refs]
