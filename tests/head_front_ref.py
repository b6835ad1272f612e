"""Reference, per-element bound and CPU emulation of the front half of an alpha head (``head_first_conv()`` in csrc/dffw_align.cpp, tested
through ``dffw_op_head_front``) and of ``fov_warp_kernel`` (``dffw_op_fov_warp``).  A plain module like head_tail_ref.py; DESIGN.md §24
holds the derivation.

Operation (End_to_End.py:77-101, 106-134).  Per sample b and slice n: f = alpha0 + fov, lin_x = -1 + 2 x / (W - 1),
    flow_x = (W // 2) (f - 1) lin_x + alpha1,    flow_y = (H // 2) (f - 1) lin_y + alpha2,    s = (x - flow_x, y - flow_y)
(a plane of width 1 is sampled at 0: grid_sample's un-normalisation multiplies by W - 1), warp(fe)[b,:,n,y,x] = the bilinear sample of
fe[b,:,n] at s with zeros outside, and
    y0[b,:,n] = relu(BN(conv1x3x3([warp(fe)[b,:,N-1] | warp(fe)[b,:,n] | flow_x, flow_y of slice n], w0))).
The head forms sample in the plane only: they do NOT blend across slices (the reference's third grid coordinate is the slice index up to
an ulp; fov_warp_kernel, which keeps that blend, is treated at the end of this module).

Reference (``reference``).  Float64 throughout on the record-rounded fe: positions, flow, sample, then eb.conv_ref64 with bn0, ReLU and
pad (0, 1, 1).  It does not reproduce the kernels' float32 positions: a kernel position on the other side of an integer is covered by the
bound, no element is left out.

Bound.  E = CAL_FACTOR (own + carried), u = 2^-24:
* own      eb's bound of the conv on the reference volume (operand term: the storage rounding of the warped values and of the flow; + the
           stored #ref part |s0 conv(ref, w0[:, :C])| as a residual term: one D serves the three forms).
* carried  |s0| conv(E_in, |w0|) (eb._carry), E_in the absolute error of the conv's input, per element:
    flow channels     dflow  = u ((g + M |f|) |lin| + 3 g + 2 g |lin| + |flow|),   M = W // 2, g = M |f - 1|
                      (alpha0 + fov rounded: u |f|, f - 1: u |f - 1|, both times M |lin|; lin: 3 u (the step, its product, the sum), times g; the
                      two products: 2 u g |lin|; the sum with the shift: u |flow|)
    sample position   ds     = dflow + u (5 |x - flow| + (W - 1) / 2)
                      (x - flow, the division, the product with W - 1 and the sum g + 1: u |x - flow| each; the difference q - 1, |q - 1| <=
                      |q| + 1, in pixels: u (|x - flow| + (W - 1) / 2): the cancellation); 0 on a plane of width 1
    warped channels   E_in   = (1 + K u) (Lx dsx + Ly dsy) + K u A,   K = 7
                      Lx / Ly: the largest horizontal / vertical difference of neighbouring pixels of the zero-padded plane over the reference's
                      cell and its eight neighbours (4 x 4 pixels).  The sample is continuous and piecewise bilinear in s, inside a cell its
                      slope in x is a mean of two horizontal differences, so |sample(s) - sample(s')| <= Lx |dsx| + Ly |dsy| across cell and
                      image borders alike: a flipped floor stays inside the window (ds << 1).  A = the sample of |fe| at s; the blend's own
                      arithmetic is K roundings on the kernel's cell, whose sum of |v_k| w_k is within Lx dsx + Ly dsy of A (K: two weight
                      complements, their product, the product with the value, three additions; sx - floor(sx) is exact).
  E_in is not scaled by eb.ALPHA: it is the same in every arithmetic.

Calibration (§18's rule).  CAL_WORST is the clean emulation's worst err / E without the factor over every case of the GPU test (``case``),
every form, arithmetic and both contraction variants of the positions; CAL_FACTOR = 4 CAL_WORST rounded up to a power of two;
tests/test_head_front.py::test_calibration re-measures it.  Never from a GPU result.

Emulation (``emulate``).  float32 positions as warp_point computes them, with a*b+c either contracted or not (hipcc may do either),
warp_octet's corner order (dy outer, dx inner), records via the arithmetic's split, the conv as head_tail_ref._conv_emu does it (BN folded
in fp32, operands split, fp32 accumulation in torch's order, fp32 shift, the stored #ref part added in front of the ReLU in the split
forms).  FAULTS are arguments of the emulation."""
import math

import torch
import torch.nn.functional as F

from oracle import error_bounds as eb

U = 2.0 ** -24
K_BLEND = 7
K_BLEND3 = 13         # fov_warp_kernel's 8 corners: three complements, two products of weights, the product with the value, seven additions
PAD = (0, 1, 1)
FORMS = ("warp", "split", "whole")
HEADS = {8: "conv3", 16: "conv2", 32: "conv1"}
PRECISIONS = ("bf16x3", "fp16", "bf16")
WARP_MAX_PLANES = 320  # head_warp_max_planes()
CAL_WORST = 0.66      # worst err / E (CAL_FACTOR = 1) of the clean emulation over cases(); test_calibration re-measures it
CAL_FACTOR = 4.0      # 4 * CAL_WORST = 2.64, rounded up to a power of two
FOV_CAL_WORST = 0.71  # the same for fov_warp_kernel over fov_case() (the flow's last rounding, u |flow|, where nothing else acts)
FOV_CAL_FACTOR = 4.0
FAULTS = ("next_slice_params", "next_column_sample", "xc_eq_w", "flow_outside", "ref_neighbour_sample", "ref_slice0", "lo_dropped", "flow_swapped",
          "alpha0_ref")


# ---- records ---------------------------------------------------------------------------------------------------------------------------
def _split(v, prec):
    if prec == "fp16":
        hi = v.half().float()
        return hi, torch.zeros_like(hi)
    hi = v.bfloat16().float()
    return hi, ((v - hi).bfloat16().float() if prec == "bf16x3" else torch.zeros_like(hi))


def records(x, prec):
    """x as the activation records hold it (float32: hi + lo is exact in fp32 for split-bf16)."""
    hi, lo = _split(x.float(), prec)
    return hi + lo


# ---- float64 geometry and its error terms ------------------------------------------------------------------------------------------------
def _axis64(f, shift, size):
    """One axis: (flow, position, dflow, dpos), each (B, N, size) float64; f, shift (B, N) float64."""
    M = float(size // 2)
    i = torch.arange(size, dtype=torch.float64)
    lin = (-1.0 + 2.0 * i / (size - 1)) if size > 1 else torch.full((1,), -1.0, dtype=torch.float64)
    f, shift = f.unsqueeze(-1), shift.unsqueeze(-1)
    flow = M * (f - 1.0) * lin + shift
    g = M * (f - 1.0).abs()
    dflow = U * ((g + M * f.abs()) * lin.abs() + 3.0 * g + 2.0 * g * lin.abs() + flow.abs())
    if size == 1:
        return flow, torch.zeros_like(flow), dflow, torch.zeros_like(flow)
    pos = i - flow
    return flow, pos, dflow, dflow + U * (5.0 * pos.abs() + (size - 1) / 2.0)


class Geometry:
    """fx, sx, dfx, dsx: (B, N, 1, W); fy, sy, dfy, dsy: (B, N, H, 1); float64."""

    def __init__(self, alpha, fov, H, W, alpha0_from_sample0=False):
        a = alpha.double()
        a0 = a[:1, 0].expand_as(a[:, 0]) if alpha0_from_sample0 else a[:, 0]
        f = a0 + fov.double()
        self.fx, self.sx, self.dfx, self.dsx = (t.unsqueeze(2) for t in _axis64(f, a[:, 1], W))
        self.fy, self.sy, self.dfy, self.dsy = (t.unsqueeze(3) for t in _axis64(f, a[:, 2], H))
        self.B, self.N, self.H, self.W = a.shape[0], a.shape[2], H, W

    def full(self, t):
        return t.expand(self.B, self.N, self.H, self.W)


P4 = 4   # zero padding of the planes: the reference's cell and its neighbours fit for every clamped cell


def _cells(s, size):
    """floor(s) clamped to [-3, size + 1] (beyond: both corners and the whole window lie in the padding) and the weight of the upper corner."""
    c0 = torch.floor(s)
    return c0.clamp(-3, size + 1).long(), s - c0


def _gather(planes_p, yi, xi):
    """planes_p (B, N, C, Hp, Wp) at padded integer positions yi, xi (B, N, H, W) -> (B, N, C, H, W)."""
    B, N, C, Hp, Wp = planes_p.shape
    idx = (yi * Wp + xi).reshape(B, N, 1, -1).expand(B, N, C, -1)
    return planes_p.reshape(B, N, C, Hp * Wp).gather(3, idx).reshape(B, N, C, *yi.shape[2:])


def sample64(planes, geo):
    """planes (B, N, C, H, W) float64 sampled at geo's positions: (value, A = the sample of |planes|, Lx, Ly), each (B, N, C, H, W)."""
    H, W = geo.H, geo.W
    pp = F.pad(planes, (P4, P4, P4, P4))
    x0, wx = _cells(geo.full(geo.sx), W)
    y0, wy = _cells(geo.full(geo.sy), H)
    wx, wy = wx.unsqueeze(2), wy.unsqueeze(2)
    v = A = 0.0
    for dy in (0, 1):
        for dx in (0, 1):
            c = _gather(pp, y0 + dy + P4, x0 + dx + P4)
            w = (wx if dx else 1.0 - wx) * (wy if dy else 1.0 - wy)
            v, A = v + c * w, A + c.abs() * w
    B, N, C = planes.shape[:3]
    flat = lambda t: t.reshape(B * N, C, *t.shape[3:])
    dxm = F.max_pool2d(flat((pp[..., 1:] - pp[..., :-1]).abs()), (4, 3), 1)          # rows y0-1 .. y0+2, differences x0-1 .. x0+1 at [y0+3, x0+3]
    dym = F.max_pool2d(flat((pp[..., 1:, :] - pp[..., :-1, :]).abs()), (3, 4), 1)
    Lx = _gather(dxm.reshape(B, N, C, *dxm.shape[2:]), y0 + 3, x0 + 3)
    Ly = _gather(dym.reshape(B, N, C, *dym.shape[2:]), y0 + 3, x0 + 3)
    return v, A, Lx, Ly


def window_max(planes, geo):
    """The largest value of planes (B, N, C, H, W; non-negative, zero outside) over the 4 x 4 pixels of the reference's cell and its neighbours."""
    B, N, C = planes.shape[:3]
    pp = F.pad(planes, (P4, P4, P4, P4))
    x0, _ = _cells(geo.full(geo.sx), geo.W)
    y0, _ = _cells(geo.full(geo.sy), geo.H)
    m = F.max_pool2d(pp.reshape(B * N, C, *pp.shape[3:]), (4, 4), 1)
    return _gather(m.reshape(B, N, C, *m.shape[2:]), y0 + 3, x0 + 3)


def _input_error(A, Lx, Ly, geo, k=K_BLEND):
    ds = Lx * geo.full(geo.dsx).unsqueeze(2) + Ly * geo.full(geo.dsy).unsqueeze(2)
    return (1.0 + k * U) * ds + k * U * A


class FrontRef:
    """ref: float64 (B, 2C, N, H, W); vol: the reference volume [ref | cur | flow]; E(prec): the bound per element; terms: own / carried."""


def reference(fe, w0, bn0, alpha, fov, prec, factor=CAL_FACTOR):
    x = records(fe, prec).double()
    B, C, N, H, W = x.shape
    geo = Geometry(alpha, fov, H, W)
    v, A, Lx, Ly = sample64(x.permute(0, 2, 1, 3, 4), geo)
    e = _input_error(A, Lx, Ly, geo)
    ncdhw = lambda t: t.permute(0, 2, 1, 3, 4)
    cur, e_cur = ncdhw(v), ncdhw(e)
    last = lambda t: t[:, :, N - 1:].expand(-1, -1, N, -1, -1)
    flow = torch.stack([geo.full(geo.fx), geo.full(geo.fy)], 1)
    e_flow = torch.stack([geo.full(geo.dfx), geo.full(geo.dfy)], 1)
    vol = torch.cat([last(cur), cur, flow], 1)
    e_in = torch.cat([last(e_cur), e_cur, e_flow], 1)
    r = eb.conv_ref64(vol, w0, pad=PAD, bn=bn0, relu=1)
    s0, _ = eb.fold_bn(bn0, 2 * C)
    refpart = F.conv3d(vol[:, :C], w0.double()[:, :C], None, 1, PAD) * s0.reshape(1, -1, 1, 1, 1)
    out = FrontRef()
    out.ref, out.vol, out.prec = r.ref, vol, prec
    own = eb.ALPHA[prec] * (r.D + refpart.abs()) + (r.sub if prec == "fp16" else 0.0)
    carried = eb._carry(e_in, w0, s0, PAD)
    out.terms = {"own": own, "carried": carried}
    out.E = factor * (own + carried)
    return out


def literal(fe, w0, bn0, alpha, fov, prec):
    """The same numbers from a literal composition: torch's grid_sample on the normalised float64 grid, F.conv3d, eval-mode batch norm, relu."""
    x = records(fe, prec).double()
    B, C, N, H, W = x.shape
    a, f = alpha.double(), alpha.double()[:, 0] + fov.double()
    lin = lambda n: torch.linspace(-1, 1, n, dtype=torch.float64)
    fx = (W // 2) * (f - 1).reshape(B, N, 1, 1) * lin(W).reshape(1, 1, 1, W) + a[:, 1].reshape(B, N, 1, 1)
    fy = (H // 2) * (f - 1).reshape(B, N, 1, 1) * lin(H).reshape(1, 1, H, 1) + a[:, 2].reshape(B, N, 1, 1)
    fx, fy = fx.expand(B, N, H, W), fy.expand(B, N, H, W)
    gx = 2.0 * (torch.arange(W, dtype=torch.float64).reshape(1, 1, 1, W) - fx) / max(W - 1, 1) - 1.0
    gy = 2.0 * (torch.arange(H, dtype=torch.float64).reshape(1, 1, H, 1) - fy) / max(H - 1, 1) - 1.0
    grid = torch.stack([gx, gy], -1).reshape(B * N, H, W, 2)
    warped = F.grid_sample(x.permute(0, 2, 1, 3, 4).reshape(B * N, C, H, W), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    warped = warped.reshape(B, N, C, H, W).permute(0, 2, 1, 3, 4)
    vol = torch.cat([warped[:, :, N - 1:].expand(-1, -1, N, -1, -1), warped, torch.stack([fx, fy], 1)], 1)
    g, b, mu, var = (t.double() for t in bn0)
    return F.relu(F.batch_norm(F.conv3d(vol, w0.double(), None, 1, PAD), mu, var, g, b, False, 0.0, eb.BN_EPS))


def ratio(got, ref, E):
    """err / E per element: 0 where both are 0, inf where only E is (or got is not finite)."""
    err = (got.detach().cpu().double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))


# ---- emulation -----------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _axis32(f, shift, size, contract, lo=0, hi=None):
    """warp_point's float32 arithmetic along one axis at the integer coordinates lo .. hi - 1 (beyond the plane for the footprint's halo):
    (flow, position), each (B, N, hi - lo) float32; f, shift (B, N) float32."""
    hi = size if hi is None else hi
    one, den = torch.tensor(1.0), torch.tensor(float(size - 1 if size > 1 else 1))
    step = torch.tensor(2.0) / den
    i = torch.arange(lo, hi)
    i_f, r_f = i.float(), (size - 1 - i).float()
    if contract:
        lin = torch.where(i < size // 2, _fma(i_f, step, -one), _fma(-r_f, step, one))
    else:
        lin = torch.where(i < size // 2, -one + i_f * step, one - r_f * step)
    a = (torch.tensor(float(size // 2)) * (f - one)).unsqueeze(-1)
    flow = _fma(a, lin, shift.unsqueeze(-1)) if contract else a * lin + shift.unsqueeze(-1)
    g = torch.tensor(2.0) * (i_f - flow) / den - one
    return flow, ((g + one) * torch.tensor(0.5)) * torch.tensor(float(size - 1))


def _sample32(planes, sx, sy, contract, fault=None):
    """warp_octet: planes (B, N, C, H, W) float32 (joined records) at float32 positions sx, sy (B, N, H, W)."""
    B, N, C, H, W = planes.shape
    pp = F.pad(planes, (P4, P4, P4, P4))
    x0f, y0f = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = (sx - x0f).unsqueeze(2), (sy - y0f).unsqueeze(2)
    one = torch.tensor(1.0)
    wx, wy = (one - wx1, wx1), (one - wy1, wy1)
    x0, y0 = x0f.clamp(-3, W + 1).long(), y0f.clamp(-3, H + 1).long()
    v = torch.zeros(B, N, C, *sx.shape[2:])
    for dy in (0, 1):
        for dx in (0, 1):
            yc, xc = y0 + dy, x0 + dx
            c = _gather(pp, yc + P4, xc + P4)
            if fault == "xc_eq_w":       # xc == W accepted: the address is the first pixel of the next row (nothing behind the last row here)
                wrap = ((xc == W) & (yc >= 0) & (yc < H - 1)).unsqueeze(2)
                c = torch.where(wrap, _gather(pp, (yc + 1).clamp(max=H - 1) + P4, torch.zeros_like(xc) + P4), c)
            wgt = wx[dx] * wy[dy]
            v = _fma(c, wgt, v) if contract else v + c * wgt
    return v


def _conv_emu(x, w, bn, prec, relu, store, res=None, zero_shift=False, pad=PAD):
    """One 1x3x3 conv in the arithmetic: BN folded in fp32, operands split, fp32 accumulation, fp32 shift (+ the stored residual), ReLU."""
    s, t = eb.fold_bn(bn, w.shape[0])
    ws = (w.double() * s.reshape(-1, 1, 1, 1, 1)).float()
    t = torch.zeros_like(t).float() if zero_shift else t.float()
    xh, xl = _split(x, prec)
    wh, wl = _split(ws, prec)
    acc = F.conv3d(xh, wh, None, 1, pad)
    if prec == "bf16x3":
        acc = acc + (F.conv3d(xh, wl, None, 1, pad) + F.conv3d(xl, wh, None, 1, pad))
    y = acc + t.reshape(1, -1, 1, 1, 1)
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    return records(y, prec) if store else y


def emulate_volume(fe, alpha, fov, prec, contract, fault=None, halo=False):
    """The conv's input [ref | cur | flow] as float32 records (B, 2C+2, N, H, W); with ``halo`` one pixel wider on every side, the halo zero
    (what every form leaves there) -- or, with the fault "flow_outside", holding the flow of the positions outside the image."""
    x = records(fe, prec)
    B, C, N, H, W = x.shape
    a = alpha.float()
    a0 = a[:, 0]
    f = a0 + fov.float()
    if fault == "alpha0_ref":           # the reference slice's scale offset with the current slice's field of view
        f = a0[:, N - 1:].expand(B, N) + fov.float()
        f[:, N - 1] = a0[:, N - 1] + fov.float()[:, N - 1]
    a1, a2 = a[:, 1], a[:, 2]
    planes = x.permute(0, 2, 1, 3, 4)
    h = 1 if halo else 0
    fx, sx = _axis32(f, a1, W, contract, -h, W + h)
    fy, sy = _axis32(f, a2, H, contract, -h, H + h)
    full = lambda t, ax: (t.unsqueeze(2) if ax == "x" else t.unsqueeze(3)).expand(B, N, H + 2 * h, W + 2 * h)
    inner = lambda t: t[:, :, h:h + H, h:h + W]
    sxi, syi = inner(full(sx, "x")), inner(full(sy, "y"))
    cur = _sample32(planes, sxi, syi, contract, fault)
    ref = cur[:, 0 if fault == "ref_slice0" else N - 1]              # (slice 0 with slice 0's own parameters)
    if fault == "ref_neighbour_sample":
        ref = torch.roll(ref, 1, 0)
    flow = torch.stack([full(fx, "x"), full(fy, "y")], 2)             # (B, N, 2, H + 2h, W + 2h)
    if fault == "next_slice_params":      # slice N-1 sampled with the parameters of the step issued ahead (the next column's slice 0): positions and flow
        cur = cur.clone()
        cur[:, N - 1] = _sample32(planes[:, N - 1:], sxi[:, :1], syi[:, :1], contract)[:, 0]
        flow[:, N - 1] = flow[:, 0]
    if fault == "lo_dropped":
        cur = _split(cur, prec)[0]
    if fault == "flow_swapped":
        flow = flow.flip(2)
    if halo and fault != "flow_outside":
        keep = torch.zeros(H + 2, W + 2)
        keep[1:-1, 1:-1] = 1.0
        flow = flow * keep
    feat = torch.cat([ref.unsqueeze(1).expand(B, N, C, H, W), cur], 2)
    feat = F.pad(feat, (h, h, h, h))
    return records(torch.cat([feat, flow], 2).permute(0, 2, 1, 3, 4).contiguous(), prec)


def emulate(fe, w0, bn0, alpha, fov, prec, form, contract=False, fault=None, vol=None):
    """y0 float32 (B, 2C, N, H, W) as the form's kernels give it; ``fault``: one of FAULTS (see can_act); ``vol``: a precomputed clean
    emulate_volume (the same for every form)."""
    B, C, N, H, W = fe.shape
    halo = fault == "flow_outside"
    if vol is None or fault is not None:
        vol = emulate_volume(fe, alpha, fov, prec, contract, fault, halo)
    pad = (0, 0, 0) if halo else PAD

    def conv(v):
        if form == "whole":
            return _conv_emu(v, w0, bn0, prec, True, True, pad=pad)
        refpart = _conv_emu(v[:, :C, :1], w0[:, :C], bn0, prec, False, True, zero_shift=True, pad=pad)
        return _conv_emu(v[:, C:], w0[:, C:], bn0, prec, True, True, res=refpart, pad=pad)

    y = conv(vol)
    if fault == "next_column_sample" and B > 1 and N > 0:
        # the first column of a sample, slice 0, gathered while the unit still names the previous sample: its features and its parameters
        bad = emulate_volume(torch.roll(fe, 1, 0), torch.roll(alpha, 1, 0), torch.roll(fov, 1, 0), prec, contract)
        mixed = vol.clone()
        mixed[1:, C:, 0] = bad[1:, C:, 0]
        yb = conv(mixed)
        y = y.clone()
        y[1:, :, 0, :8, :16] = yb[1:, :, 0, :8, :16]
    return y


def forms_of(C, B, N, H, W):
    """The forms a shape can take: the warp form on whole 8 x 16 columns of an 8- or 16-channel level with at most 320 planes."""
    warp = C in (8, 16) and H % 8 == 0 and W % 16 == 0 and B * N <= WARP_MAX_PLANES
    return FORMS if warp else FORMS[1:]


def can_act(fault, form, prec, B, N):
    """Whether a fault changes anything in a form (the CPU test names a case for every fault): the step issued ahead and the footprint's halo
    exist in head_warp_kernel alone, a neighbouring sample needs two, another slice needs two, a lo half exists in split-bf16."""
    if fault in ("next_slice_params", "alpha0_ref", "ref_slice0") and N < 2:
        return False
    if fault in ("next_column_sample", "ref_neighbour_sample") and B < 2:
        return False
    if fault in ("next_slice_params", "next_column_sample", "flow_outside"):
        return form == "warp"
    if fault == "lo_dropped":
        return prec == "bf16x3"
    return True


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
WARPS = ("identity", "integer", "outside", "fractional", "f14", "f06", "mixed")
FEATURES = eb.REGIMES + ("smooth", "placed")


def warp_params(kind, B, N, H, W, seed):
    """(alpha (B,3,N), fov (B,N)) float32 of a regime, distinct per sample and slice (as far as the regime leaves a choice)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(B * N, dtype=torch.float32).reshape(B, N)
    rnd = lambda: torch.rand(B, N, generator=g) * 2 - 1
    fov = 0.875 + (k % 17) / 64.0                                    # dyadic: alpha0 + fov is exact where alpha0 is
    f = torch.ones(B, N)
    if kind == "identity":
        a1 = a2 = torch.zeros(B, N)
    elif kind == "integer":
        steps = torch.tensor([1.0, -1.0, 3.0, -3.0])
        a1, a2 = steps[(k.long()) % 4], steps[(k.long() // 4 + k.long()) % 4]
    elif kind == "outside":
        a1 = (W + (k % 5)) * torch.where(k % 2 == 0, 1.0, -1.0)
        a2 = (k % 3) - 1.0
    elif kind == "fractional":
        a1, a2 = 2.5 * rnd(), 2.5 * rnd()
    elif kind in ("f14", "f06"):
        f = (1.4 if kind == "f14" else 0.6) + 0.02 * rnd()
        a1, a2 = 0.75 * rnd(), 0.75 * rnd()
    else:
        f = 1.0 + 0.3 * rnd()
        a1, a2 = 3.0 * rnd(), 3.0 * rnd()
    alpha = torch.stack([f - fov, a1, a2], 1).float().contiguous()
    return alpha, fov.contiguous()


def places(H, W):
    p = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)]
    return list(dict.fromkeys(p))


def features(kind, shape, seed):
    B, C, N, H, W = shape
    if kind in eb.REGIMES:
        return eb.regime_input(kind, shape, seed)
    if kind == "placed":       # one 1.0 per (b, n, channel) plane, every plane at another place (cycling)
        x = torch.zeros(shape)
        pl = places(H, W)
        for b in range(B):
            for n in range(N):
                for c in range(C):
                    y, xx = pl[((b * N + n) * C + c) % len(pl)]
                    x[b, c, n, y, xx] = 1.0
        return x
    yy = torch.arange(H, dtype=torch.float64).reshape(1, 1, 1, H, 1) / H
    xx = torch.arange(W, dtype=torch.float64).reshape(1, 1, 1, 1, W) / W
    c = torch.arange(C, dtype=torch.float64).reshape(1, C, 1, 1, 1)
    n = torch.arange(N, dtype=torch.float64).reshape(1, 1, N, 1, 1)
    b = torch.arange(B, dtype=torch.float64).reshape(B, 1, 1, 1, 1)
    v = 0.6 + 0.4 * torch.sin(2 * math.pi * (yy * (1 + c % 3) + 0.37 * c + 0.11 * n + 0.23 * b)) * torch.cos(2 * math.pi * (xx * (1 + c % 2) + 0.19 * c))
    return v.float()


def front_params(kind, C, seed):
    """(w0 (2C, 2C+2, 1, 3, 3), bn0) in a regime of eb.REGIMES, eb-style."""
    g = torch.Generator().manual_seed(seed)
    bn0 = eb.bn_regime(kind, 2 * C, seed + 1)
    w0 = eb._block_weight((2 * C, 2 * C + 2, 1, 3, 3), 9 * (2 * C + 2), g, bn0)
    if kind == "offset":      # the BN centred on what the features' common offset 3 gives
        bn0 = eb.bn_regime(kind, 2 * C, seed + 1, conv_mean=3.0 * float(w0[:, :2 * C].double().sum() / (2 * C)))
    return w0, bn0


# the shapes of tests/test_gpu_head_front.py: (C, (B, N, H, W), DFFW_SRD_WGS)
SHAPES = [(C, s, wgs) for C in (8, 16) for s, wgs in (((1, 1, 8, 16), 0), ((1, 2, 8, 32), 0), ((2, 3, 24, 48), 0), ((3, 10, 16, 96), 8), ((32, 10, 8, 16), 0),
                                                         ((33, 10, 8, 16), 0), ((1, 3, 20, 24), 0))] + [(32, (1, 2, 8, 8), 0), (32, (2, 3, 12, 20), 0)]


def case(i, j):
    """Case j (0 .. len(WARPS) - 1) of SHAPES[i]: warp regime j with feature regime (i + j) % len(FEATURES): (fe, (w0, bn0), alpha, fov, name)."""
    C, (B, N, H, W), _ = SHAPES[i]
    wk, fk = WARPS[j], FEATURES[(i + j) % len(FEATURES)]
    fe = features(fk, (B, C, N, H, W), 1000 + 10 * i + j)
    alpha, fov = warp_params(wk, B, N, H, W, 2000 + 10 * i + j)
    return fe, front_params(fk if fk in eb.REGIMES else "post_relu", C, 3000 + 10 * i + j), alpha, fov, "C%d %s %s/%s" % (C, (B, N, H, W), wk, fk)


# ---- fov_warp_kernel (dffw_op_fov_warp) --------------------------------------------------------------------------------------------------------
# out[b,c,n] = the sample of x[b,c] at (s, slice coordinate); flow = (flow_x, flow_y).  The kernel computes the slice coordinate as
# ((2 n / (N - 1) - 1 + 1) / 2) (N - 1) in float32 and blends across slices where it falls short of n; the float64 reference samples slice n.
# dsz = u (4 n + (N - 1) / 2) (the division, the sum g + 1 and the last product: u n each; q - 1: u (n + (N - 1) / 2)), Lz = the largest
# difference between slice n and slices n - 1 and n + 1 (zero beyond the volume) over the 4 x 4 pixels of the reference's cell and its
# neighbours (a sample of the difference is a mean of its corners, wherever inside that window the kernel's position falls):
#     E_out = FOV_CAL_FACTOR ((1 + K3 u) (Lx dsx + Ly dsy) + Lz dsz + K3 u A),   E_flow = FOV_CAL_FACTOR dflow.
# x stays float32: no records.  The instantiation with 64-bit offsets needs a volume of 4 GiB per (sample, channel) and is not covered.
class FovRef:
    pass


def fov_reference(x, alpha, fov, compat_batch_alpha0=False, factor=FOV_CAL_FACTOR):
    B, C, N, H, W = x.shape
    geo = Geometry(alpha.reshape(B, 3, N), fov.reshape(B, N), H, W, compat_batch_alpha0)
    planes = x.double().permute(0, 2, 1, 3, 4)
    v, A, Lx, Ly = sample64(planes, geo)
    zero = torch.zeros_like(planes[:, :1])
    below, above = torch.cat([zero, planes[:, :-1]], 1), torch.cat([planes[:, 1:], zero], 1)
    Lz = window_max(torch.maximum((below - planes).abs(), (above - planes).abs()), geo)
    n = torch.arange(N, dtype=torch.float64).reshape(1, N, 1, 1, 1)
    dsz = U * (4.0 * n + (N - 1) / 2.0) if N > 1 else torch.zeros_like(n)
    out = FovRef()
    out.out = v.permute(0, 2, 1, 3, 4)
    out.flow = torch.stack([geo.full(geo.fx), geo.full(geo.fy)], 1)
    out.E_out = factor * (_input_error(A, Lx, Ly, geo, K_BLEND3) + Lz * dsz).permute(0, 2, 1, 3, 4)
    out.E_flow = factor * torch.stack([geo.full(geo.dfx), geo.full(geo.dfy)], 1)
    return out


def fov_emulate(x, alpha, fov, compat_batch_alpha0=False, contract=False):
    """(out, flow) float32 as fov_warp_kernel computes them: the in-plane weights as above, the slice weights from the float32 slice
    coordinate, the (dz, dy, dx) order, slices of zero weight skipped."""
    B, C, N, H, W = x.shape
    a = alpha.reshape(B, 3, N).float()
    a0 = a[:1, 0].expand(B, N) if compat_batch_alpha0 else a[:, 0]
    f = a0 + fov.reshape(B, N).float()
    fx, sx = _axis32(f, a[:, 1], W, contract)
    fy, sy = _axis32(f, a[:, 2], H, contract)
    fx, sx = (t.unsqueeze(2).expand(B, N, H, W) for t in (fx, sx))
    fy, sy = (t.unsqueeze(3).expand(B, N, H, W) for t in (fy, sy))
    one, den = torch.tensor(1.0), torch.tensor(float(N - 1 if N > 1 else 1))
    nf = torch.arange(N).float()
    sz = (((torch.tensor(2.0) * nf / den - one) + one) * torch.tensor(0.5)) * torch.tensor(float(N - 1))
    z0f = torch.floor(sz)
    wz1 = sz - z0f
    wz = (one - wz1, wz1)
    planes = F.pad(x.float().permute(0, 2, 1, 3, 4), (P4, P4, P4, P4))
    x0f, y0f = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = (sx - x0f).unsqueeze(2), (sy - y0f).unsqueeze(2)
    wx, wy = (one - wx1, wx1), (one - wy1, wy1)
    x0, y0 = x0f.clamp(-3, W + 1).long(), y0f.clamp(-3, H + 1).long()
    v = torch.zeros(B, N, C, H, W)
    for dz in (0, 1):
        zz = z0f.long() + dz
        ok = ((zz >= 0) & (zz < N) & (wz[dz] != 0)).float().reshape(1, N, 1, 1, 1)
        src = planes[:, zz.clamp(0, N - 1)] * ok
        for dy in (0, 1):
            for dx in (0, 1):
                c = _gather(src, y0 + dy + P4, x0 + dx + P4)
                wgt = wx[dx] * wy[dy] * wz[dz].reshape(1, N, 1, 1, 1)
                v = _fma(c, wgt, v) if contract else v + c * wgt
    return v.permute(0, 2, 1, 3, 4).contiguous(), torch.stack([fx, fy], 1).contiguous()


# the cases of the GPU test: (B, C, N, H, W), compat_batch_alpha0
FOV_SHAPES = [((1, 3, n, 8, 16), False) for n in (1, 2, 3, 10, 15)] + [((2, 8, 10, 12, 20), False), ((1, 3, 3, 1, 16), False), ((1, 3, 3, 8, 1), False),
                                                                         ((2, 3, 10, 8, 16), True)]


def fov_case(i, j):
    """Case j of FOV_SHAPES[i]: warp regime j on a random / smooth / placed stack (cycling): (x, alpha, fov, compat, name)."""
    (B, C, N, H, W), compat = FOV_SHAPES[i]
    kind = ("trained_bn", "smooth", "placed", "constant")[(i + j) % 4]
    x = features(kind, (B, C, N, H, W), 4000 + 10 * i + j)
    alpha, fov = warp_params(WARPS[j], B, N, H, W, 5000 + 10 * i + j)
    return x, alpha, fov, compat, "%s %s/%s%s" % ((B, C, N, H, W), WARPS[j], kind, " compat" if compat else "")
