"""Reference, bounds and a CPU emulation for the backward of a conv over a channel concatenation; shared by
tests/test_conv_cat_grad.py and tests/test_gpu_conv_cat_grad.py.  Everything is built on tests/conv_grad_ref.py: the geometry is its "k333".

Reference: ``cg.grads64`` (float64 autograd) on ``torch.cat([xa, xb], 1)``, grad_x split at Ca.

Bounds.  grad_w is the plain conv's weight gradient on the concatenation, so its bound is ``cg.wgrad_ref64(cat, gy).bound(prec)``:
``ALPHA[prec] * G`` plus the fp16 subnormal term.  grad_xa / grad_xb are adjoint convs of grad_y on the filter's slices ``w[:, :Ca]`` and
``w[:, Ca:]``, so theirs is ``cg.dgrad_ref64(slice, gy).bound(prec)``.  No constant of this file's own.

Emulation.  ``cat_fill`` restates the kernel's two-source footprint fill on the record tensors (flat 16-bit arrays, one 8-channel octet at a
time, each source at its own row pitch) and can plant the faults tests/test_conv_cat_grad.py names; ``cg.emulate_wgrad`` on what it yields is
dffw::conv_wgrad_cat_kernel + conv_wgrad_finish_kernel."""
import functools

import torch

import conv_grad_ref as cg
from oracle import error_bounds as eb

GEOM = "k333"
FAULTS = ("swapped", "switch_octet", "b_channel", "b_pitch")


def cat_case(regime, B, ca, cb, cout, N, H, W, seed, impulse_channel=None):
    """(xa, xb, w, gy) float32 CPU tensors: ``cg.make_case`` of the Ca + Cb -> Cout conv, its x split at Ca."""
    x, w, gy = cg.make_case(regime, GEOM, B, ca + cb, cout, N, H, W, seed, impulse_channel=impulse_channel)
    return x[:, :ca].contiguous(), x[:, ca:].contiguous(), w, gy


def refs64(xa, xb, w, gy):
    """(Ref64 of grad_xa, of grad_xb, of grad_w): the references are cg.grads64 on the concatenation, split at Ca; the scales are those of the two
    sliced adjoint convs and of the plain weight gradient."""
    ca = xa.shape[1]
    x = torch.cat([xa, xb], 1)
    gx, gw = cg.grads64(x, w, gy, GEOM)
    da, db = cg.dgrad_ref64(w[:, :ca].contiguous(), gy, GEOM), cg.dgrad_ref64(w[:, ca:].contiguous(), gy, GEOM)
    rw = cg.wgrad_ref64(x, gy, GEOM, tuple(w.shape))
    ra = eb.Ref64(gx[:, :ca].contiguous(), gx[:, :ca].contiguous(), da.D, da.sub)
    rb = eb.Ref64(gx[:, ca:].contiguous(), gx[:, ca:].contiguous(), db.D, db.sub)
    return ra, rb, eb.Ref64(gw, gw, rw.D, rw.sub)


@functools.lru_cache(maxsize=None)
def case(regime, ca, cb, cout, shape, channel=None):
    """One case and its three float64 references, computed once and shared by the precisions and the tests."""
    B, N, H, W = shape
    xa, xb, w, gy = cat_case(regime, B, ca, cb, cout, N, H, W, seed=23 + ca + 3 * cb + 7 * cout, impulse_channel=channel)
    return (xa, xb, w, gy) + refs64(xa, xb, w, gy)


def cat_fill(ra, rb, fault=None):
    """The records of the concatenation as conv_wgrad_cat_kernel's fill reads them.  ``ra`` [B,N,H,W,parts,Ca], ``rb`` [.., Cb] int16 records
    (cg.to_records).  Per pixel, part and octet (8 channels from ch = 8 * oct): below Ca the octet is a's, at ``pixel * parts * Ca + part * Ca +
    ch`` of a's flat array; below Ca + Cb it is b's, at ``pixel * parts * Cb + part * Cb + (ch - Ca)`` of b's.  A planted fault may index past a
    row or the array; the flat index then wraps, which is as wrong as anything else found there.
      swapped       the two sources exchanged (b first)
      switch_octet  the switch tested with <= : the octet at ch == Ca still read from a
      b_channel     b read at channel ch instead of ch - Ca
      b_pitch       b read with a's row pitch parts * Ca"""
    if fault == "swapped":
        ra, rb = rb, ra
    parts, ca, cb = ra.shape[4], ra.shape[5], rb.shape[5]
    fa, fb = ra.reshape(-1), rb.reshape(-1)
    npix = ra.numel() // (parts * ca)
    pixel = torch.arange(npix).reshape(-1, 1, 1)
    part = torch.arange(parts).reshape(1, -1, 1)
    lane = torch.arange(8).reshape(1, 1, -1)
    out = torch.zeros(npix, parts, ca + cb, dtype=torch.int16)
    for ch in range(0, ca + cb, 8):
        in_a = ch <= ca if fault == "switch_octet" else ch < ca
        if in_a:
            src, idx = fa, pixel * (parts * ca) + part * ca + ch + lane
        else:
            pitch = parts * (ca if fault == "b_pitch" else cb)
            src, idx = fb, pixel * pitch + part * cb + (ch if fault == "b_channel" else ch - ca) + lane
        out[:, :, ch:ch + 8] = src[idx % src.numel()]
    return out.reshape(tuple(ra.shape[:5]) + (ca + cb,))


def emulate_cat_wgrad(xa, xb, gy, prec, fault=None, **kw):
    """grad_w in the kernel's arithmetic: the two-source fill on the records of xa and xb, then cg.emulate_wgrad.  Without a fault the fill must
    yield the records of the concatenation bit for bit, and the emulation then runs on the concatenation itself.  With one it runs on the values
    the faulty fill read (hi + lo of a record is an fp32 value; cg.emulate_wgrad splits it again: into the same sum, at a rounding tie into other parts)."""
    filled = cat_fill(cg.to_records(xa, prec), cg.to_records(xb, prec), fault)
    x = torch.cat([xa, xb], 1)
    if fault is None:
        assert torch.equal(filled, cg.to_records(x, prec)), "the restated fill does not yield the concatenation's records"
    else:
        x = cg.from_records(filled, prec, x.shape[1])
    return cg.emulate_wgrad(x, gy, GEOM, prec, **kw)
