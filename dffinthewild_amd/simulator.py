"""Synthetic focal stacks on the GPU: the reference's simulator (Simulator/synthetic_blur_movement.py:155-280) as one call.

For a batch of RGB-D frames at working size, a camera per frame and N slices, ``render`` returns the blurred slices (uint8,
exactly the arrays the reference writes with imwrite), the defocus maps, the ground-truth depth warped with the last slice, the
per-slice focus distances and fields of view, and a status word per frame (bit 0: the reference would discard it).  All of it
runs in the HIP kernels of dffw_sim.hip; DESIGN.md §10 states the arithmetic contract.

The stack feeds the depth network directly (focus distances in metres, as End_to_End's loaders hand them over)::

    out = simulator.render(image, depth, cams, shifts, ...)
    mid, p1, p2, p3 = net.forward_raw(out["images"], out["focus_dists"].float()[:, :, None, None], layout="NHWC")

No camera presets ship here: construct ``Camera`` from your own calibration (INTEGRATION.md points at the reference's four).
"""
from dataclasses import dataclass

import torch

from . import engine


@dataclass(frozen=True)
class Camera:
    """One camera: lens focal length (metres), F-number, the linear focus-breathing model alpha = slope/fd + intercept of the
    field of view, and the normal distributions of the per-slice shifts (beta along x, gamma along y, in full-sensor pixels;
    ``size_ratio`` scales them to the working width)."""
    focal_length_m: float
    f_number: float
    alpha_slope: float
    alpha_intercept: float
    beta_mean: float = 0.0
    beta_sigma: float = 0.0
    gamma_mean: float = 0.0
    gamma_sigma: float = 0.0
    size_ratio: float = 1.0

    def lens(self):
        return (float(self.focal_length_m), float(self.f_number), float(self.alpha_slope), float(self.alpha_intercept))


def draw_shifts(cameras, B, N, generator=None):
    """(B,N,2) float64 CPU tensor of per-slice (beta, gamma): normal draws with each frame's camera statistics times its
    size ratio, as the reference draws them (:216-217); slice 0 is not warped and gets zeros."""
    cams = _per_frame(cameras, B)
    z = torch.randn((B, N, 2), dtype=torch.float64, generator=generator)
    out = torch.zeros((B, N, 2), dtype=torch.float64)
    for b, c in enumerate(cams):
        out[b, 1:, 0] = (z[b, 1:, 0] * c.beta_sigma + c.beta_mean) * c.size_ratio
        out[b, 1:, 1] = (z[b, 1:, 1] * c.gamma_sigma + c.gamma_mean) * c.size_ratio
    return out


def _per_frame(cameras, B):
    cams = [cameras] * B if isinstance(cameras, Camera) else list(cameras)
    if len(cams) != B or not all(isinstance(c, Camera) for c in cams):
        raise ValueError(f"need one Camera or a list of {B} Cameras")
    return cams


def max_radius(cameras, n_slices, pixel_per_meter, depth_range, focus_range, num_planes):
    """Upper bound of every blur radius these cameras give (host plan on a unit depth range, plus one for the data-dependent
    last bit of scene_max).  Selects the LDS or the global-memory render kernel; correctness does not depend on it."""
    p = engine.sim_params(pixel_per_meter, depth_range, focus_range, num_planes)
    r = 1
    for c in {c.lens() for c in cameras}:
        _, tables = engine.sim_plan_host(p, c, 0.0, 1.0, n_slices)
        r = max(r, max(int(abs(t[0]).max()) for t in tables) + 1)
    return r


def render(image, depth, cameras, shifts, n_slices, pixel_per_meter, depth_range, focus_range, num_planes, *, tap=False,
           workspace=None):
    """Simulate B focal stacks on the GPU.

    image     (B,H,W,3) float32 CUDA tensor, 0..255, channel order as cv2 reads it (BGR)
    depth     (B,H,W) float64 CUDA tensor, raw depth (normalised per frame to depth_range)
    cameras   one Camera or a list of B
    shifts    (B,N,2) float64 (beta, gamma) in working pixels, e.g. draw_shifts(...); slice 0's row is ignored
    n_slices  N (>= 2);  pixel_per_meter: sensor pixels per metre at working size
    depth_range (min_depth, max_depth): d' = max_depth*(d - min d)/(max d - min d) + min_depth
    focus_range (min_focus, max_focus) in metres;  num_planes: depth planes of the CoC layer table
    Returns a dict of CUDA tensors: images uint8 (B,N,H,W,3) RGB, defocus float64 (B,N,H,W), depth float32 (B,H,W),
    focus_dists float64 (B,N), fov float64 (B,N), status int32 (B); with ``tap`` also warped float32 (B,N,H,W,3)."""
    B, H, W, _ = image.shape
    cams = _per_frame(cameras, B)
    if tuple(shifts.shape) != (B, n_slices, 2):
        raise ValueError(f"shifts must be ({B}, {n_slices}, 2), got {tuple(shifts.shape)}")
    dev = image.device
    rmax = max_radius(cams, n_slices, pixel_per_meter, depth_range, focus_range, num_planes)
    p = engine.sim_params(pixel_per_meter, depth_range, focus_range, num_planes, max_radius=rmax)
    cam_t = torch.tensor([c.lens() for c in cams], dtype=torch.float64, device=dev)
    out = engine.op_sim_render(image, depth, cam_t, shifts.to(device=dev, dtype=torch.float64), p, tap=tap, workspace=workspace)
    sl = out.pop("slices")
    out["focus_dists"] = sl[..., 0]
    out["fov"] = sl[..., 1]
    return out
