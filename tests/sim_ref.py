"""Independent CPU restatement of the synthetic focal-stack simulator (Simulator/synthetic_blur_movement.py:155-280), the
oracle of the GPU simulator (dffw_sim_render) at any size and batch.  DESIGN.md §10 states the contract.

The structure is the reference's (whole-image blur per CoC layer, then the layer masks), the arithmetic is the one each of its
steps has: Python float64 scalars, the warp through torch CPU float32 ops and grid_sample, the disk blur as an exact integer sum
over reflect-101 padding rounded to nearest.  tests/test_sim.py checks it bit for bit against the goldens recorded from the
reference's own module (tools/make_goldens_sim.py)."""
import numpy as np
import torch
import torch.nn.functional as F


def plan(cam, scene_min, scene_max, N, ppm, focus_range, num_planes):
    """Per-slice float64 scalars (dict of lists) and CoC layer tables [[coc, lo, hi], ...] per slice."""
    fl, fnum, slope, icpt = (float(v) for v in cam)
    min_fd, max_fd = (float(v) for v in focus_range)
    ppm = float(ppm)
    f = fl * ppm
    lens_dia = f / fnum
    fds = 1 / np.linspace(1 / max_fd, 1 / min_fd, N, endpoint=True)
    max_fd_px, min_fd_px = max_fd * ppm, min_fd * ppm
    min_afov = 1 / (f * min_fd_px / (min_fd_px - f))
    max_afov = 1 / (f * max_fd_px / (max_fd_px - f))
    origin_max_afov = max_afov / min_afov + slope * (1 / scene_max) + icpt
    out = {k: [] for k in ("fd", "fd_px", "lens_to_sensor", "fov", "coc_scale")}
    tables = []
    for n in range(N):
        fd = fds[n]
        fd_px = ppm * fd
        lts = f * fd_px / (fd_px - f)
        fov = 1.0
        if n:
            fov = origin_max_afov / ((1 / lts) / min_afov + (slope * (1 / fd) + icpt))
        coc_scale = lts * lens_dia / fd_px
        for k, v in zip(out, (fd, fd_px, lts, fov, coc_scale)):
            out[k].append(float(v))
        layers = []
        span = scene_max - scene_min
        for k in range(num_planes):
            lo = k / num_planes * span + scene_min
            hi = (k + 1) / num_planes * span + scene_min
            c = round(coc_scale * ((lo + (hi - lo) / 2) - fd) / (lo + (hi - lo) / 2))
            if k and hi == scene_max:
                hi += 0.1
            if k and layers[-1][0] == c:
                layers[-1][2] = hi
            else:
                layers.append([int(c), lo, hi])
        tables.append(layers)
    out.update(f_px=f, lens_dia=lens_dia, min_afov=min_afov, max_afov=max_afov, origin_max_afov=origin_max_afov,
               scene_min=scene_min, scene_max=scene_max)
    return out, tables


def disk_rows(r):
    """Row half-widths 0..r of cv2.circle(zeros, (r,r), r, 1, -1): the midpoint fill as DESIGN.md restates it, as a table of
    the widest fill of every row."""
    hw = [-1] * (r + 1)
    dx, dy, err, plus, minus = r, 0, 0, 1, 2 * r - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def reflect101(p, n):
    """cv2.borderInterpolate(p, n, BORDER_REFLECT_101), vectorised, any p."""
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    t = 2 * (n - 1)
    m = np.mod(p, t)
    return np.where(m < n, m, t - m)


def disk_blur(u8, r):
    """filter2D(u8, -1, disk(r)/K) with BORDER_REFLECT_101 as exact integer sums rounded to nearest (K odd: no ties)."""
    H, W, C = u8.shape
    hw = disk_rows(r)
    K = sum((2 * h + 1) * (1 if y == 0 else 2) for y, h in enumerate(hw))
    ys = reflect101(np.arange(-r, H + r), H)
    xs = reflect101(np.arange(-r, W + r), W)
    pad = u8[ys][:, xs].astype(np.int64)
    pre = np.zeros((H + 2 * r, W + 2 * r + 1, C), np.int64)
    pre[:, 1:] = np.cumsum(pad, axis=1)
    S = np.zeros((H, W, C), np.int64)
    cols = np.arange(W) + r
    for dy in range(-r, r + 1):
        h = hw[abs(dy)]
        rows = pre[r + dy:r + dy + H]
        S += rows[:, cols + h + 1] - rows[:, cols - h]
    return ((2 * S + K) // (2 * K)).astype(np.uint8)


def warp(x, fov, beta, gamma):
    """The simulator's FOV warp of x (H,W) or (H,W,C) float32 on the torch CPU: the grid in the reference's operation order
    ((W//2)*((FoV-1)*linspace) - beta, float32), grid_sample bilinear, zero padding, align_corners=True."""
    a = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    a = a[None, None] if a.dim() == 2 else a.permute(2, 0, 1)[None]
    H, W = a.shape[-2:]
    lx = torch.linspace(-1, 1, steps=W)[None, :].expand(H, W)
    ly = torch.linspace(-1, 1, steps=H)[:, None].expand(H, W)
    s = float(fov) - 1   # float64, a wrapped scalar to torch
    b = torch.from_numpy(np.asarray(float(beta)))
    g = torch.from_numpy(np.asarray(float(gamma)))
    fx = (W // 2) * (s * lx) - b
    fy = (H // 2) * (s * ly) - g
    px = torch.arange(W).float()[None, :].expand(H, W) - fx
    py = torch.arange(H).float()[:, None].expand(H, W) - fy
    grid = torch.stack((2.0 * px / max(W - 1, 1) - 1.0, 2.0 * py / max(H - 1, 1) - 1.0), dim=-1)[None].float()
    out = F.grid_sample(a, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
    return out[0].numpy() if np.ndim(x) == 2 else out.permute(1, 2, 0).numpy()


def render_one(image, depth, cam, shifts, N, ppm, depth_range, focus_range, num_planes):
    """One frame: image float32 (H,W,3) 0..255, raw depth float64 (H,W), cam (focal m, F, slope, intercept), shifts (N,2).
    Returns dict(images uint8 (N,H,W,3), defocus float64 (N,H,W), depth float32 (H,W), warped float32 (N,H,W,3), discard,
    scalars, tables)."""
    min_depth, max_depth = depth_range
    d = max_depth * (depth - np.min(depth)) / (np.max(depth) - np.min(depth)) + min_depth
    smin, smax = float(np.min(d)), float(np.max(d))
    sc, tables = plan(cam, smin, smax, N, ppm, focus_range, num_planes)
    dpx = d * ppm
    H, W = d.shape
    images = np.zeros((N, H, W, 3), np.uint8)
    defocus = np.zeros((N, H, W), np.float64)
    warped = np.zeros((N, H, W, 3), np.float32)
    img = image.astype(np.float32)
    for n in range(N):
        fd_px = np.float64(sc["fd_px"][n])
        if n:
            w = warp(img, sc["fov"][n], shifts[n][0], shifts[n][1])
            dpn = warp(dpx, sc["fov"][n], shifts[n][0], shifts[n][1])
        else:
            w, dpn = img, dpx
        warped[n] = w
        defocus[n] = np.abs(sc["coc_scale"][n] * (dpn - fd_px) / dpn)   # NumPy 2: float64 for the float32 warp too
        u8 = w.astype(np.uint8)
        out = np.zeros((H, W, 3), np.uint8)
        for c, lo, hi in tables[n]:
            m = (d >= lo) & (d < hi)
            if m.any():
                out[m] = disk_blur(u8, max(1, abs(c)))[m]
        images[n] = out[..., ::-1]
    dout = warp(d.astype(np.float32), sc["fov"][N - 1], shifts[N - 1][0], shifts[N - 1][1])
    return dict(images=images, defocus=defocus, depth=dout.astype(np.float32), warped=warped, discard=bool(np.min(dout) == 0),
                scalars=sc, tables=tables)


def render(image, depth, cams, shifts, ppm, depth_range, focus_range, num_planes):
    """Batch of render_one: image (B,H,W,3), depth (B,H,W), cams (B,4), shifts (B,N,2)."""
    res = [render_one(image[b], depth[b], cams[b], shifts[b], shifts.shape[1], ppm, depth_range, focus_range, num_planes)
           for b in range(image.shape[0])]
    out = {k: np.stack([r[k] for r in res]) for k in ("images", "defocus", "depth", "warped")}
    out["status"] = np.array([int(r["discard"]) for r in res], np.int32)
    out["runs"] = res
    return out


def case_inputs(seed, B, H, W, *, plateau=0.0):
    """Seeded RGB-D frames: integer-valued float32 images (as decoded 8-bit frames), smooth positive depth with texture.
    plateau > 0 clips that fraction of the depth range so that many pixels sit exactly at the maximum."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    imgs, deps = [], []
    for b in range(B):
        ph = rng.random(4) * 6.0
        base = (np.sin(3 * x + ph[0]) + np.cos(5 * y + ph[1])) * 60 + 128
        img = base[..., None] + rng.normal(0, 40, (H, W, 3))
        imgs.append(np.clip(np.floor(img), 0, 255).astype(np.float32))
        dep = 0.7 + 2.5 * (x * (0.5 + ph[2] / 12) + y * y) + 0.3 * np.sin(9 * x + ph[3]) + rng.random((H, W)) * 0.05
        if plateau:
            dep = np.minimum(dep, dep.max() - plateau * (dep.max() - dep.min()))
        deps.append(dep.astype(np.float64))
    return np.stack(imgs), np.stack(deps)


def golden_frame(seed, h, w):
    """The frame of the golden fixtures (tools/make_goldens_sim.py): (h,w,3) uint8 image and (h,w) float64 depth, smooth (so
    the fixtures compress) with some texture."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    ph = rng.random(6) * 6
    img = np.stack([128 + 90 * np.sin(4 * x + ph[c]) * np.cos(3 * y + ph[c + 3]) + 20 * ((np.floor(x * 24) + np.floor(y * 16)) % 2)
                    for c in range(3)], -1)
    img = np.clip(np.floor(img), 0, 255).astype(np.uint8)
    dep = 1.0 + 3.0 * (x * (0.4 + ph[0] / 10) + y * y) + 0.4 * np.sin(7 * x + ph[1]) + 0.02 * rng.random((h, w))
    return img, dep


def dx_encode(u8):
    """uint8 array -> differences along the second-to-last axis modulo 256 (lossless; compresses well for smooth images)."""
    d = u8.astype(np.int16)
    d[..., 1:, :] -= u8[..., :-1, :].astype(np.int16)
    return (d % 256).astype(np.uint8)


def dx_decode(d):
    return (np.cumsum(d.astype(np.int64), axis=-2) % 256).astype(np.uint8)
