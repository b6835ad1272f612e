#!/usr/bin/env python3
"""Golden vectors for the focal-stack simulator: what the reference's own Simulator/synthetic_blur_movement.py writes for one
frame.

The module is executed unmodified, top-level statement by top-level statement, in a namespace where its data and I/O
dependencies are stand-ins injected through sys.modules:
  mat73.loadmat   seeded frames (sim_ref.golden_frame) already at working size plus the 16-pixel border the script crops
                  (224 x 352 after the crop)
  cv2             resize: identity that asserts the size; circle: the filled-disk restatement; filter2D: exact
                  float64 correlation with BORDER_REFLECT_101, round half to even, saturate; cvtColor: channel reversal;
                  imwrite: captured
  scipy.io        savemat: captured
  random          randint picks the camera branch; normalvariate draws from a seeded random.Random
  tqdm            pass-through
FOV_warp is wrapped after its definition so that every warped float image is recorded (the tap golden).  The run happens in a
temporary directory and ends at the script's exit() after the first frame.  The four camera presets are read from the branch
assignments and stored in the fixtures, with the argparse defaults: they are reference data and live only here.
Fixture contents: the seeds (the frame is regenerated from them), the blurred uint8 slices in full (as x-differences modulo 256,
sim_ref.dx_decode), the shifts and FoVs the warps received, SHA-256 digests of every warped float slice, defocus slice and the
output depth with their first rows in full, the recorded scalars, the last slice's layer table and the camera presets.

Run here only (the reference does not exist on the test machines):
    python tools/make_goldens_sim.py   ->   tests/golden/sim_cam{0..3}_n{N}.npz
"""
import ast
import hashlib
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference/Simulator/synthetic_blur_movement.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
HEIGHT, WIDTH = 224, 352
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sim_ref  # noqa: E402  (disk_rows: the restated cv2.circle fill)


class Cv2:
    COLOR_BGR2RGB = 4

    def __init__(self):
        self.written = {}

    def resize(self, a, size):
        assert a.shape[1] == size[0] and a.shape[0] == size[1], (a.shape, size)
        return a

    def circle(self, img, center, radius, color, thickness):
        assert thickness < 0 and center == (radius, radius)
        for dy, hw in enumerate(sim_ref.disk_rows(radius)):
            for yy in {radius - dy, radius + dy}:
                img[yy, radius - hw:radius + hw + 1] = color[0]
        return img

    def filter2D(self, src, ddepth, kernel):
        assert ddepth == -1 and src.dtype == np.uint8
        kh, kw = kernel.shape
        ry, rx = kh // 2, kw // 2
        H, W = src.shape[:2]
        pad = src[sim_ref.reflect101(np.arange(-ry, H + ry), H)][:, sim_ref.reflect101(np.arange(-rx, W + rx), W)].astype(np.float64)
        acc = np.zeros(src.shape, np.float64)
        for dy in range(kh):
            for dx in range(kw):
                if kernel[dy, dx] != 0:
                    acc += kernel[dy, dx] * pad[dy:dy + H, dx:dx + W]
        return np.clip(np.rint(acc), 0, 255).astype(np.uint8)

    def cvtColor(self, img, code):
        assert code == self.COLOR_BGR2RGB
        return img[..., ::-1].copy()

    def imwrite(self, path, img):
        self.written[os.path.basename(path)] = img.copy()
        return True


def presets():
    """The four camera branches' assignments, evaluated with width = 352."""
    tree = ast.parse(open(REF).read())
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and getattr(node.test.left, "id", "") == "random_choice_devices":
            k = node.test.comparators[0].value
            vals = {}
            for st in node.body:
                if isinstance(st, ast.Assign):
                    vals[st.targets[0].id] = eval(compile(ast.Expression(st.value), REF, "eval"), {"width": WIDTH})
            out[k] = vals
    assert sorted(out) == [0, 1, 2, 3], out
    return out


def run(cam, N, seed, draw_seed):
    cv2 = Cv2()
    saved = {}
    img, dep = sim_ref.golden_frame(seed, HEIGHT + 32, WIDTH + 32)
    img, dep = img[..., None], dep[..., None]
    draws = []
    rnd = __import__("random").Random(draw_seed)

    def normalvariate(mu, sigma):
        v = rnd.normalvariate(mu, sigma)
        draws.append(v)
        return v

    mods = {
        "cv2": cv2,
        "mat73": types.SimpleNamespace(loadmat=lambda p: {"images": img, "depths": dep}),
        "scipy": types.SimpleNamespace(),
        "scipy.io": types.SimpleNamespace(savemat=lambda p, d: saved.__setitem__(os.path.basename(p), {k: np.array(v) for k, v in d.items()})),
        "random": types.SimpleNamespace(randint=lambda a, b: cam, normalvariate=normalvariate),
        "tqdm": types.SimpleNamespace(tqdm=lambda it, **k: it),
    }
    mods["scipy"].io = mods["scipy.io"]
    old_mods = {k: sys.modules.get(k) for k in mods}
    old_argv, old_cwd = sys.argv, os.getcwd()
    taps = []
    tree = ast.parse(open(REF).read())
    ns = {"__name__": "__sim__"}
    try:
        sys.modules.update(mods)
        sys.argv = ["synthetic_blur_movement.py", "--num_imgs", str(N)]
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                for st in tree.body:
                    exec(compile(ast.Module([st], []), REF, "exec"), ns)
                    if isinstance(st, ast.FunctionDef) and st.name == "FOV_warp":
                        inner = ns["FOV_warp"]

                        def wrapped(x, Fov, beta, gamma, inner=inner):
                            o = inner(x, Fov, beta, gamma)
                            taps.append((np.array(o), float(Fov), float(beta), float(gamma)))
                            return o
                        ns["FOV_warp"] = wrapped
            except SystemExit:
                pass
    finally:
        os.chdir(old_cwd)
        sys.argv = old_argv
        for k, v in old_mods.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    args = ns["args"]
    images = np.stack([cv2.written[f"img{n}.png"] for n in range(N)])
    image0 = img[16:-16, 16:-16, :, 0].astype(np.float32)
    warped = np.stack([image0] + [t[0] for t in taps]).astype(np.float32)
    discard = "depth.mat" not in saved
    g = dict(cam=cam, N=N, seed=seed, draw_seed=draw_seed, H=HEIGHT, W=WIDTH, images_dx=sim_ref.dx_encode(images), shifts=np.array([[0.0, 0.0]] + [[t[2], t[3]] for t in taps]), fov=np.array([1.0] + [t[1] for t in taps]),
             draws=np.array(draws), status=np.int32(discard),
             warped_sha=np.array([hashlib.sha256(np.ascontiguousarray(w).tobytes()).hexdigest() for w in warped]),
             warped_band=warped[:, :2].copy(), ppm=args.pixel_vs_meter, num_planes=args.num_planes, min_depth=args.min_depth,
             max_depth=args.max_depth, min_focus=ns["min_focus_dist"], max_focus=ns["max_focus_dist"])
    if not discard:
        defocus = np.moveaxis(saved["depth.mat"]["defocus"], 2, 0)
        depth_out = saved["depth.mat"]["depth"].astype(np.float32)
        g.update(depth_out_sha=hashlib.sha256(np.ascontiguousarray(depth_out).tobytes()).hexdigest(), depth_out_band=depth_out[:8].copy(),
                 defocus_sha=np.array([hashlib.sha256(np.ascontiguousarray(d).tobytes()).hexdigest() for d in defocus]),
                 defocus_band=defocus[:, :2].copy(),
                 camera_setting=np.array([float(np.squeeze(saved["camera_param.mat"][k])) for k in
                                          ("focal_length", "aperture_size", "pixel_mm", "max_focus_dist", "min_focus_dist")]))
    # recorded scalars: focus distances and the per-slice values of the loop, from the namespace after the last slice
    g["focus_dists"] = np.array(ns["focus_dists"])
    g["origin_max_AFOV"] = float(ns["origin_max_AFOV"])
    g["min_AFOV"], g["max_AFOV"] = float(ns["min_AFOV"]), float(ns["max_AFOV"])
    last = ns["coc_min_max_dis"]
    g["last_table"] = np.array([[c, lo, hi] for c, lo, hi in last], np.float64)
    return g


def main():
    os.makedirs(OUT, exist_ok=True)
    pre = presets()
    cases = [(c, 10, 100 + c, 200 + c) for c in range(4)] + [(1, 5, 105, 205)]
    for cam, N, seed, dseed in cases:
        g = run(cam, N, seed, dseed)
        p = pre[cam]
        g["preset"] = np.array([p["focal_length"], p["F_num"], p["alpha_slope"], p["y_intercept"], p["beta_mean"], p["beta_var"],
                                p["gamma_mean"], p["gamma_var"], p["size_ratio"]])
        path = os.path.join(OUT, f"sim_cam{cam}_n{N}.npz")
        np.savez_compressed(path, **g)
        print(path, os.path.getsize(path), "status", int(g["status"]))


if __name__ == "__main__":
    main()
