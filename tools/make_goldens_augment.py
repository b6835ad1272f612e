#!/usr/bin/env python3
"""Golden vectors for the training-sample assembly: what the REFERENCE's five training loaders return.

Same technique as oracle/make_goldens_pack.py.  `train_codes/train_Dataloader.py` cannot be imported (cv2 / h5py / OpenEXR / scipy
are absent, and `augmentation.py` needs skimage), but everything between the decode calls is plain NumPy / torch.  So this script
reads the two files where they lie, takes the five loader ClassDef nodes and the module-level DDFF_* FunctionDef nodes of the first
and the FunctionDef nodes the loaders call of the second, and compiles exactly those, unmodified, into a namespace whose DECODE
dependencies are stand-in data sources (`cv2.imread`, `h5py.File`, `listdir`, `open`, the OpenEXR depth reader).  `random` is seeded,
`__init__` and `__getitem__` run in train mode as the reference wrote them, and nothing of the reference's text is written into this
repository: the fixtures hold arrays only.  Two pieces of instrumentation record what passes by without changing it: `get_seeds`
(the seeds actually drawn) and the first augmentation call of each loader (the decoded source exactly as the loader holds it).

FlyingThings3d decodes 540 x 960 x 15 sources; to keep its fixture small the instance's `input_size` and the `cropping` derived
from it are set to a 300 x 340 source before `__getitem__` (the loader's code is untouched; only the random crop's range shrinks).
`np.int`, removed from NumPy 1.24+, is aliased to `int` while the Smartphone loader's `__init__` runs.

Every fixture holds two samples of one decoded source (two `__getitem__` calls on one seeded stream).  The seed of `random` is
picked per fixture by trying, so that between the fixtures all eight poses, a sample with both flips off, gamma below and above 1 and a
sample whose contrast / brightness saturate both clamps occur; the script asserts that coverage, that `pipeline.train_seeds`
reproduces the recorded draws, and that the CPU restatement tests/augment_ref.py meets the contract's bounds against the reference
(bit-exact labels; FS within 2^-22, float64-chain fixtures with at most 1 element in 10^4 differing).

The goldens record what the NumPy installed here computes (NEP 50 promotion), as DESIGN.md §10 says for the simulator.

Run where the reference is present (TEST INFRASTRUCTURE):
    python tools/make_goldens_augment.py [--check]   ->   tests/golden/aug_*.npz     (--check: compare with the committed files)
"""
import ast
import io
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref  # noqa: E402
from dffinthewild_amd.pipeline import train_seeds  # noqa: E402
from oracle.make_goldens_pack import FakeCv2, FakeOs, base_ns, image  # noqa: E402

REF_LOADER = "/root/reference/train_codes/train_Dataloader.py"
REF_AUG = "/root/reference/train_codes/augmentation.py"
OUT = os.path.join(ROOT, "tests", "golden")
LOADERS = ["FocalStackDDFFH5Reader", "FS6_dataset", "FlyingThings3d", "HCI_dataset", "Smartphone"]
AUG_FUNCS = ["image_augmentation", "horizontal_flip", "vertical_flip", "rotate", "randcrop_3d", "horizontal_flip_w_conf",
             "vertical_flip_w_conf", "rotate_w_conf", "randcrop_3d_w_conf"]
SAMPLES = 2
CHECK = "--check" in sys.argv


def namespace(**extra):
    ns = base_ns(isfile=lambda p: True, **extra)
    tree = ast.parse(open(REF_AUG).read(), REF_AUG)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in AUG_FUNCS]
    assert {n.name for n in keep} == set(AUG_FUNCS)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_AUG, "exec"), ns)
    tree = ast.parse(open(REF_LOADER).read(), REF_LOADER)
    keep = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name in LOADERS) or (isinstance(n, ast.FunctionDef) and n.name.startswith("DDFF_"))]
    assert {n.name for n in keep if isinstance(n, ast.ClassDef)} == set(LOADERS)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_LOADER, "exec"), ns)
    return ns


def record(ns, name, log):
    """passes the call through to the reference's function, keeping copies of its array arguments"""
    inner = ns[name]

    def outer(*args):
        log.append([np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args])
        return inner(*args)
    ns[name] = outer


def depth_map(h, w, tag, lo, hi, special):
    """(h,w) float32 'decoded depth': periodic (compresses), spans [lo, hi], and holds `special` exactly in places"""
    v = image(h, w, tag, plain=True)[:, :, 0].astype(np.float32)
    d = (lo + (hi - lo) * v / np.float32(255)).astype(np.float32)
    d[v % 17 == 0] = special
    return d


def pose_id(fx, fy, k):
    a = np.arange(6).reshape(2, 3)
    return augment_ref.pose(a, fx, fy, k, 0, 1).tobytes() + bytes([k & 1])


def coverage(seeds):
    out = set()
    for b in range(len(seeds["angle"])):
        c, br, g, fx, fy, k = (seeds[n][b] for n in ("contrast", "brightness", "gamma", "flip_x", "flip_y", "angle"))
        out.add(("pose", pose_id(fx, fy, k)))
        if fx <= 0.5 and fy <= 0.5:
            out.add("flips_off")
        out.add("gamma<1" if g < 1 else "gamma>1")
        if 0.5 - 0.5 * c + br < 0 and 0.5 + 0.5 * c + br > 1:
            out.add("both_clamps")
    return out


COVERED = set()


def pick_seed(cropping):
    """the seed of `random` whose SAMPLES draws add most to what the earlier fixtures cover"""
    best = max(range(400), key=lambda s: (len(coverage(train_seeds(random.Random(s), SAMPLES, cropping)) - COVERED), -s))
    COVERED.update(coverage(train_seeds(random.Random(best), SAMPLES, cropping)))
    return best


def run(name, ds, seed, cropping, fetch):
    """SAMPLES calls of the loader's __getitem__(0) on one seeded stream; returns the recorded seeds and the loader's outputs"""
    drawn = []
    inner = ds.get_seeds
    ds.get_seeds = lambda: drawn.append(inner()) or drawn[-1]
    random.seed(seed)
    with np.errstate(divide="ignore"):
        outs = [fetch(ds[0]) for _ in range(SAMPLES)]
    mine = train_seeds(random.Random(seed), SAMPLES, cropping)
    off = 0 if cropping is None else 2
    for b, d in enumerate(drawn):
        assert len(d) == 6 + off
        if cropping is not None:
            assert tuple(d[:2]) == tuple(mine["crop"][b])
        assert tuple(d[off:]) == tuple(mine[k][b] for k in ("contrast", "brightness", "gamma", "flip_x", "flip_y", "angle")), name
    return mine, outs


def save(name, seed, cropping, seeds, outs, raw, raw_f32, layout, norm64, size, gt_src, conf_src, gt_range, sentinel, **extra):
    FS = np.stack([np.asarray(o["FS"]) for o in outs])
    gt = np.stack([np.asarray(o["gt"]) for o in outs])
    mask = np.stack([np.asarray(o["mask"]) for o in outs])
    assert FS.dtype == np.float32 and mask.dtype == np.bool_
    arrays = dict(raw=raw, raw_f32=np.asarray(int(raw_f32)), layout=np.asarray(layout), norm64=np.asarray(int(norm64)), size=np.asarray(size),
                  gt_src=gt_src, gt_range=np.asarray([np.nan, np.nan] if gt_range is None else [-np.inf if v is None else v for v in gt_range]),
                  sentinel=np.asarray(float(sentinel)), random_seed=np.asarray(seed), cropping=np.asarray((-1, -1) if cropping is None else cropping),
                  crop=np.asarray(seeds.get("crop", [(0, 0)] * SAMPLES)), FS=FS, gt=gt, mask=mask, **extra)
    for k in ("contrast", "brightness", "gamma", "flip_x", "flip_y", "angle"):
        arrays[k] = np.asarray(seeds[k])
    if conf_src is not None:
        arrays["conf_src"] = conf_src
        arrays["conf"] = np.stack([np.asarray(o["conf"]) for o in outs])
    # the restatement against the reference, on the CPU, within the contract's bounds
    src = raw.astype(np.float32) if raw_f32 else raw
    for b in range(SAMPLES):
        r = augment_ref.augment_one(src, layout, *(seeds[k][b] for k in ("contrast", "brightness", "gamma", "flip_x", "flip_y", "angle")),
                                    origin=tuple(arrays["crop"][b]), size=tuple(size), norm64=norm64, gt=gt_src, conf=conf_src,
                                    gt_range=gt_range, sentinel=sentinel)
        augment_ref.check_fs(r[0], FS[b], seeds["gamma"][b] == 1, norm64, f"{name}[{b}] restatement vs reference")
        ref_gt = extra["gt_unscaled"][b] if "gt_unscaled" in extra else gt[b]
        assert r[1].dtype == np.float32 and np.array_equal(r[1], ref_gt, equal_nan=True) and np.array_equal(r[2], mask[b]), name
        if conf_src is not None:
            assert np.array_equal(r[3], arrays["conf"][b]), name
    p = os.path.join(OUT, f"aug_{name}.npz")
    if CHECK:
        old = np.load(p)
        assert sorted(old.files) == sorted(arrays), (name, old.files)
        worst = 0.0
        for k, v in arrays.items():
            a, v = old[k], np.asarray(v)
            assert a.shape == v.shape and a.dtype == v.dtype, (name, k)
            if v.dtype.kind == "f":
                worst = max(worst, float(np.nanmax(np.abs(np.where(np.isfinite(v), a - v, 0.0)), initial=0.0)))
                assert np.array_equal(a, v, equal_nan=True), (name, k)
            else:
                assert np.array_equal(a, v), (name, k)
        print(f"{name}: committed fixture equals the reference in place, max |d| = {worst}")
        return
    np.savez_compressed(p, **arrays)
    kb = os.path.getsize(p) / 1024
    print(f"{name}: seed {seed}, FS {FS.shape}, raw {raw.shape} {raw.dtype}, {kb:.0f} KiB")
    assert os.path.getsize(p) <= 1121075, "fixture larger than the largest one committed before"


def as_u8(x):
    """a float32 array of whole byte values, stored as uint8 (the test widens it again: exact)"""
    u = x.astype(np.uint8)
    assert np.array_equal(u.astype(x.dtype), x)
    return u


def ddff():
    # train_Dataloader.py:31-80: hdf5 stack (N,H,W,3) -> float32 chain; flips / rot90 on axes (2, 1, (1,2)); sentinel 0, no range;
    # gt rescaled by the focus range afterwards (the caller's line)
    stack = np.stack([image(224, 224, 60 + i, plain=True) for i in range(10)], axis=0)[None]
    disp = depth_map(224, 224, 5, 0.02, 0.28, 0.0)[None]
    log = []
    ns = namespace(h5py=type("H5", (), {"File": staticmethod(lambda p, m: {"stack_train": stack, "disp_train": disp})}))
    record(ns, "image_augmentation", log)
    ds = ns["FocalStackDDFFH5Reader"]("ddff.h5")
    seed = pick_seed(None)
    seeds, outs = run("ddff", ds, seed, None, lambda o: dict(FS=o[0].numpy(), gt=o[1].numpy(), mask=o[3].numpy()))
    assert log[0][0].dtype == np.float32 and outs[0]["gt"].dtype == np.float64
    lo, hi = float(ds.min_dist), float(ds.max_dist)
    unscaled = [(torch.from_numpy(o["gt"]) * (hi - lo) + lo) for o in outs]     # only to check the restatement's labels below
    gt_src = disp[0]
    r = [augment_ref.labels(gt_src, seeds["flip_x"][b], seeds["flip_y"][b], seeds["angle"][b], (0, 0), (224, 224))[0] for b in range(SAMPLES)]
    for b in range(SAMPLES):   # the loader's own rescale of the restatement's gt, in float64 torch, equals what it returned
        assert torch.equal((torch.from_numpy(r[b]).double() - lo) / (hi - lo), torch.from_numpy(outs[b]["gt"]))
        assert np.allclose(unscaled[b].numpy(), r[b], atol=1e-6)
    save("ddff", seed, None, seeds, outs, as_u8(log[0][0]), True, "NHWC", False, (224, 224), gt_src, None, None, 0.0,
         min_dist=np.asarray(lo), max_dist=np.asarray(hi), gt_unscaled=np.stack(r))


def fs6():
    # :81-141: five uint8 images concatenated onto a float64 array -> float64 chain; float16 depth; <0 or >2 -> 0
    root = "Datasets/fs_6/train/"
    names = [f"s{i:02d}All.tif" for i in range(5)]
    table = {root + n: image(256, 256, 70 + i, plain=True) for i, n in enumerate(names)}
    dpt = depth_map(256, 256, 6, -0.2, 2.4, 0.0).astype(np.float16)
    ns = namespace(cv2=FakeCv2(table), listdir=lambda p: names + ["s00Dpt.exr"])
    ds = ns["FS6_dataset"]("train")
    ds.read_dpt = lambda p: dpt.copy()                                           # the OpenEXR decode
    seed = pick_seed(None)
    seeds, outs = run("fs6", ds, seed, None, lambda o: dict(FS=o[0].numpy(), gt=o[1].numpy(), mask=o[3].numpy()))
    raw = np.stack([table[root + n] for n in names], axis=3)                     # (H,W,3,N)
    save("fs6", seed, None, seeds, outs, raw, False, "HWCN", True, (256, 256), dpt.astype(np.float32), None, (0.0, 2.0), 0.0)


def flyingthings():
    # :143-215: 15 uint8 images (H,W,3,15) -> crop -> float64 chain (x/255 on a uint8 array); depth < 0 -> 0
    H, W = 300, 340
    paths = [f"ft/im{i:02d}.png" for i in range(15)]
    table = {p: image(H, W, 80 + i, plain=True) for i, p in enumerate(paths)}
    table["ft/disp.exr"] = depth_map(H, W, 7, -5.0, 60.0, 0.0)
    listing = " ".join(paths + ["ft/disp.exr"]) + "\n"
    log = []
    ns = namespace(cv2=FakeCv2(table), os=FakeOs({}), open=lambda p, m="r": io.StringIO(listing))
    record(ns, "randcrop_3d", log)
    ds = ns["FlyingThings3d"]("train")
    ds.input_size = (H, W)
    ds.cropping = (H - ds.train_size[0], W - ds.train_size[1])
    seed = pick_seed(ds.cropping)
    seeds, outs = run("flyingthings", ds, seed, ds.cropping, lambda o: dict(FS=o[0].numpy(), gt=o[1].numpy(), mask=o[2].numpy()))
    assert log[0][0].dtype == np.uint8 and log[0][0].shape == (H, W, 3, 15)
    save("flyingthings", seed, ds.cropping, seeds, outs, log[0][0], False, "HWCN", True, ds.train_size, log[0][1], None, (0.0, None), 0.0)


def hci():
    # :216-268: hdf5 stack (10,512,512,3) -> float32 (512,512,3,10) -> crop 256 -> float32 chain; sentinel -3, no range
    stack = np.stack([image(512, 512, 90 + i, plain=True) for i in range(10)], axis=0)[None]
    disp = depth_map(512, 512, 8, -2.5, 2.5, -3.0)[None]
    h5 = {"stack_train": stack, "disp_train": disp, "focus_position_disp": np.linspace(-2.0, 2.0, 10, dtype=np.float32)[None]}
    log = []
    ns = namespace(h5py=type("H5", (), {"File": staticmethod(lambda p, m: h5)}))
    record(ns, "randcrop_3d", log)
    ds = ns["HCI_dataset"]("hci.h5")
    seed = pick_seed(ds.cropping)
    seeds, outs = run("hci", ds, seed, ds.cropping, lambda o: dict(FS=o[0].numpy(), gt=o[1].numpy(), mask=o[3].numpy()))
    assert log[0][0].dtype == np.float32 and log[0][0].shape == (512, 512, 3, 10)
    save("hci", seed, ds.cropping, seeds, outs, as_u8(log[0][0]), True, "HWCN", False, ds.size, log[0][1], None, None, -3.0)


def smartphone():
    # :269-379: 504x378 JPEGs, centre crop -> (336,252,N,3) float32 -> crop 224 -> float32 chain; gt outside [1/3.91092, 1/0.10201] -> 0; conf
    root = "Datasets/Real_data_DP/"
    idx = np.rint(np.linspace(0, 48, 10, endpoint=True)).astype(int)
    t1 = root + "train1/"
    table = {f"{t1}scaled_images/scene0/{j}/result_scaled_image_center.jpg": image(504, 378, 100 + k, plain=True) for k, j in enumerate(idx)}
    table[f"{t1}merged_depth/scene0/result_merged_depth_center.png"] = image(504, 378, 3, plain=True)[:, :, 0]
    table[f"{t1}merged_conf/scene0/result_merged_conf_center.exr"] = (image(504, 378, 4, plain=True) / 200.0).astype(np.float32)
    listing = {f"{root}train{i}/scaled_images/": (["scene0"] if i == 1 else []) for i in range(1, 8)}
    log = []
    ns = namespace(cv2=FakeCv2(table), os=FakeOs(listing))
    record(ns, "randcrop_3d_w_conf", log)
    np.int = int                                                                # removed alias the loader still uses (:278)
    try:
        ds = ns["Smartphone"]("train", 10)
    finally:
        del np.int
    seed = pick_seed(ds.cropping)
    seeds, outs = run("smartphone", ds, seed, ds.cropping,
                      lambda o: dict(FS=o[0].numpy(), gt=o[1].numpy(), mask=o[3].numpy(), conf=np.asarray(o[4])))
    x, gt_src, conf_src = log[0][:3]
    assert x.dtype == np.float32 and x.shape == (336, 252, 10, 3) and gt_src.dtype == conf_src.dtype == np.float32
    save("smartphone", seed, ds.cropping, seeds, outs, as_u8(x), True, "HWNC", False, ds.rand_crop, gt_src, conf_src,
         (ds.min_depth, ds.max_depth), 0.0)


if __name__ == "__main__":
    for f in (ddff, fs6, flyingthings, hci, smartphone):
        f()
    want = {("pose", pose_id(fx, fy, k)) for fx in (0, 1) for fy in (0, 1) for k in range(4)} | {"flips_off", "gamma<1", "gamma>1", "both_clamps"}
    assert len(want) == 12 and COVERED >= want, want - COVERED
    print("coverage: all eight poses, flips off, gamma below and above 1, both clamps saturated")
