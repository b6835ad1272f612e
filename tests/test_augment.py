"""CPU: the training-sample assembly contract.  The restatement tests/augment_ref.py against the goldens made from
the reference's own loader classes (tools/make_goldens_augment.py), train_seeds against the recorded draws, and the argument
checks of pipeline.augment_stack that need no device."""
import glob
import os
import random

import numpy as np
import pytest
import torch

import augment_ref

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aug_*.npz")))
SEED_KEYS = ("contrast", "brightness", "gamma", "flip_x", "flip_y", "angle")


def golden_case(path):
    """-> (npz, keyword arguments shared by augment_ref.augment_one and the GPU call, per-sample seeds dict)"""
    g = np.load(path)
    raw = g["raw"].astype(np.float32) if int(g["raw_f32"]) else g["raw"]
    rng = None if np.isnan(g["gt_range"]).all() else tuple(None if np.isinf(v) else float(v) for v in g["gt_range"])
    kw = dict(raw=raw, layout=str(g["layout"]), size=tuple(int(v) for v in g["size"]), norm64=bool(g["norm64"]), gt=g["gt_src"],
              conf=g["conf_src"] if "conf_src" in g.files else None, gt_range=rng, sentinel=float(g["sentinel"]))
    seeds = {k: g[k].tolist() for k in SEED_KEYS}
    seeds["crop"] = [tuple(int(v) for v in c) for c in g["crop"]]
    return g, kw, seeds


def test_the_five_loader_fixtures_are_there():
    assert [os.path.basename(p) for p in GOLDEN] == ["aug_ddff.npz", "aug_flyingthings.npz", "aug_fs6.npz", "aug_hci.npz", "aug_smartphone.npz"]
    poses, flags = set(), set()
    for p in GOLDEN:
        _, _, s = golden_case(p)
        for b in range(len(s["angle"])):
            poses.add(augment_ref.pose(np.arange(6).reshape(2, 3), s["flip_x"][b], s["flip_y"][b], s["angle"][b], 0, 1).tobytes() + bytes([s["angle"][b] & 1]))
            flags.add(s["gamma"][b] < 1)
            flags.add("off" if s["flip_x"][b] <= 0.5 and s["flip_y"][b] <= 0.5 else "on")
    assert len(poses) == 8 and flags == {True, False, "off", "on"}


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_restatement_matches_reference_golden(path):
    g, kw, seeds = golden_case(path)
    raw = kw.pop("raw")
    for b in range(len(seeds["angle"])):
        out = augment_ref.augment_one(raw, kw["layout"], *(seeds[k][b] for k in SEED_KEYS), origin=seeds["crop"][b], size=kw["size"],
                                      norm64=kw["norm64"], gt=kw["gt"], conf=kw["conf"], gt_range=kw["gt_range"], sentinel=kw["sentinel"])
        augment_ref.check_fs(out[0], g["FS"][b], seeds["gamma"][b] == 1, kw["norm64"], f"{os.path.basename(path)}[{b}]")
        ref_gt = g["gt_unscaled"][b] if "gt_unscaled" in g.files else g["gt"][b]
        assert out[1].dtype == np.float32 and np.array_equal(out[1].view(np.uint32), ref_gt.view(np.uint32))
        assert out[2].dtype == np.bool_ and np.array_equal(out[2], g["mask"][b])
        if kw["conf"] is not None:
            assert np.array_equal(out[3].view(np.uint32), g["conf"][b].view(np.uint32))


def test_ddff_gt_rescale_is_the_callers_line():
    """The DDFF loader alone rescales gt by its focus range after the mask (float32 array minus a float64 scalar: float64).  The
    caller keeps that line; applied in float64 torch to the restatement's gt it equals what the loader returned, exactly."""
    g, kw, seeds = golden_case([p for p in GOLDEN if p.endswith("aug_ddff.npz")][0])
    lo, hi = float(g["min_dist"]), float(g["max_dist"])
    for b in range(len(seeds["angle"])):
        gt, mask = augment_ref.labels(kw["gt"], seeds["flip_x"][b], seeds["flip_y"][b], seeds["angle"][b], seeds["crop"][b], kw["size"])
        scaled = (torch.from_numpy(gt).double() - lo) / (hi - lo)
        assert g["gt"].dtype == np.float64 and torch.equal(scaled, torch.from_numpy(g["gt"][b]))
        assert np.array_equal(mask, g["mask"][b])


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_train_seeds_reproduces_recorded_draws(path):
    from dffinthewild_amd.pipeline import train_seeds
    g, _, seeds = golden_case(path)
    cropping = None if int(g["cropping"][0]) < 0 else tuple(int(v) for v in g["cropping"])
    mine = train_seeds(random.Random(int(g["random_seed"])), len(seeds["angle"]), cropping)
    for k in SEED_KEYS:
        assert mine[k] == seeds[k], k
    if cropping is None:
        assert "crop" not in mine
    else:
        assert [tuple(c) for c in mine["crop"]] == seeds["crop"]
    assert all(isinstance(v, int) and 0 <= v <= 3 for v in mine["angle"])


@pytest.mark.parametrize("norm64", [False, True], ids=["f32", "f64"])
def test_exhaustive_byte_values_and_poses_gamma_one(norm64):
    """All 256 byte values x 3 channels x 16 (flip_x, flip_y, angle) combinations = the eight poses twice, gamma == 1: the restatement is
    bit-identical to the chain written out here in plain NumPy on a 16 x 16 x 3 x 2 array (uint8 -> float64 arithmetic, float32 array
    -> float32 arithmetic, as the loaders hold their sources)."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    src = np.stack([np.stack([v, v[::-1], v.T], axis=2), np.stack([v.T, v, v[:, ::-1]], axis=2)], axis=3)      # (16,16,3,2) HWCN
    k = 0
    for contrast, brightness in ((1.0, 0.0), (1.57, 0.093), (0.41, -0.1), (1.6, -0.07)):
        for fx in (0.2, 0.9):
            for fy in (0.5, 0.51):
                for angle in range(4):
                    x = src if norm64 else src.astype(np.float32)
                    x = x / 255
                    x = (0.5 + contrast * (x - 0.5)) + brightness
                    x = np.maximum(np.minimum(x, 1.0), 0)
                    x = np.power(x, 1.0)
                    x = np.maximum(np.minimum(x, 1.0), 0)
                    x = x / 0.5 - 1.0
                    assert x.dtype == (np.float64 if norm64 else np.float32)
                    if fx > 0.5:
                        x = np.flip(x, 1)
                    if fy > 0.5:
                        x = np.flip(x, 0)
                    x = np.rot90(x, angle, axes=(0, 1))
                    want = torch.Tensor(np.transpose(x, (2, 3, 0, 1)).copy()).numpy()
                    got = augment_ref.augment_one(src, "HWCN", contrast, brightness, 1.0, fx, fy, angle, norm64=norm64)
                    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (contrast, fx, fy, angle)
                    k += 1
    assert k == 64


def test_identity_parameters_equal_the_test_loaders_normalisation():
    """contrast 1, brightness 0, gamma 1: the chain equals v/127.5 - 1 (pack_stack's arithmetic) for all 256 byte values, in both chains"""
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(augment_ref.photometric(v, 1.0, 0.0, 1.0, False), v.astype(np.float32) / np.float32(127.5) - np.float32(1.0))
    assert np.array_equal(augment_ref.photometric(v, 1.0, 0.0, 1.0, True), (v / 127.5 - 1.0).astype(np.float32))


def test_augment_stack_argument_errors_without_gpu(lib_built):
    from dffinthewild_amd import pipeline
    ident = dict(contrast=1.0, brightness=0.0, gamma=1.0, flip_x=0, flip_y=0, angle=0)
    raw = torch.zeros(2, 4, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipeline.augment_stack(raw, "NHWC", **ident)
    with pytest.raises(ValueError, match="layout"):
        pipeline.augment_stack(raw, "CHWN", **ident)
    with pytest.raises(ValueError, match="norm"):
        pipeline.augment_stack(raw, "NHWC", norm="f16", **ident)
    with pytest.raises(TypeError):
        pipeline.augment_stack(raw, "NHWC")                 # the seeds are required keywords


def test_c_abi_rejects_bad_arguments_without_gpu(lib_built):
    from dffinthewild_amd import engine
    import ctypes
    st = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)
    assert engine.lib.dffw_augment_stack(0, None, 0, st, 1, 1, 8, 8, 8, 8, None, 0, None, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None) == -1
    assert b"null" in engine.lib.dffw_last_error()
    one = ctypes.c_void_p(8)                                 # never dereferenced: the window check comes first
    assert engine.lib.dffw_augment_stack(0, one, 0, st, 1, 1, 8, 8, 9, 8, one, 0, one, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None) == -1
    assert b"window" in engine.lib.dffw_last_error()
    assert engine.lib.dffw_augment_stack(0, one, 7, st, 1, 1, 8, 8, 8, 8, one, 0, one, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None) == -1
    assert b"dtype" in engine.lib.dffw_last_error()
