"""Training-sample assembly on the GPU (pipeline.augment_stack -> dffw_augment_stack): against the goldens made from the reference's
loader classes and against the CPU restatement tests/augment_ref.py at other shapes, batches, layouts and strides.  Bounds as in
DESIGN.md §11: labels, geometry and FS with gamma == 1 bit-exact; FS otherwise within 2^-22, float64 chain with at most 1 element in
10^4 differing at all."""
import os
import random

import numpy as np
import pytest
import torch

import augment_ref
from test_augment import GOLDEN, SEED_KEYS, golden_case

pytestmark = pytest.mark.gpu

STACK_KERNELS = {(torch.uint8, "f32"): "dffw::augment_stack<u8,f32>", (torch.uint8, "f64"): "dffw::augment_stack<u8,f64>",
                 (torch.float32, "f32"): "dffw::augment_stack<f32,f32>", (torch.float32, "f64"): "dffw::augment_stack<f32,f64>"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(raw_t, layout, seeds, **kw):
    from dffinthewild_amd import engine, pipeline
    out = pipeline.augment_stack(raw_t, layout, **seeds, **kw)
    torch.cuda.synchronize()
    names = engine.op_kernels()
    out = out if isinstance(out, tuple) else (out,)
    return [o.cpu().numpy() for o in out], names


def compare(got, ref, seeds, norm64, what):
    """per sample: FS within the contract's bounds, labels bit-exact"""
    assert len(got) == len(ref)
    for b in range(ref[0].shape[0]):
        augment_ref.check_fs(got[0][b], ref[0][b], seeds["gamma"][b] == 1, norm64, f"{what}[{b}]")
    for a, r in zip(got[1:], ref[1:]):
        assert a.shape == r.shape and a.dtype == r.dtype, (what, a.shape, r.shape, a.dtype, r.dtype)
        assert np.array_equal(bits(a), bits(r)), what


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_gpu_augment_matches_reference_goldens(lib_built, path):
    g, kw, seeds = golden_case(path)
    S = len(seeds["angle"])
    raw = torch.from_numpy(kw["raw"]).cuda().unsqueeze(0).expand(S, *kw["raw"].shape)        # one decoded source, S samples: batch stride 0
    gt = torch.from_numpy(kw["gt"]).cuda().unsqueeze(0).expand(S, -1, -1)
    conf = None if kw["conf"] is None else torch.from_numpy(kw["conf"]).cuda().unsqueeze(0).expand(S, -1, -1)
    got, names = run(raw, kw["layout"], seeds, size=kw["size"], norm="f64" if kw["norm64"] else "f32", gt=gt, conf=conf,
                     gt_range=kw["gt_range"], sentinel=kw["sentinel"])
    ref_gt = g["gt_unscaled"] if "gt_unscaled" in g.files else g["gt"]
    ref = [g["FS"], ref_gt, g["mask"]] + ([g["conf"]] if conf is not None else [])
    compare(got, ref, seeds, kw["norm64"], os.path.basename(path))
    assert names == [STACK_KERNELS[(raw.dtype, "f64" if kw["norm64"] else "f32")], "dffw::augment_labels"]
    if "gt_unscaled" in g.files:   # DDFF: the loader's own rescale stays with the caller, in float64 torch
        lo, hi = float(g["min_dist"]), float(g["max_dist"])
        assert torch.equal((torch.from_numpy(got[1]).double() - lo) / (hi - lo), torch.from_numpy(g["gt"]))


def draw(seed, B, cropping=None, **fixed):
    from dffinthewild_amd.pipeline import train_seeds
    s = train_seeds(random.Random(seed), B, cropping)
    for k, v in fixed.items():
        s[k] = list(v) if isinstance(v, (list, tuple)) else [v] * B
    return s


def view_of_larger(src, layout):
    """the source as a non-contiguous view: the interior of a buffer larger along both image axes"""
    ay, ax = (1 + a for a in augment_ref.LAYOUTS[layout][1:3])
    shape = list(src.shape)
    shape[ay] += 5
    shape[ax] += 7
    big = torch.full(shape, 201, dtype=src.dtype, device="cuda")
    idx = [slice(None)] * src.dim()
    idx[ay], idx[ax] = slice(2, 2 + src.shape[ay]), slice(4, 4 + src.shape[ax])
    v = big[tuple(idx)]
    v.copy_(src)
    assert not v.is_contiguous()
    return v


def layout_shape(layout, B, N, H, W):
    dims = dict(zip(augment_ref.LAYOUTS[layout], (N, H, W, 3)))
    return (B,) + tuple(dims[a] for a in range(4))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("norm", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["NHWC", "HWCN", "HWNC"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32src"])
def test_gpu_augment_matches_restatement(lib_built, dtype, layout, norm, B):
    """square 61 x 61 window (not a multiple of the tile, nor of 4) cropped per sample from a 70 x 91 source that is itself a view of a
    larger buffer; per-sample distinct seeds, every pose mixed in one batch; gt with range rule and conf"""
    N, H, W, h = (15 if B == 1 else 1), 70, 91, 61
    seed = 1000 + 10 * B + len(layout) + (norm == "f64") + 2 * (dtype == np.uint8) + sum(map(ord, layout))
    src = augment_ref.source(layout_shape(layout, B, N, H, W), seed, dtype)
    seeds = draw(seed, B, (H - h, W - h))
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-0.5, 2.5, (B, H, W)).astype(np.float32)
    gt[:, ::7, ::5] = 0.0
    gt[:, 3, 4] = np.nan
    conf = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    kw = dict(size=(h, h), gt_range=(0.1, 2.0), sentinel=0.0)
    got, names = run(view_of_larger(torch.from_numpy(src).cuda(), layout), layout, seeds, norm=norm, gt=torch.from_numpy(gt).cuda(),
                     conf=torch.from_numpy(conf).cuda(), **kw)
    ref = augment_ref.augment(src, layout, seeds, norm64=norm == "f64", gt=gt, conf=conf, **kw)
    compare(got, ref, seeds, norm == "f64", f"{layout}-{norm}-B{B}")
    assert names == [STACK_KERNELS[(torch.from_numpy(src).dtype, norm)], "dffw::augment_labels"]


@pytest.mark.parametrize("angles", [(0, 2, 2, 0), (1, 3, 3, 1)], ids=["even", "odd"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32src"])
def test_gpu_augment_non_square_window(lib_built, dtype, angles):
    """60 x 83: neither a multiple of the 32 x 64 tile nor of the 4-pixel store; angles of one parity"""
    B, N, H, W, h, w = 4, 3, 77, 100, 60, 83
    src = augment_ref.source((B, N, H, W, 3), 5, dtype)
    seeds = draw(55, B, (H - h, W - w), angle=angles)
    gt = np.random.default_rng(5).normal(0, 1, (B, H, W)).astype(np.float32)
    got, _ = run(torch.from_numpy(src).cuda(), "NHWC", seeds, size=(h, w), gt=torch.from_numpy(gt).cuda(), sentinel=-3.0)
    assert got[0].shape == ((B, 3, N, w, h) if angles[0] & 1 else (B, 3, N, h, w))
    compare(got, augment_ref.augment(src, "NHWC", seeds, size=(h, w), gt=gt, sentinel=-3.0), seeds, False, "60x83")


def test_gpu_augment_every_pose_gamma_one_bit_exact(lib_built):
    """16 (flip_x, flip_y, angle) combinations in one batch, gamma == 1, no labels: FS bit-identical, FS alone returned"""
    B, N, H, W = 16, 2, 96, 96
    src = augment_ref.source((B, H, W, 3, N), 6)
    seeds = draw(6, B, gamma=1.0, flip_x=[b & 1 for b in range(B)], flip_y=[(b >> 1) & 1 for b in range(B)], angle=[b >> 2 for b in range(B)])
    for norm in ("f32", "f64"):
        (fs,), names = run(torch.from_numpy(src).cuda(), "HWCN", seeds, norm=norm)
        assert np.array_equal(bits(fs), bits(augment_ref.augment(src, "HWCN", seeds, norm64=norm == "f64")))
        assert names == [STACK_KERNELS[(torch.uint8, norm)]]


def test_gpu_augment_mixed_parity_and_window_errors(lib_built):
    from dffinthewild_amd import pipeline
    raw = torch.zeros((2, 3, 40, 48, 3), dtype=torch.uint8, device="cuda")
    ident = dict(contrast=1.0, brightness=0.0, gamma=1.0, flip_x=0, flip_y=0)
    with pytest.raises(ValueError, match="parity"):
        pipeline.augment_stack(raw, "NHWC", angle=[0, 1], **ident)
    assert pipeline.augment_stack(raw, "NHWC", angle=[0, 1], size=(40, 40), **ident).shape == (2, 3, 3, 40, 40)    # square: mixed is fine
    with pytest.raises(ValueError, match="does not fit"):
        pipeline.augment_stack(raw, "NHWC", angle=0, crop=(1, 0), **ident)
    with pytest.raises(ValueError, match="does not fit"):
        pipeline.augment_stack(raw, "NHWC", angle=0, size=(41, 48), **ident)
    with pytest.raises(ValueError, match="expected one value or 2"):
        pipeline.augment_stack(raw, "NHWC", angle=[0, 0, 0], **ident)
    with pytest.raises(ValueError, match="gt must be"):
        pipeline.augment_stack(raw, "NHWC", angle=0, gt=torch.zeros((2, 40, 40), device="cuda"), **ident)
    torch.cuda.synchronize()


@pytest.mark.parametrize("norm", ["f32", "f64"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32src"])
def test_gpu_augment_identity_equals_pack_stack(lib_built, dtype, norm):
    """contrast 1, brightness 0, gamma 1, no flip, angle 0 on a x32 window: bit-identical to pack_stack in both chains"""
    from dffinthewild_amd import pipeline
    B, N, H, W = 2, 5, 70, 110
    raw = torch.from_numpy(augment_ref.source((B, H, W, N, 3), 7)).cuda().to(dtype)
    a = pipeline.augment_stack(raw, "HWNC", contrast=1.0, brightness=0.0, gamma=1.0, flip_x=False, flip_y=False, angle=0, crop=(3, 9),
                               size=(64, 96), norm=norm)
    p = pipeline.pack_stack(raw, "HWNC", crop=(3, 9, 64, 96), norm=norm)
    assert a.shape == p.shape == (B, 3, N, 64, 96) and torch.equal(a.view(torch.int32), p.view(torch.int32))


def test_gpu_augment_repeatable_and_every_element_written(lib_built):
    """Two runs give the same bits, and no output element keeps what the allocator's block held before: a block of NaN bytes (0xFF)
    of each output's size is freed right before the call, so torch hands the poisoned memory to the wrapper's torch.empty."""
    B, N, H, W, h, w = 3, 4, 90, 120, 75, 101
    src = augment_ref.source((B, N, H, W, 3), 8)
    raw = torch.from_numpy(src).cuda()
    seeds = draw(8, B, (H - h, W - w), angle=[2, 0, 2])
    gt = np.random.default_rng(8).uniform(0.5, 1.5, (B, H, W)).astype(np.float32)
    gt_t = torch.from_numpy(gt).cuda()
    outs = []
    for _ in range(3):
        poison = [torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda") for n in (B * 3 * N * h * w * 4, B * h * w * 4, B * h * w, B * h * w * 4)]
        torch.cuda.synchronize()
        del poison
        got, _ = run(raw, "NHWC", seeds, size=(h, w), gt=gt_t, conf=gt_t)
        outs.append(got)
    for got in outs:
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and not np.isnan(got[3]).any()
        assert set(np.unique(got[2].view(np.uint8)).tolist()) <= {0, 1}
        for a, r in zip(got, outs[0]):
            assert np.array_equal(bits(a), bits(r))
    compare(outs[0], augment_ref.augment(src, "NHWC", seeds, size=(h, w), gt=gt, conf=gt), seeds, False, "poisoned")


def test_gpu_augment_sits_between_simulator_and_network(lib_built):
    """simulator.render -> augment_stack -> Network.forward: the simulator's uint8 stacks go in as they are; FS equals the restatement
    applied to the simulator's images and the forward returns finite maps of the augmented shape"""
    import sim_ref
    from test_gpu_sim import PHONE_A, PHONE_B, PPM
    from dffinthewild_amd import graph, pipeline, simulator, synth
    from dffinthewild_amd.Depth_Estimation_Network import Network
    B, N, H, W = 2, 5, 64, 96
    image, depth = sim_ref.case_inputs(11, B, H, W)
    cams = [simulator.Camera(*PHONE_A, beta_sigma=3.0, gamma_sigma=2.0, size_ratio=0.1), simulator.Camera(*PHONE_B)]
    sh = simulator.draw_shifts(cams, B, N, generator=torch.Generator().manual_seed(0))
    out = simulator.render(torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda(), cams, sh, N, PPM, (0.1, 1.0), (0.1, 0.9), 2000)
    seeds = draw(12, B, angle=[1, 3])
    FS, gt, mask = pipeline.augment_stack(out["images"], "NHWC", gt=out["depth"], **seeds)
    assert FS.shape == (B, 3, N, W, H) and gt.shape == mask.shape == (B, W, H) and mask.dtype == torch.bool
    ref = augment_ref.augment(out["images"].cpu().numpy(), "NHWC", seeds, gt=out["depth"].cpu().numpy())
    compare([FS.cpu().numpy(), gt.cpu().numpy(), mask.cpu().numpy()], ref, seeds, False, "sim")
    entries = list(graph.param_entries(graph.dff_net_convs()))
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(entries, seed=0).items()})
    net = net.cuda().eval()
    with torch.no_grad():
        maps = net(FS, out["focus_dists"].float()[:, :, None, None])
    assert maps[-1].shape == (B, W, H) and all(torch.isfinite(m).all() for m in maps)
