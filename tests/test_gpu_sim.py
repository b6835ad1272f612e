"""Focal-stack simulator on the GPU (dffw_sim_render): bit-identical to the reference's goldens (tools/make_goldens_sim.py)
and to the CPU restatement tests/sim_ref.py at other sizes, batches, cameras and radii."""
import hashlib
import os

import numpy as np
import pytest
import torch

import sim_ref
from test_sim import GOLDEN, golden_case

pytestmark = pytest.mark.gpu

PPM = 61625.0
KW = dict(ppm=PPM, depth_range=(0.1, 1.0), focus_range=(0.1, 0.9), num_planes=2000)
# cameras for the restatement cases (not the reference's presets): focal length m, F-number, alpha slope, intercept
PHONE_A = (0.0046, 1.8, -0.003, 0.012)
PHONE_B = (0.0062, 1.6, -0.0041, 0.006)
PHONE_C = (0.0040, 2.0, -0.002, 0.018)
LONG_LENS = (0.016, 1.8, -0.003, 0.01)   # radii beyond the LDS halo


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gpu_render(image, depth, cams, shifts, kw, *, tap=True, max_radius=None, workspace=None):
    from dffinthewild_amd import engine, simulator
    B, N = shifts.shape[:2]
    cam_objs = [simulator.Camera(*c) for c in cams]
    rmax = max_radius if max_radius is not None else simulator.max_radius(cam_objs, N, kw["ppm"], kw["depth_range"], kw["focus_range"],
                                                                            kw["num_planes"])
    p = engine.sim_params(kw["ppm"], kw["depth_range"], kw["focus_range"], kw["num_planes"], max_radius=rmax)
    out = engine.op_sim_render(torch.from_numpy(np.ascontiguousarray(image, np.float32)).cuda(), torch.from_numpy(depth).cuda(),
                               torch.tensor(np.asarray(cams, np.float64)).cuda(), torch.from_numpy(np.asarray(shifts, np.float64)).cuda(),
                               p, tap=tap, workspace=workspace)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, engine.op_kernels()


def assert_same(got, ref):
    for k in ("images", "defocus", "depth", "warped", "status"):
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            diff = np.argwhere(a != b)
            raise AssertionError(f"{k}: {len(diff)} elements differ, first {diff[:3].tolist()}: {a[tuple(diff[0])]} vs {b[tuple(diff[0])]}")


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_gpu_sim_matches_reference_goldens(lib_built, path):
    g, (image, depth, cams, shifts), kw = golden_case(path)
    out, kernels = gpu_render(image, depth, cams, shifts, kw)
    N = int(g["N"])
    assert np.array_equal(out["images"][0], sim_ref.dx_decode(g["images_dx"]))
    assert [sha(out["warped"][0, n]) for n in range(N)] == list(g["warped_sha"])
    assert [sha(out["defocus"][0, n]) for n in range(N)] == list(g["defocus_sha"])
    assert sha(out["depth"][0]) == str(g["depth_out_sha"])
    assert int(out["status"][0]) == int(g["status"])
    assert np.array_equal(out["slices"][0, :, 0], g["focus_dists"]) and np.array_equal(out["slices"][0, 1:, 1], g["fov"][1:])
    assert kernels == ["dffw::sim_minmax", "dffw::sim_plan", "dffw::sim_render<true>"]


def _ref(image, depth, cams, shifts, kw):
    return sim_ref.render(image, depth, cams, shifts, **kw)


def _shifts(seed, B, N, scale=3.0):
    s = np.random.default_rng(seed).normal(0, scale, (B, N, 2))
    s[:, 0] = 0
    return s


@pytest.mark.parametrize("B,N,H,W,cams", [
    (3, 10, 96, 160, [PHONE_A, PHONE_B, PHONE_C]),
    (1, 5, 96, 160, [PHONE_B]),
    (2, 15, 75, 131, [PHONE_C, PHONE_A]),
], ids=["b3_mixed", "n5", "n15_odd"])
def test_gpu_sim_matches_restatement(lib_built, B, N, H, W, cams):
    image, depth = sim_ref.case_inputs(10 + N, B, H, W)
    sh = _shifts(N, B, N)
    out, kernels = gpu_render(image, depth, cams, sh, KW)
    assert_same(out, _ref(image, depth, np.asarray(cams), sh, KW))
    assert kernels[-1] == "dffw::sim_render<true>"


def test_gpu_sim_global_path(lib_built):
    """A lens whose blur radius exceeds the LDS halo: the global-memory kernel, same bits; the LDS kernel's per-tile fallback too."""
    B, N, H, W = 1, 4, 48, 80
    image, depth = sim_ref.case_inputs(5, B, H, W)
    sh = _shifts(5, B, N)
    ref = _ref(image, depth, np.asarray([LONG_LENS]), sh, KW)
    assert max(abs(c) for t in ref["runs"][0]["tables"] for c, _, _ in t) > 32
    out, kernels = gpu_render(image, depth, [LONG_LENS], sh, KW)
    assert kernels == ["dffw::sim_minmax", "dffw::sim_plan", "dffw::sim_render<false>"]
    assert_same(out, ref)
    out2, kernels2 = gpu_render(image, depth, [LONG_LENS], sh, KW, max_radius=1)   # a wrong hint costs speed only
    assert kernels2[-1] == "dffw::sim_render<true>"
    assert_same(out2, ref)


def test_gpu_sim_pixels_at_scene_max(lib_built):
    """A plateau at the maximum depth: with one plane the last edge is not extended and those pixels come out black."""
    B, N, H, W = 1, 5, 64, 96
    image, depth = sim_ref.case_inputs(7, B, H, W, plateau=0.2)
    sh = _shifts(7, B, N)
    for planes in (1, 2000):
        kw = dict(KW, num_planes=planes)
        ref = _ref(image, depth, np.asarray([PHONE_A]), sh, kw)
        out, _ = gpu_render(image, depth, [PHONE_A], sh, kw)
        assert_same(out, ref)
        at_max = depth[0] == depth[0].max()
        assert at_max.sum() > 100
        black = (out["images"][0][:, at_max] == 0).all()
        assert black == (planes == 1)


def test_gpu_sim_discard_bit(lib_built):
    B, N, H, W = 2, 5, 64, 96
    image, depth = sim_ref.case_inputs(8, B, H, W)
    sh = _shifts(8, B, N, scale=1.0)
    sh[1, -1] = (40.0, -30.0)    # the last slice's warp leaves the image: zeros in the output depth
    ref = _ref(image, depth, np.asarray([PHONE_B, PHONE_B]), sh, KW)
    out, _ = gpu_render(image, depth, [PHONE_B, PHONE_B], sh, KW)
    assert_same(out, ref)
    assert out["status"].tolist() == [0, 1]
    assert np.isinf(out["defocus"][1, -1]).any()


def test_gpu_sim_repeatable_and_poisoned_workspace(lib_built):
    from dffinthewild_amd import engine
    B, N, H, W = 2, 6, 70, 100
    image, depth = sim_ref.case_inputs(9, B, H, W)
    sh = _shifts(9, B, N)
    need = engine.sim_workspace_bytes(B, N, H, W, KW["num_planes"])
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        outs.append(gpu_render(image, depth, [PHONE_A, PHONE_C], sh, KW, workspace=ws)[0])
    for o in outs[1:]:
        for k in outs[0]:
            assert np.array_equal(outs[0][k].view(np.uint8), o[k].view(np.uint8)), k


def test_gpu_sim_feeds_forward_raw(lib_built):
    """The simulated stack goes straight into Network.forward_raw and equals forward(pack_stack(images))."""
    from dffinthewild_amd import graph, pipeline, simulator, synth
    from dffinthewild_amd.Depth_Estimation_Network import Network
    B, N, H, W = 2, 5, 64, 96
    image, depth = sim_ref.case_inputs(11, B, H, W)
    cams = [simulator.Camera(*PHONE_A, beta_sigma=3.0, gamma_sigma=2.0, size_ratio=0.1), simulator.Camera(*PHONE_B)]
    sh = simulator.draw_shifts(cams, B, N, generator=torch.Generator().manual_seed(0))
    out = simulator.render(torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda(), cams, sh, N, PPM, (0.1, 1.0), (0.1, 0.9), 2000)
    assert out["images"].shape == (B, N, H, W, 3) and out["focus_dists"].shape == (B, N)
    entries = list(graph.param_entries(graph.dff_net_convs()))
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(entries, seed=0).items()}
    net = Network()
    net.load_state_dict(sd)
    net = net.cuda().eval()
    fd = out["focus_dists"].float()[:, :, None, None]
    with torch.no_grad():
        a = net.forward_raw(out["images"], fd, layout="NHWC")
        b = net(pipeline.pack_stack(out["images"], "NHWC"), fd)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
