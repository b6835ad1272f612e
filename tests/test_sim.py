"""Focal-stack simulator, CPU side: the fixtures recorded from the reference's own simulator module (tools/make_goldens_sim.py),
the independent restatement tests/sim_ref.py against them bit for bit, and the library's host plan (dffw_sim_plan_host) and
disk table (dffw_sim_disk_rows) against both."""
import glob
import hashlib
import os

import numpy as np
import pytest

import sim_ref

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "sim_cam*_n*.npz")))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden_case(path):
    """(golden, inputs) with inputs = image (1,H,W,3) float32, depth (1,H,W), cams (1,4), shifts (1,N,2) and the settings."""
    g = np.load(path)
    img, dep = sim_ref.golden_frame(int(g["seed"]), int(g["H"]) + 32, int(g["W"]) + 32)
    image = img[16:-16, 16:-16].astype(np.float32)[None]
    depth = dep[16:-16, 16:-16].astype(np.float64)[None]
    cams = g["preset"][None, :4].astype(np.float64)
    shifts = g["shifts"][None].astype(np.float64)
    kw = dict(ppm=float(g["ppm"]), depth_range=(float(g["min_depth"]), float(g["max_depth"])),
              focus_range=(float(g["min_focus"]), float(g["max_focus"])), num_planes=int(g["num_planes"]))
    return g, (image, depth, cams, shifts), kw


def test_sim_goldens_cover_every_camera():
    cams = {int(np.load(p)["cam"]) for p in GOLDEN}
    Ns = {int(np.load(p)["N"]) for p in GOLDEN}
    assert cams == {0, 1, 2, 3} and 10 in Ns and len(Ns) >= 2
    for p in GOLDEN:
        assert os.path.getsize(p) < 1 << 20


@pytest.fixture(scope="module", params=GOLDEN, ids=os.path.basename)
def ref_run(request):
    g, (image, depth, cams, shifts), kw = golden_case(request.param)
    return g, sim_ref.render(image, depth, cams, shifts, **kw), kw


def test_sim_ref_matches_reference_images(ref_run):
    g, out, _ = ref_run
    assert np.array_equal(out["images"][0], sim_ref.dx_decode(g["images_dx"]))


def test_sim_ref_matches_reference_floats(ref_run):
    g, out, _ = ref_run
    N = int(g["N"])
    assert [sha(out["warped"][0, n]) for n in range(N)] == list(g["warped_sha"])
    assert np.array_equal(out["warped"][0, :, :2], g["warped_band"])
    assert int(out["status"][0]) == int(g["status"])
    assert [sha(out["defocus"][0, n]) for n in range(N)] == list(g["defocus_sha"])
    assert np.array_equal(out["defocus"][0, :, :2], g["defocus_band"])
    assert sha(out["depth"][0]) == str(g["depth_out_sha"])
    assert np.array_equal(out["depth"][0, :8], g["depth_out_band"])


def test_sim_ref_matches_reference_scalars(ref_run):
    g, out, _ = ref_run
    run = out["runs"][0]
    sc = run["scalars"]
    assert np.array_equal(np.array(sc["fd"]), g["focus_dists"])
    assert np.array_equal(np.array(sc["fov"][1:]), g["fov"][1:])
    assert (sc["min_afov"], sc["max_afov"], sc["origin_max_afov"]) == (float(g["min_AFOV"]), float(g["max_AFOV"]), float(g["origin_max_AFOV"]))
    assert np.array_equal(np.array(run["tables"][-1], np.float64), g["last_table"])
    cs = g["camera_setting"]   # focal length px, aperture, ppm, scene max, scene min
    assert (sc["f_px"], sc["lens_dia"], sc["scene_max"], sc["scene_min"]) == (cs[0], cs[1], cs[3], cs[4])


def _params(kw, **extra):
    from dffinthewild_amd import engine
    return engine.sim_params(kw["ppm"], kw["depth_range"], kw["focus_range"], kw["num_planes"], **extra)


def _host_vs_ref(params, cam, dmin, dmax, N, kw):
    from dffinthewild_amd import engine
    sc, tables = engine.sim_plan_host(params, cam, dmin, dmax, N)
    dr = kw["depth_range"]
    smin = dr[1] * (dmin - dmin) / (dmax - dmin) + dr[0]
    smax = dr[1] * (dmax - dmin) / (dmax - dmin) + dr[0]
    rsc, rt = sim_ref.plan(cam, smin, smax, N, kw["ppm"], kw["focus_range"], kw["num_planes"])
    names = engine.SIM_SCALARS
    for n in range(N):
        for k in ("fd", "fd_px", "lens_to_sensor", "fov", "coc_scale"):
            assert sc[n, names.index(k)] == rsc[k][n], (k, n)
        for k in ("f_px", "lens_dia", "scene_min", "scene_max", "min_afov", "max_afov", "origin_max_afov"):
            assert sc[n, names.index(k)] == rsc[k], (k, n)
        coc, lo, hi = tables[n]
        ref = np.array(rt[n], np.float64)
        assert np.array_equal(coc, ref[:, 0].astype(np.int32)) and np.array_equal(lo, ref[:, 1]) and np.array_equal(hi, ref[:, 2])
    return sc, tables


def test_sim_plan_host_matches_goldens(lib_built, ref_run):
    g, _, kw = ref_run
    _, (image, depth, cams, shifts), _ = golden_case(os.path.join(os.path.dirname(__file__), "golden", f"sim_cam{int(g['cam'])}_n{int(g['N'])}.npz"))
    N = int(g["N"])
    sc, tables = _host_vs_ref(_params(kw), cams[0], depth.min(), depth.max(), N, kw)
    from dffinthewild_amd import engine
    assert np.array_equal(sc[:, engine.SIM_SCALARS.index("fd")], g["focus_dists"])
    assert np.array_equal(sc[1:, engine.SIM_SCALARS.index("fov")], g["fov"][1:])
    coc, lo, hi = tables[-1]
    assert np.array_equal(np.stack([coc, lo, hi], 1), g["last_table"])


def test_sim_plan_host_last_edge_not_extended(lib_built):
    """The 0.1 extension is checked for planes k > 0 only, so with one plane the last edge stays at scene_max and pixels there
    fall in no layer.  (With more planes the last edge (smax - smin) + smin came out equal to scene_max in every case tried:
    scene_max is itself a rounded sum onto scene_min.)"""
    kw = dict(ppm=61625.0, depth_range=(0.1, 1.0), focus_range=(0.1, 0.9), num_planes=1)
    sc, tables = _host_vs_ref(_params(kw), (0.0048, 1.7, -0.004, 0.02), 0.5, 4.0, 6, kw)
    from dffinthewild_amd import engine
    smax = sc[0, engine.SIM_SCALARS.index("scene_max")]
    assert all(len(t[0]) == 1 and t[2][-1] == smax for t in tables)
    kw2 = dict(kw, num_planes=2000)
    _, t2 = _host_vs_ref(_params(kw2), (0.0048, 1.7, -0.004, 0.02), 0.5, 4.0, 6, kw2)
    assert all(t[2][-1] == smax + 0.1 for t in t2)


def test_sim_disk_rows_match_restatement(lib_built):
    from dffinthewild_amd import engine
    for r in range(0, 65):
        hw, K = engine.sim_disk_rows(r)
        assert hw == sim_ref.disk_rows(r), r
        assert K == sum((2 * h + 1) * (1 if y == 0 else 2) for y, h in enumerate(hw)) and K % 2 == 1
    assert engine.sim_disk_rows(1) == ([1, 0], 5) and engine.sim_disk_rows(2) == ([2, 1, 0], 13)


def test_sim_ref_disk_blur_is_filter2d_restatement():
    """The integer disk mean equals the float64 correlation with the normalised disk, rounded, on reflect-101 padding."""
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    for r in (1, 2, 5, 9, 20):
        hw = sim_ref.disk_rows(r)
        k = np.zeros((2 * r + 1, 2 * r + 1))
        for dy, h in enumerate(hw):
            k[r + dy, r - h:r + h + 1] = k[r - dy, r - h:r + h + 1] = 1
        k /= k.sum()
        pad = u8[sim_ref.reflect101(np.arange(-r, 13 + r), 13)][:, sim_ref.reflect101(np.arange(-r, 17 + r), 17)].astype(np.float64)
        acc = sum(k[a, b] * pad[a:a + 13, b:b + 17] for a in range(2 * r + 1) for b in range(2 * r + 1) if k[a, b])
        assert np.array_equal(np.rint(acc).astype(np.uint8), sim_ref.disk_blur(u8, r)), r
