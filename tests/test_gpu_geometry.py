"""GPU tests (MI355X) of the geometry path: hn_grid_points, the marching-tetrahedra passes (hn_iso_*) against the NumPy
float32 restatement (tests/isosurface_restated.py), NerfModel.query_points against a CPU restatement of the field
(tests/field_restated.py, composed from the oracle's blocks), density_grid and extract_mesh.

Tolerances.  Faces are integers and the orderings are part of the definition: identical.  A position is ONE
interpolation pos(a) + t * (pos(b) - pos(a)) of fp32 operations that both sides round one by one; 4 * 2^-23 * max|bound|
allows a few roundings of it.  Normals 1e-5.  query_points: what tests/test_gpu_model.py applies to `warped_points` and
`rgb` in fp32 mode (1e-4 element-wise, gpu_common.assert_close); sigma gets the absolute tolerance that bound gives the raw
density, 1e-4 * max(1, max|raw|), since Softplus has slope <= 1."""
import functools
import os

import numpy as np
import pytest
import torch

import field_restated as FR
import hashprng as H
import hypernerf_torch_amd as HN
import isosurface_restated as R
import test_isosurface_host as HT
from gpu_common import DEV, EMB, assert_close, rays_for
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import models, warping
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu

# name -> (grid builder, iso, bounds, what the checker must report on the GPU's own output)
FIELDS = {
    "sphere17": (lambda: HT.sphere(17), 0.0, HT.UNIT, dict(closed=True, oriented=True, euler=2)),
    "sphere33": (lambda: HT.sphere(33), 0.0, HT.UNIT, dict(closed=True, oriented=True, euler=2)),
    "torus17": (lambda: HT.torus(17), 0.0, HT.UNIT, dict(closed=True, oriented=True, euler=0)),
    "two_spheres17": (lambda: HT.two_spheres(17), 0.0, HT.UNIT, dict(closed=True, oriented=True, euler=4)),
    "octahedron17": (lambda: HT.octahedron()[0], 0.0, HT.octahedron()[1], dict(closed=True, oriented=True, euler=2)),
    "plane_5x7x9": (lambda: HT.plane((5, 7, 9), 0.9), 0.0, HT.PLANE_BOUNDS, dict(closed=False)),
    "plane_2x2x2": (lambda: HT.plane((2, 2, 2), 0.6), 0.0, HT.PLANE_BOUNDS, dict(closed=False)),
    # many workgroups in every pass, and point / cell / edge counts that are no multiple of 256
    "wavy_33x17x9": (lambda: (HT.plane((33, 17, 9), 0.9)
                              + 0.2 * np.sin(7.0 * HT.positions((33, 17, 9), HT.PLANE_BOUNDS)[..., 0])).astype(np.float32),
                     0.05, HT.PLANE_BOUNDS, dict(closed=False)),
}


@functools.lru_cache(maxsize=None)
def restated(name):
    build, iso, bounds, _ = FIELDS[name]
    f = build()
    return f, R.extract_isosurface(f, iso, bounds)


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_isosurface_matches_the_restatement(name):
    _, iso, bounds, expect = FIELDS[name]
    f, ref = restated(name)
    g = torch.from_numpy(f).to(DEV)
    a = HN.extract_isosurface(g, iso, bounds)
    b = HN.extract_isosurface(g, iso, bounds)
    for k in ("vertices", "normals", "faces"):
        assert a[k].device == g.device and a[k].is_contiguous()
        assert torch.equal(a[k], b[k]), f"{name}: {k} differs between two runs"
    v, nrm, faces = (a[k].cpu().numpy() for k in ("vertices", "normals", "faces"))
    assert v.dtype == np.float32 and nrm.dtype == np.float32 and faces.dtype == np.int32
    assert v.shape == ref["vertices"].shape and faces.shape == ref["faces"].shape and faces.shape[0] > 0, (v.shape, faces.shape)
    assert np.array_equal(faces, ref["faces"])
    pos_err = float(np.abs(v.astype(np.float64) - ref["vertices"].astype(np.float64)).max())
    nrm_err = float(np.abs(nrm.astype(np.float64) - ref["normals"].astype(np.float64)).max())
    print(f"{name}: V {v.shape[0]} F {faces.shape[0]} max position error {pos_err:.3e} max normal error {nrm_err:.3e}")
    assert pos_err <= 4.0 * 2.0 ** -23 * max(abs(x) for x in bounds)
    assert nrm_err <= 1e-5
    # the checker on the GPU's own mesh
    c = R.check_mesh(v, faces)
    for k, want in expect.items():
        assert c[k] == want, (name, k, c)
    if expect.get("closed"):
        assert c["volume"] > 0, c
    if name == "octahedron17":
        assert abs(c["volume"] - 256.0 / 3.0) < 1e-4, c["volume"]
    if name.startswith("sphere"):
        want = 4.0 / 3.0 * np.pi * 0.7071 ** 3
        assert abs(c["volume"] - want) / want < (0.01 if name == "sphere33" else 0.02)
    if name.startswith("plane"):
        offset = 0.9 if name == "plane_5x7x9" else 0.6
        assert np.abs(v.astype(np.float64) @ HT.PLANE_N + 0.0123 + offset).max() < 1e-6
        assert np.abs(nrm - (-HT.PLANE_N / np.linalg.norm(HT.PLANE_N))).max() < 1e-6


def test_empty_surface_and_nan():
    g = torch.zeros((5, 6, 7), device=DEV)
    for grid, iso in ((g, 0.5), (g, -0.5), (torch.full((3, 3, 3), float("nan"), device=DEV), 0.0)):
        m = HN.extract_isosurface(grid, iso, HT.UNIT)
        assert m["vertices"].shape == (0, 3) and m["normals"].shape == (0, 3) and m["faces"].shape == (0, 3)
        assert m["faces"].dtype == torch.int32 and m["vertices"].is_cuda


def test_grid_points_bit_exact():
    shape, bounds = (5, 7, 9), (-1.0, 1.5, -0.7, 0.9, 0.1, 2.0)
    n = 5 * 7 * 9
    whole = F.grid_points(shape, bounds, 0, n, DEV).cpu().numpy()
    assert np.array_equal(whole, R.lattice_points(shape, bounds))
    # a chunk that starts and ends in the middle of a k-row, and the padded tail (indices past the lattice = last point)
    for start, count in ((37, 130), (300, 64), (n - 1, 3)):
        got = F.grid_points(shape, bounds, start, count, DEV).cpu().numpy()
        assert np.array_equal(got, R.lattice_points(shape, bounds, start, count)), (start, count)
    with pytest.raises(ValueError):
        F.grid_points(shape, bounds, n, 4, DEV)


QUERY_CASES = {
    "bendy_fused": (dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True), "translation", {}),
    "axis": (dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=False, use_alpha_cond=False),
             "translation", {}),
    "nowarp": (dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=False, use_alpha_cond=False), "translation", {}),
    "se3_axis": (dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=True, use_alpha_cond=True),
                 "se3", {}),
    "call_nowarp": (dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=True, use_alpha_cond=True), "translation",
                    dict(use_warp=False)),
}


def small_model(kw, warp_kind, seed, nc=8, nf=8):
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.7, **kw)
    if warp_kind == "se3":
        m.warp_field = warping.SE3Field(in_ch=3)
    sd = H.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    for k in sd:        # small rigid motions, as tests/test_gpu_model.py sets them up
        if k.startswith(("warp_field.w_net.logit_layer", "warp_field.v_net.logit_layer")):
            sd[k] = sd[k] * 0.02
    m.load_state_dict(sd)
    return m.to(DEV), sd


def query_inputs(seed, b=6, s=8):
    pts = H.uniform(seed, "query_pts", (b, s, 3), -1.0, 1.0)
    vd = H.uniform(seed, "query_vd", (b, 3), -1.0, 1.0)
    vd = vd / vd.norm(dim=-1, keepdim=True)
    return pts, vd, rays_for(seed, b)[2]


def assert_query_close(out, ref, what):
    b, s = ref["sigma"].shape
    assert out["warped_points"].shape == ref["warped_points"].shape and out["rgb"].shape == (b, s, 3)
    assert out["sigma"].shape == (b, s) and out["sigma"].dtype == torch.float32
    assert not any(v.requires_grad for v in out.values())
    assert_close(out["warped_points"], ref["warped_points"], 1e-4, f"{what} warped_points")
    assert_close(out["rgb"], ref["rgb"], 1e-4, f"{what} rgb")
    tol = 1e-4 * max(1.0, float(ref["alpha"].abs().max()))
    err = float((out["sigma"].cpu().double() - ref["sigma"].double()).abs().max())
    print(f"{what}: sigma max abs error {err:.3e} (bound {tol:.3e})")
    assert torch.isfinite(out["sigma"]).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize("case", sorted(QUERY_CASES))
@pytest.mark.parametrize("level", ["coarse", "fine"])
def test_query_points_vs_field_restatement(case, level):
    HN.set_precision("fp32")
    kw, warp_kind, call = QUERY_CASES[case]
    seed = 131
    m, sd = small_model(kw, warp_kind, seed)
    pts, vd, idx = query_inputs(seed)
    cfg = O.ModelCfg(n_samples_coarse=8, n_samples_fine=8, warp_kind=warp_kind, **kw)
    with torch.no_grad():
        ref = FR.query_points(sd, cfg, level, pts, vd, idx, **call)
    meta = {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}
    out = m.query_points(pts.to(DEV), meta, level=level, viewdirs=vd.to(DEV), **call)      # called in grad mode
    assert_query_close(out, ref, f"query_points {case} {level}")
    # ids as (B, 1), and no view direction: sigma and the warp do not depend on it
    out2 = m.query_points(pts.to(DEV), {k: v[:, None] for k, v in meta.items()}, level=level, **call)
    assert torch.equal(out2["sigma"], out["sigma"]) and torch.equal(out2["warped_points"], out["warped_points"])
    if case == "bendy_fused":
        assert ("level", level) in m._template_calls
    if case == "se3_axis":
        assert any(k[0] == "tgather" for k in m._template_calls)
    assert getattr(m, "_level_state", None) is None


def test_query_points_honours_render_opts():
    HN.set_precision("fp32")
    kw, warp_kind, _ = QUERY_CASES["bendy_fused"]
    seed = 137
    m, sd = small_model(kw, warp_kind, seed)
    pts, vd, idx = query_inputs(seed)
    cfg = O.ModelCfg(n_samples_coarse=8, n_samples_fine=8, **kw)
    with torch.no_grad():
        plain = FR.query_points(sd, cfg, "fine", pts, vd, idx)
    # the threshold in the middle of the widest gap between neighbouring densities of the central half: no density of the
    # fixture may sit within the comparison's tolerance of it
    srt = plain["sigma"].reshape(-1).sort().values[12:36]
    gap, at = (srt[1:] - srt[:-1]).max(0)
    dust = float(srt[at] + 0.5 * gap)
    assert float(gap) > 4e-4 * max(1.0, float(plain["alpha"].abs().max())), "no usable gap for the dust threshold"
    opts = {"dust_threshold": dust, "bounding_box": (-0.6, 0.7, -0.8, 0.5, -0.9, 0.9)}
    with torch.no_grad():
        ref = FR.query_points(sd, cfg, "fine", pts, vd, idx, render_opts=opts)
    zeros = int((ref["sigma"] == 0).sum())
    assert 0 < zeros < ref["sigma"].numel() and zeros > int((plain["sigma"] < dust).sum())      # both filters bite
    meta = {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}
    out = m.query_points(pts.to(DEV), meta, viewdirs=vd.to(DEV), render_opts=opts)
    assert_query_close(out, ref, "query_points render_opts")
    assert torch.equal(out["sigma"].cpu() == 0, ref["sigma"] == 0)
    only_box = m.query_points(pts.to(DEV), meta, viewdirs=vd.to(DEV), render_opts={"bounding_box": opts["bounding_box"]})
    inside = O.filter_sigma(pts, torch.ones(pts.shape[:2]), {"bounding_box": opts["bounding_box"]}) > 0
    assert torch.equal(only_box["sigma"].cpu() > 0, inside)
    # noise_std of the model (0.7) adds nothing: two calls agree bit for bit
    again = m.query_points(pts.to(DEV), meta, viewdirs=vd.to(DEV), render_opts=opts)
    assert torch.equal(again["sigma"], out["sigma"]) and torch.equal(again["rgb"], out["rgb"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_density_grid_equals_query_points_and_ignores_chunk(prec):
    HN.set_precision(prec)
    kw, warp_kind, _ = QUERY_CASES["bendy_fused"]
    m, _ = small_model(kw, warp_kind, 139)
    shape, bounds, frame = (5, 6, 7), (-0.8, 0.9, -0.7, 0.6, -0.5, 0.75), 17
    n = 5 * 6 * 7
    one = HN.density_grid(m, bounds, shape, frame)                       # one chunk: 4 rows of 64, 46 padded points
    many = HN.density_grid(m, bounds, shape, frame, chunk=64)            # four chunks of one row
    assert one.shape == shape and one.dtype == torch.float32 and one.device == next(m.parameters()).device
    assert torch.equal(one, many)
    pts = F.grid_points(shape, bounds, 0, n, DEV).view(15, 14, 3)        # the same points in another row layout
    ids = torch.full((15,), frame, dtype=torch.int64, device=DEV)
    direct = m.query_points(pts, {k: ids for k in ("warp", "camera", "appearance", "time")})["sigma"]
    assert torch.equal(one.reshape(-1), direct.reshape(-1))
    assert float(one.std()) > 0
    other = HN.density_grid(m, bounds, shape, frame + 1)                 # another frame: another warp, another field
    assert not torch.equal(other, one)
    coarse = HN.density_grid(m, bounds, shape, frame, level="coarse")
    assert not torch.equal(coarse, one)
    boxed = HN.density_grid(m, bounds, shape, frame, render_opts={"bounding_box": (-9.0, 0.0, -9.0, 9.0, -9.0, 9.0)})
    x = torch.from_numpy(R.lattice_points(shape, bounds)[:, 0].reshape(shape)).to(DEV)
    assert torch.equal(boxed, torch.where(x <= 0.0, one, torch.zeros_like(one)))


def test_extract_mesh_is_the_composition(tmp_path):
    HN.set_precision("fp32")
    kw, warp_kind, _ = QUERY_CASES["bendy_fused"]
    m, _ = small_model(kw, warp_kind, 149)
    bounds, res, frame = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), (9, 8, 10), 3
    grid = HN.density_grid(m, bounds, res, frame, chunk=256)
    iso = float(grid.median())
    mesh = HN.extract_mesh(m, bounds, res, frame, iso=iso, chunk=256)
    ref = HN.extract_isosurface(grid, iso, bounds)
    assert mesh["faces"].shape[0] > 0 and mesh["vertices"].shape[0] > 0
    for k in ("vertices", "normals", "faces"):
        assert torch.equal(mesh[k], ref[k]), k
    cpu = R.extract_isosurface(grid.cpu().numpy(), iso, bounds)
    assert np.array_equal(mesh["faces"].cpu().numpy(), cpu["faces"])
    path = os.path.join(tmp_path, "mesh.ply")
    HN.write_ply(path, mesh["vertices"], mesh["faces"], mesh["normals"])
    back = HN.read_ply(path)
    for k in ("vertices", "normals", "faces"):
        assert np.array_equal(back[k], mesh[k].cpu().numpy()), k


@pytest.mark.parametrize("case", ["bendy_fused", "se3_axis"])
def test_forward_is_undisturbed_by_query_points(case):
    """Same model, same rays, same draws: forward before and after a query_points call (both levels, with render_opts)
    gives the same bits — cached programs, packed weights and _level_state are left as forward needs them."""
    HN.set_precision("fp32")
    kw, warp_kind, _ = QUERY_CASES[case]
    seed, b, nc, nf = 151, 12, 8, 8
    m, _ = small_model(kw, warp_kind, seed, nc, nf)
    o, d, idx = rays_for(seed, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1).to(DEV), "u": H.uniform(seed, "u", (b, nf), 0, 1).to(DEV),
           "noise_coarse": (H.normal(seed, "n1", (b, nc, 1)) * 0.7).to(DEV),
           "noise_fine": (H.normal(seed, "n2", (b, nc + nf, 1)) * 0.7).to(DEV)}
    before = m(rays, {}, rng=rng)
    pts, vd, qidx = query_inputs(seed)
    meta = {k: qidx.to(DEV) for k in ("warp", "camera", "appearance", "time")}
    for level in ("coarse", "fine"):
        m.query_points(pts.to(DEV), meta, level=level, viewdirs=vd.to(DEV), render_opts={"dust_threshold": 0.1})
    after = m(rays, {}, rng=rng)
    for lvl in ("coarse", "fine"):
        for k in ("points", "warped_points", "rgb", "depth", "med_depth", "acc", "weights", "med_points"):
            assert torch.equal(before[lvl][k], after[lvl][k]), f"{case} {lvl}/{k}"
    loss = (after["coarse"]["rgb"] ** 2).mean() + (after["fine"]["rgb"] ** 2).mean()
    loss.backward()                                                      # and the training path still differentiates
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())
