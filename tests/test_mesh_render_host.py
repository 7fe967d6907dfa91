"""CPU tests of the mesh renderer's definition (tests/mesh_render_restated.py, the NumPy float32 restatement of
csrc/hn_mesh_render.hip) against a float64 brute-force caster of the same rule, of the cameras that feed it and of the
argument checks that run before any kernel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import mesh_render_restated as R
import mesh_render_scenes as S
import nerfies_scene as NS
from hypernerf_torch_amd import _lib as L
from oracle import hypernerf_oracle as O

PARITY = 1e-4          # the project's fp32 parity bound, relative
RAY_BOUND = 2e-6       # the project's bound on generated rays
MARGIN = 1e-4          # a pixel within this of an edge (normalised edge values) may go to either neighbour


@functools.lru_cache(maxsize=None)
def casts(mesh_name, cam_name):
    m = S.host_mesh(mesh_name)
    rays = S.host_rays(S.camera(cam_name))
    return m, rays, R.cast(m["vertices"], m["faces"], rays), R.cast(m["vertices"], m["faces"], rays, np.float64, MARGIN)


@pytest.mark.parametrize("cam_name", S.CAMERAS)
@pytest.mark.parametrize("mesh_name", list(S.GRIDS))
def test_fp32_statement_agrees_with_the_float64_caster(mesh_name, cam_name):
    _, _, got, want = casts(mesh_name, cam_name)
    amb = want["ambiguous"]
    n_pix = amb.size
    covered = int((want["face"] >= 0).sum())
    differ = int((got["face"] != want["face"]).sum())
    both = (got["face"] >= 0) & (want["face"] >= 0) & (got["face"] == want["face"])
    rel = np.abs(got["depth"].astype(np.float64) - want["depth"])[both] / want["depth"][both]
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{mesh_name}/{cam_name}: {covered} of {n_pix} covered, {int(amb.sum())} ambiguous, {differ} face differences, "
          f"depth rel err {worst:.2e}")
    assert covered > 0
    assert amb.sum() <= 0.01 * n_pix, "a condition of the test: at most 1 % of the pixels lie on an edge"
    assert np.array_equal(got["face"][~amb], want["face"][~amb])
    assert worst <= PARITY
    # barycentrics: non-negative, sum to one, and they rebuild the hit point
    hit = got["face"] >= 0
    w = got["bary"][hit].astype(np.float64)
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1.0).max() < 1e-6
    assert not got["bary"][~hit].any() and not got["depth"][~hit].any()


@pytest.mark.parametrize("mesh_name", ["sphere9", "sphere17"])
def test_no_pinholes(mesh_name):
    m = S.host_mesh(mesh_name)
    rmin = np.linalg.norm(m["vertices"].astype(np.float64) - S.SPHERE_CENTRE, axis=1).min()
    for cam_name in ("plain", "distorted"):
        _, rays, got, _ = casts(mesh_name, cam_name)
        o, d = rays[:, :3].astype(np.float64), rays[:, 3:6].astype(np.float64)
        to_c = S.SPHERE_CENTRE - o
        along = np.einsum("ij,ij->i", to_c, d)
        dist = np.linalg.norm(to_c - along[:, None] * d, axis=1)
        must = (dist < 0.97 * rmin) & (along > 0)
        assert must.sum() > 50, "the sphere fills a good part of the image"
        assert (got["face"][must] >= 0).all(), f"{int((got['face'][must] < 0).sum())} pinholes through {cam_name}"
    _, _, got, _ = casts(mesh_name, "inside")
    assert (got["face"] >= 0).all(), "from inside a closed surface every pixel is covered"


def test_depth_of_a_quad_is_the_analytic_plane():
    n, c = np.array([0.2, -0.3, 1.0]), 1.7                        # the plane n . x = c
    xy = np.array([[-9.0, -7.0], [9.0, -7.0], [9.0, 7.0], [-9.0, 7.0]])
    corners = np.concatenate([xy, ((c - xy @ n[:2]) / n[2])[:, None]], axis=1)
    quad = S.quad(corners)
    for cam_name in ("plain", "distorted"):
        rays = S.host_rays(S.camera(cam_name))
        got = R.cast(quad["vertices"], quad["faces"], rays)
        assert (got["face"] >= 0).all()
        o, d = rays[:, :3].astype(np.float64), rays[:, 3:6].astype(np.float64)
        # the plane through the ROUNDED corners: three of them span it, the fourth is off it by a rounding
        v = quad["vertices"].astype(np.float64)
        nn = np.cross(v[1] - v[0], v[2] - v[0])
        want = ((v[0] - o) @ nn) / (d @ nn)
        rel = np.abs(got["depth"] - want) / want
        print(f"quad/{cam_name}: depth rel err {rel.max():.2e}")
        assert rel.max() <= PARITY
        assert set(np.unique(got["face"])) == {0, 1}


def test_coincident_faces_go_to_the_smaller_id_and_degenerate_faces_are_never_hit():
    rays = S.host_rays(S.camera("plain"))
    corners = [[-9, -7, 2], [9, -7, 2], [9, 7, 2], [-9, 7, 2]]
    q = S.quad(corners)
    v = np.concatenate([q["vertices"], q["vertices"], [[0, 0, 1], [np.nan, 0, 1], [-1, 0, 1], [0.25, 0, 1], [1, 0, 1]]]).astype(np.float32)
    #         a zero-area face, two with a repeated id, a NaN vertex — all in front of the quads — then the quad twice
    f = np.array([[10, 11, 12], [0, 8, 8], [8, 8, 8], [9, 0, 1], [4, 5, 6], [4, 6, 7], [0, 1, 2], [0, 2, 3]], dtype=np.int32)
    got = R.cast(v, f, rays)
    assert set(np.unique(got["face"])) == {4, 5}
    flipped = R.cast(v, f[[0, 1, 2, 3, 6, 7, 4, 5]], rays)
    assert np.array_equal(flipped["face"], got["face"]) and np.array_equal(flipped["depth"], got["depth"])
    nan_rays = rays.copy()
    nan_rays[5, 4] = np.nan
    got2 = R.cast(v, f, nan_rays)
    assert got2["face"][5] == -1 and got2["depth"][5] == 0 and np.array_equal(np.delete(got2["face"], 5), np.delete(got["face"], 5))


def test_camera_from_c2w_gives_the_llff_rays():
    rng = np.random.RandomState(3)
    h, w, focal = 37, 50, 41.5
    for _ in range(3):
        rot = NS._rotation(rng)
        c2w = np.concatenate([rot, rng.uniform(-2, 2, (3, 1))], axis=1).astype(np.float32)      # the oracle runs in fp32
        rec = HN.camera_from_c2w(c2w, focal, w, h)
        assert rec.dtype == np.float32 and rec.shape == (24,)
        want = O.image_rays(h, w, focal, torch.from_numpy(c2w), 0.5, 4.0, ndc=False).numpy()
        got = NS.rays_f64(R.camera_dict(rec, (w, h)), 0.5, 4.0)
        err = np.abs(got - want).max()
        print(f"camera_from_c2w: max ray difference {err:.2e}")
        assert err <= RAY_BOUND
        # and a tensor pose gives the same record
        assert np.array_equal(HN.camera_from_c2w(torch.from_numpy(c2w), focal, w, h), rec)
    with pytest.raises(ValueError, match="NDC"):
        HN.camera_from_c2w(c2w, focal, w, h, ndc=True)
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        HN.camera_from_c2w(np.eye(4), focal, w, h)
    with pytest.raises(ValueError, match="positive"):
        HN.camera_from_c2w(c2w, 0.0, w, h)


@pytest.mark.parametrize("up", [(0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -0.5, 0.8)])
def test_orbit_cameras_look_at_the_centre_from_the_radius(up):
    centre, radius, wh = np.array([0.4, -0.2, 1.1]), 2.5, (50, 37)
    cams = HN.orbit_cameras(centre, radius, 7, elevation=25.0, up=up, focal=44.0, image_wh=wh)
    assert cams.shape == (7, 24) and cams.dtype == np.float32
    u = np.asarray(up) / np.linalg.norm(up)
    for rec in cams:
        r = rec.astype(np.float64)
        rot = r[0:9].reshape(3, 3)
        assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6 and np.linalg.det(rot) > 0.999
        assert abs(np.linalg.norm(r[9:12] - centre) - radius) < 1e-6 * radius
        pix, z = R.project(rec, centre[None])
        assert abs(z[0] - radius) < 1e-5 and np.abs(pix[0] - np.array([wh[0] / 2, wh[1] / 2])).max() < 1e-4
        assert abs((r[9:12] - centre) @ u / radius - np.sin(np.deg2rad(25.0))) < 1e-6       # the elevation
        above, _ = R.project(rec, (centre + 0.1 * u)[None])
        assert above[0, 1] < wh[1] / 2 and abs(above[0, 0] - wh[0] / 2) < 1e-4              # `up` is up in the image
    assert len({tuple(np.round(c[9:12], 4)) for c in cams}) == 7
    for bad in (dict(elevation=90.0), dict(radius=0.0), dict(n=0), dict(up=(0, 0, 0)), dict(focal=-1.0), dict(image_wh=(0, 4))):
        kw = dict(center=centre, radius=radius, n=7, elevation=0.0, up=up, focal=44.0, image_wh=wh)
        kw.update(bad)
        with pytest.raises(ValueError):
            HN.orbit_cameras(**kw)


@pytest.mark.parametrize("cam_name", ["plain", "distorted"])
def test_forward_projection_undoes_the_newton_inverse(cam_name):
    rec = S.camera(cam_name)
    w, h = S.WH
    rays = NS.rays_f64(R.camera_dict(rec, S.WH), 0.0, 6.0)
    j, i = np.mgrid[0:h, 0:w]
    for depth in (0.5, 3.0):
        pix, z = R.project(rec, rays[:, :3] + depth * rays[:, 3:6])
        assert (z > 0).all()
        err = max(np.abs(pix[:, 0] - (i.reshape(-1) + 0.5)).max(), np.abs(pix[:, 1] - (j.reshape(-1) + 0.5)).max())
        print(f"{cam_name}: pixel -> ray -> pixel round trip {err:.2e} px")
        assert err < 1e-4


def test_the_nerfies_dataset_hands_out_the_record_of_an_image(tmp_path):
    from hypernerf_torch_amd.datasets.nerfies import NerfiesDataset
    scene = NS.make_scene(7)
    root = NS.write_scene(str(tmp_path / "capture"), scene)
    ds = NerfiesDataset(root, split="train", image_scale=2, device="cpu")
    for idx in range(len(ds.ids)):
        rec = ds.camera_record(idx)
        assert rec.dtype == torch.float32 and tuple(rec.shape) == (24,) and torch.equal(rec, ds.cams[idx])
        # the forward model of that record returns every pixel of the image's own rays
        cam = NS.scaled_camera(scene["cameras"][ds.ids[idx]], scene["image_scale"], scene["scene"])
        rays = NS.rays_f64(cam, ds.near, ds.far)
        pix, z = R.project(rec.numpy(), rays[:, :3] + 0.7 * rays[:, 3:6])
        j, i = np.mgrid[0:ds.img_wh[1], 0:ds.img_wh[0]]
        assert (z > 0).all() and np.abs(pix - np.stack([i.reshape(-1) + 0.5, j.reshape(-1) + 0.5], -1)).max() < 1e-3


def test_entry_points_are_declared_built_and_refuse_bad_arguments():
    names = {"hn_mesh_project", "hn_mesh_bin_count", "hn_mesh_bin_fill", "hn_mesh_trace", "hn_mesh_shade"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES) and "hn_mesh_render.hip" in L.SOURCES
    assert HN.render_mesh is HN.geometry.render_mesh
    lib = L.load()
    one = C.c_void_p(64)         # a non-NULL pointer that is never followed: every call below is refused before a launch
    col, bad_col = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.5, 1.5, 0.5)
    assert lib.hn_mesh_project(one, 0, one, one, one, None) == -2
    assert lib.hn_mesh_project(None, 4, one, one, one, None) == -3
    assert lib.hn_mesh_project(one, 4, one, one, None, None) == -3
    assert lib.hn_mesh_bin_count(one, 0, one, one, one, 4, one, 8, 8, one, one, None) == -2
    assert lib.hn_mesh_bin_count(one, 4, one, one, one, 4, one, 0, 8, one, one, None) == -2
    assert lib.hn_mesh_bin_count(one, 4, one, one, one, 4, one, 8, 65536, one, one, None) == -2
    assert lib.hn_mesh_bin_count(one, 4, one, one, one, 4, one, 8, 8, one, None, None) == -3
    assert lib.hn_mesh_bin_fill(one, 4, one, one, one, 4, one, 8, 8, one, 0, one, one, None) == -2
    assert lib.hn_mesh_bin_fill(one, 4, one, one, one, 4, one, 8, 8, one, 2 ** 31, one, one, None) == -2
    assert lib.hn_mesh_bin_fill(one, 4, one, one, one, 4, one, 8, 8, None, 9, one, one, None) == -3
    assert lib.hn_mesh_trace(one, 4, one, 4, one, 5, 8, 8, one, one, one, 9, one, one, one, None) == -2
    assert lib.hn_mesh_trace(one, 4, one, 4, one, 8, 0, 8, one, one, one, 9, one, one, one, None) == -2
    assert lib.hn_mesh_trace(one, 4, one, 4, one, 8, 8, 8, one, one, one, -1, one, one, one, None) == -2
    assert lib.hn_mesh_trace(one, 4, one, 4, one, 8, 8, 8, one, one, None, 9, one, one, one, None) == -3
    assert lib.hn_mesh_trace(one, 4, one, 4, None, 8, 8, 8, one, one, one, 9, one, one, one, None) == -3
    assert lib.hn_mesh_trace(None, 0, None, 0, one, 8, 8, 8, one, one, None, 0, one, one, None, None) == -3
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 0, one, 8, 0, one, one, 1, 0.3, col, col, one, one, one, None) == -2
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 3, one, 8, 64, one, one, 1, 0.3, col, col, one, one, one, None) == -2
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 0, one, 8, 64, one, one, 1, 1.5, col, col, one, one, one, None) == -2
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 0, one, 8, 64, one, one, 1, 0.3, bad_col, col, one, one, one, None) == -2
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 1, one, 8, 64, one, one, 1, 0.3, col, col, one, one, one, None) == -3
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 0, one, 8, 64, None, one, 1, 0.3, col, col, one, one, one, None) == -3
    assert lib.hn_mesh_shade(one, 4, one, 4, None, None, 0, one, 8, 64, one, one, 1, 0.3, col, None, one, one, one, None) == -3


def cpu_mesh(**over):
    q = S.quad([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]])
    m = {"vertices": torch.from_numpy(q["vertices"]), "faces": torch.from_numpy(q["faces"]),
         "normals": torch.tensor([[0.0, 0.0, -1.0]] * 4), "colors": torch.full((4, 3), 200, dtype=torch.uint8)}
    m.update(over)
    return {k: v for k, v in m.items() if v is not None}


def test_render_mesh_checks_its_arguments_before_it_needs_a_gpu():
    w, h = 8, 6
    rays = torch.zeros(w * h, 8)
    cam = torch.from_numpy(S.camera("plain", (w, h)))
    m = cpu_mesh()
    for over in (dict(vertices=m["vertices"].double()), dict(vertices=m["vertices"][:, :2]), dict(faces=m["faces"].long()),
                 dict(faces=m["faces"][:, :2]), dict(normals=m["normals"][:3]), dict(colors=m["colors"][:3]),
                 dict(colors=m["colors"].to(torch.int32))):
        with pytest.raises(ValueError, match="|".join(over)):
            HN.render_mesh(cpu_mesh(**over), rays, cam, (w, h))
    with pytest.raises(ValueError, match="dict"):
        HN.render_mesh(m["vertices"], rays, cam, (w, h))
    with pytest.raises(ValueError, match="image_wh|sides"):
        HN.render_mesh(m, rays, cam, (w, 0))
    with pytest.raises(ValueError, match="sides"):
        HN.render_mesh(m, rays, cam, (65536, 1))
    with pytest.raises(ValueError, match="camera"):
        HN.render_mesh(m, rays, cam[:20], (w, h))
    with pytest.raises(ValueError, match="camera"):
        HN.render_mesh(m, rays, cam.double(), (w, h))
    with pytest.raises(ValueError, match="rays"):
        HN.render_mesh(m, rays[:-1], cam, (w, h))
    with pytest.raises(ValueError, match="rays"):
        HN.render_mesh(m, rays[:, :5], cam, (w, h))
    with pytest.raises(ValueError, match="shading"):
        HN.render_mesh(m, rays, cam, (w, h), shading="phong")
    with pytest.raises(ValueError, match="ambient"):
        HN.render_mesh(m, rays, cam, (w, h), ambient=1.5)
    with pytest.raises(ValueError, match="background"):
        HN.render_mesh(m, rays, cam, (w, h), background=(1, 1))
    with pytest.raises(ValueError, match="base_color"):
        HN.render_mesh(m, rays, cam, (w, h), base_color=(0.5, 0.5, 2.0))
    # a call that passes every check still needs the GPU: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        HN.render_mesh(m, rays, cam, (w, h))
    with pytest.raises(ValueError, match="GPU"):
        HN.mesh_turntable(m, "unused.gif", n=2, image_wh=(w, h))
    with pytest.raises(ValueError, match="no vertices"):
        HN.mesh_turntable(cpu_mesh(vertices=torch.zeros(0, 3), normals=None, colors=None), "unused.gif")


def test_depth_agreement_on_hand_made_images():
    face = torch.tensor([[0, 3, -1], [-1, 7, 2]], dtype=torch.int32)
    mesh_depth = torch.tensor([[1.0, 2.0, 0.0], [0.0, 4.0, 5.0]])
    field_depth = torch.tensor([[1.5, 2.0, 9.0], [3.0, 3.0, 9.0]])
    acc = torch.tensor([[0.9, 0.5, 0.8], [0.1, 1.0, 0.49]])
    got = HN.depth_agreement(mesh_depth, face, field_depth, acc)
    # mesh covers 4 pixels, the field 4, both 3 (errors -0.5, 0, 1), the union 5
    assert int(got["n"]) == 3 and got["n"].dtype == torch.int64
    assert float(got["abs_mean"]) == pytest.approx(0.5) and float(got["rmse"]) == pytest.approx(np.sqrt(1.25 / 3))
    assert float(got["iou"]) == pytest.approx(3 / 5)
    strict = HN.depth_agreement(mesh_depth, face, field_depth, acc, acc_min=0.95)
    assert int(strict["n"]) == 1 and float(strict["abs_mean"]) == pytest.approx(1.0) and float(strict["iou"]) == pytest.approx(1 / 4)
    nothing = HN.depth_agreement(mesh_depth, torch.full_like(face, -1), field_depth, torch.zeros_like(acc))
    assert int(nothing["n"]) == 0 and all(torch.isnan(nothing[k]) for k in ("abs_mean", "rmse", "iou"))
    with pytest.raises(ValueError, match="size"):
        HN.depth_agreement(mesh_depth[:1], face, field_depth, acc)
    with pytest.raises(ValueError, match="integer"):
        HN.depth_agreement(mesh_depth, face.float(), field_depth, acc)
