"""GPU tests of the mesh renderer (csrc/hn_mesh_render.hip, geometry.render_mesh) against the NumPy float32 restatement
of its definition (tests/mesh_render_restated.py): face, depth and barycentrics bit for bit, on meshes extract_isosurface
made on the GPU and rays the GPU's own generator wrote; binning against brute force; batching; robustness; shading;
determinism; the depth agreement numbers and the turntable GIF.  A restated image is computed once and shared."""
import functools
import os

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import mesh_render_restated as R
import mesh_render_scenes as S
import test_isosurface_host as HT
from gpu_common import DEV, EMB, load_hash
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import inference

pytestmark = pytest.mark.gpu

TRACE_KEYS = ("face", "depth", "bary")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.dtype == b.dtype and a.size == b.size and np.array_equal(bits(a).reshape(-1), bits(b).reshape(-1))


def to_gpu(mesh):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in mesh.items() if v is not None}


def to_host(mesh):
    return {k: v.cpu().numpy() for k, v in mesh.items()}


@functools.lru_cache(maxsize=None)
def gpu_mesh(name):
    return HN.extract_isosurface(torch.from_numpy(S.GRIDS[name]()).to(DEV), 0.0, HT.UNIT)


@functools.lru_cache(maxsize=None)
def gpu_rays(cam_name, wh):
    cam = torch.from_numpy(S.camera(cam_name, wh)).to(DEV)
    return cam, HN.camera_rays(cam, wh[0], wh[1], 0.0, 6.0)


@functools.lru_cache(maxsize=None)
def restated(mesh_name, cam_name, wh):
    m = to_host(gpu_mesh(mesh_name))
    return R.cast(m["vertices"], m["faces"], gpu_rays(cam_name, wh)[1].cpu().numpy())


def assert_traced(got, want, wh, what):
    for k in TRACE_KEYS:
        assert tuple(got[k].shape[:2]) == (wh[1], wh[0]), (what, k)
        assert same_bits(got[k], want[k]), f"{what}: '{k}' differs from the restatement"


def check_both_ways(mesh, cam, rays, wh, want, what):
    """binning=True and binning=False both give the restated arrays, bit for bit."""
    binned = HN.render_mesh(mesh, rays, cam, wh)
    brute = HN.render_mesh(mesh, rays, cam, wh, binning=False)
    assert_traced(binned, want, wh, what + " (binned)")
    assert_traced(brute, want, wh, what + " (brute force)")
    for k in ("normal", "rgb", "rgb8"):
        assert torch.equal(binned[k], brute[k]), (what, k)
    return binned


@pytest.mark.parametrize("cam_name", S.CAMERAS)
@pytest.mark.parametrize("mesh_name", list(S.GRIDS))
def test_bit_identity_with_the_restatement(mesh_name, cam_name):
    cam, rays = gpu_rays(cam_name, S.WH)
    want = restated(mesh_name, cam_name, S.WH)
    assert (want["face"] >= 0).sum() > 100
    got = check_both_ways(gpu_mesh(mesh_name), cam, rays, S.WH, want, f"{mesh_name}/{cam_name}")
    assert got["face"].dtype == torch.int32 and got["depth"].dtype == torch.float32 and got["rgb8"].dtype == torch.uint8
    assert got["face"].device == rays.device


@pytest.mark.parametrize("cam_name", S.CAMERAS)
@pytest.mark.parametrize("wh", [(50, 37), (16, 16), (1, 1)])
def test_image_sizes_with_edge_tiles_one_tile_and_one_pixel(wh, cam_name):
    cam, rays = gpu_rays(cam_name, wh)
    want = restated("sphere17", cam_name, wh)
    assert (want["face"] >= 0).any()
    check_both_ways(gpu_mesh("sphere17"), cam, rays, wh, want, f"sphere17/{cam_name}/{wh}")


def test_a_quad_that_fills_the_distorted_image():
    cam, rays = gpu_rays("distorted", S.WH)
    quad = S.quad([[-9, -7, 2.0], [9, -7, 2.5], [9, 7, 2.0], [-9, 7, 1.5]])
    want = R.cast(quad["vertices"], quad["faces"], rays.cpu().numpy())
    assert (want["face"] >= 0).all()
    check_both_ways(to_gpu(quad), cam, rays, S.WH, want, "quad/distorted")


def test_a_ground_quad_under_and_behind_the_camera_takes_the_whole_image_box():
    quad = S.quad([[-5, 1, -8], [5, 1, -8], [5, 1, 8], [-5, 1, 8]])        # y = 1: below the camera at z = -3, y down
    mesh = to_gpu(quad)
    for cam_name in ("plain", "distorted"):
        cam, rays = gpu_rays(cam_name, S.WH)
        _, flags = F.mesh_project(mesh["vertices"], cam)
        assert flags.tolist() == [1, 1, 0, 0]
        want = R.cast(quad["vertices"], quad["faces"], rays.cpu().numpy())
        covered = want["face"].reshape(S.WH[1], S.WH[0]) >= 0
        assert covered[-1].all() and not covered[0].any(), "the ground fills the lower part of the image only"
        check_both_ways(mesh, cam, rays, S.WH, want, f"ground/{cam_name}")
    # all three vertices of a face behind the camera: binned to nothing, and the ray agrees
    behind = to_gpu(S.quad([[-5, 1, -8], [5, 1, -8], [5, -1, -4], [-5, -1, -4]]))
    cam, rays = gpu_rays("plain", S.WH)
    begin, end, pairs = F.mesh_bins(behind["vertices"], behind["faces"], cam, S.WH)
    assert pairs.numel() == 0 and torch.equal(begin, end)
    assert (HN.render_mesh(behind, rays, cam, S.WH, binning=False)["face"] == -1).all()


def stacked_triangles(n, seed):
    """n small triangles around pixel (40, 20) of the plain camera's 64 x 48 image (tile (2, 1)), at n different depths in
    a shuffled order, so that the nearest is neither the first nor the last of a batch by construction."""
    rng = np.random.RandomState(seed)
    rec = S.camera("plain").astype(np.float64)
    order = rng.permutation(n)
    verts, faces = [], []
    for k in range(n):
        z = 2.0 + 0.01 * order[k]
        for du, dv in ((-3.0, -2.5), (3.5, -2.0), (0.5, 3.0)):
            x, y = (40.5 + du - rec[15]) / rec[12], (20.5 + dv - rec[16]) / rec[12]
            verts.append(rec[9:12] + z * np.array([x, y, 1.0]))
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    return {"vertices": np.asarray(verts, dtype=np.float32), "faces": np.asarray(faces, dtype=np.int32)}, int(np.argmin(order))


@pytest.mark.parametrize("n", [65, 130])
def test_batches_of_faces_in_one_tile(n):
    cam, rays = gpu_rays("plain", S.WH)
    mesh, nearest = stacked_triangles(n, n)
    want = R.cast(mesh["vertices"], mesh["faces"], rays.cpu().numpy())
    assert want["face"].reshape(S.WH[1], S.WH[0])[20, 40] == nearest
    dev_mesh = to_gpu(mesh)
    check_both_ways(dev_mesh, cam, rays, S.WH, want, f"{n} stacked triangles")
    begin, end, _ = F.mesh_bins(dev_mesh["vertices"], dev_mesh["faces"], cam, S.WH)
    per_tile = (end - begin).cpu().numpy()
    assert per_tile.max() == n and (per_tile > 0).sum() <= 4, "the triangles sit inside one tile (and touch few others)"


def test_coincident_faces_go_to_the_smaller_id():
    cam, rays = gpu_rays("plain", S.WH)
    q = S.quad([[-9, -7, 2], [9, -7, 2], [9, 7, 2], [-9, 7, 2]])
    mesh = {"vertices": np.concatenate([q["vertices"], q["vertices"]]), "faces": np.concatenate([q["faces"] + 4, q["faces"]])}
    want = R.cast(mesh["vertices"], mesh["faces"], rays.cpu().numpy())
    assert set(np.unique(want["face"])) == {0, 1}
    check_both_ways(to_gpu(mesh), cam, rays, S.WH, want, "coincident quads")


def test_degenerate_faces_nan_and_an_empty_mesh_leave_the_rest_alone():
    cam, rays = gpu_rays("plain", S.WH)
    base = to_host(gpu_mesh("sphere17"))
    clean = HN.render_mesh(gpu_mesh("sphere17"), rays, cam, S.WH)
    v0 = base["vertices"].shape[0]
    extra_v = np.array([[-1, 0, -2], [0.25, 0, -2], [1, 0, -2], [np.nan, 0, -2], [0, np.inf, -2]], dtype=np.float32)
    extra_f = np.array([[v0, v0 + 1, v0 + 2],         # zero area, in front of the sphere
                        [0, 5, 5], [7, 7, 7],          # repeated ids
                        [v0 + 3, 0, 1], [2, v0 + 4, 3]], dtype=np.int32)       # a NaN and an infinite vertex
    mesh = {"vertices": np.concatenate([base["vertices"], extra_v]), "faces": np.concatenate([base["faces"], extra_f]),
            "normals": np.concatenate([base["normals"], np.zeros_like(extra_v)])}
    for binning in (True, False):
        got = HN.render_mesh(to_gpu(mesh), rays, cam, S.WH, binning=binning)
        for k in clean:
            assert same_bits(got[k], clean[k]), (k, binning)
    # a NaN ray row: that pixel sees nothing, every other pixel is unchanged
    bad = rays.clone()
    p = 20 * S.WH[0] + 30
    assert clean["face"].view(-1)[p] >= 0
    bad[p, 4] = float("nan")
    for binning in (True, False):
        got = HN.render_mesh(gpu_mesh("sphere17"), bad, cam, S.WH, background=(0.2, 0.4, 0.6), binning=binning)
        assert got["face"].view(-1)[p] == -1 and got["depth"].view(-1)[p] == 0 and not got["bary"].view(-1, 3)[p].any()
        assert got["rgb8"].view(-1, 3)[p].tolist() == [51, 102, 153]
        keep = torch.arange(rays.shape[0], device=DEV) != p
        for k in TRACE_KEYS:
            assert same_bits(got[k].view(rays.shape[0], -1)[keep], clean[k].view(rays.shape[0], -1)[keep]), (k, binning)
    # an empty mesh: all background, no launch fault
    empty = {"vertices": torch.zeros((0, 3), device=DEV), "faces": torch.zeros((0, 3), dtype=torch.int32, device=DEV)}
    for binning in (True, False):
        got = HN.render_mesh(empty, rays, cam, S.WH, background=(0.2, 0.4, 0.6), binning=binning)
        assert (got["face"] == -1).all() and not got["depth"].any() and not got["bary"].any() and not got["normal"].any()
        assert (got["rgb8"].view(-1, 3) == torch.tensor([51, 102, 153], dtype=torch.uint8, device=DEV)).all()
        assert torch.equal(got["rgb"].view(-1, 3), torch.tensor([0.2, 0.4, 0.6], device=DEV).expand(rays.shape[0], 3))
    torch.cuda.synchronize()


def test_an_out_of_range_face_id_raises_and_leaves_the_outputs_untouched():
    cam, rays = gpu_rays("plain", S.WH)
    mesh = gpu_mesh("sphere9")
    v, n = mesh["vertices"].shape[0], rays.shape[0]
    for bad_id in (v, -1, 2 ** 31 - 1):
        faces = mesh["faces"].clone()
        faces[faces.shape[0] // 2, 1] = bad_id
        out = {"face": torch.full((n,), 77, dtype=torch.int32, device=DEV), "depth": torch.full((n,), 7.0, device=DEV),
               "bary": torch.full((n, 3), 7.0, device=DEV)}
        for binning in (True, False):
            with pytest.raises(ValueError, match="outside"):
                F.mesh_trace(mesh["vertices"], faces, rays, cam, S.WH, binning=binning, out=out)
            with pytest.raises(ValueError, match="outside"):
                HN.render_mesh({"vertices": mesh["vertices"], "faces": faces}, rays, cam, S.WH, binning=binning)
        assert (out["face"] == 77).all() and (out["depth"] == 7.0).all() and (out["bary"] == 7.0).all()
    # and `out` is what a good call writes into
    got = F.mesh_trace(mesh["vertices"], mesh["faces"], rays, cam, S.WH, out=out)
    assert got["face"] is out["face"] and same_bits(out["depth"], restated("sphere9", "plain", S.WH)["depth"])


def colours(v, kind):
    rng = np.random.RandomState(11)
    if kind == "uint8":
        return rng.randint(0, 256, (v, 3)).astype(np.uint8)
    if kind == "fp32":
        return rng.uniform(-0.2, 1.4, (v, 3)).astype(np.float32)          # past both ends: the clamp is exercised
    return None


@pytest.mark.parametrize("shading,ambient", [("headlight", 0.3), ("headlight", 0.0), ("none", 0.3)])
@pytest.mark.parametrize("kind", ["uint8", "fp32", None])
@pytest.mark.parametrize("with_normals", [True, False])
def test_shading_against_the_restatement(with_normals, kind, shading, ambient):
    cam, rays = gpu_rays("distorted", S.WH)
    base = to_host(gpu_mesh("sphere17"))
    mesh = {"vertices": base["vertices"], "faces": base["faces"], "normals": base["normals"] if with_normals else None,
            "colors": colours(base["vertices"].shape[0], kind)}
    background, base_color = (0.1, 0.5, 0.9), (0.7, 0.6, 0.2)
    got = HN.render_mesh(to_gpu(mesh), rays, cam, S.WH, shading=shading, ambient=ambient, background=background,
                         base_color=base_color)
    want_trace = restated("sphere17", "distorted", S.WH)
    assert_traced(got, want_trace, S.WH, "shading scene")
    want = R.shade(mesh["vertices"], mesh["faces"], mesh["normals"], mesh["colors"], rays.cpu().numpy(), want_trace["face"],
                   want_trace["bary"], shading, ambient, background, base_color)
    normal, rgb = got["normal"].cpu().numpy().reshape(-1, 3), got["rgb"].cpu().numpy().reshape(-1, 3)
    err_n, err_c = np.abs(normal - want["normal"]).max(), np.abs(rgb - want["rgb"]).max()
    print(f"normals={with_normals} colours={kind} {shading}/{ambient}: normal err {err_n:.2e}, rgb err {err_c:.2e}")
    assert err_n <= 1e-6 and err_c <= 1e-6
    assert np.array_equal(got["rgb8"].cpu().numpy().reshape(-1, 3), R.quantise(rgb)), "rgb8 = floor(255 rgb + 0.5) of its own rgb"
    hit = want_trace["face"] >= 0
    assert np.abs(np.linalg.norm(normal[hit].astype(np.float64), axis=1) - 1.0).max() < 1e-6 and not normal[~hit].any()
    assert (rgb[~hit] == np.asarray(background, dtype=np.float32)).all() and rgb.min() >= 0.0 and rgb.max() <= 1.0
    if shading == "none" and kind is None:
        assert (rgb[hit] == np.asarray(base_color, dtype=np.float32)).all()


def test_two_runs_and_permuted_faces_give_the_same_image():
    for cam_name in ("distorted", "inside"):
        cam, rays = gpu_rays(cam_name, S.WH)
        mesh = gpu_mesh("torus33")
        a, b = HN.render_mesh(mesh, rays, cam, S.WH), HN.render_mesh(mesh, rays, cam, S.WH)
        for k in a:
            assert same_bits(a[k], b[k]), k
        perm = torch.from_numpy(np.random.RandomState(5).permutation(mesh["faces"].shape[0])).to(DEV)
        shuffled = dict(mesh, faces=mesh["faces"][perm].contiguous())
        c = HN.render_mesh(shuffled, rays, cam, S.WH)
        assert same_bits(c["depth"], a["depth"])
        undone = torch.where(c["face"] >= 0, perm[c["face"].clamp(min=0).long()].to(torch.int32), c["face"])
        assert torch.equal(undone, a["face"])


def test_depth_agreement_on_hand_made_images():
    face = torch.tensor([[0, 3, -1], [-1, 7, 2]], dtype=torch.int32, device=DEV)
    mesh_depth = torch.tensor([[1.0, 2.0, 0.0], [0.0, 4.0, 5.0]], device=DEV)
    field_depth = torch.tensor([[1.5, 2.0, 9.0], [3.0, 3.0, 9.0]], device=DEV)
    acc = torch.tensor([[0.9, 0.5, 0.8], [0.1, 1.0, 0.49]], device=DEV)
    got = HN.depth_agreement(mesh_depth, face, field_depth.view(-1), acc)
    assert all(v.is_cuda and v.dim() == 0 for v in got.values())
    assert int(got["n"]) == 3 and float(got["abs_mean"]) == pytest.approx(0.5)
    assert float(got["rmse"]) == pytest.approx(np.sqrt(1.25 / 3)) and float(got["iou"]) == pytest.approx(3 / 5)


def test_mesh_depth_error_is_depth_agreement_of_both_renderers():
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    HN.set_precision("fp32")
    model = NerfModel(EMB, n_samples_coarse=16, n_samples_fine=16, noise_std=None, view_fourier_dim=6,
                      hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True)
    load_hash(model, 7)
    model = model.to(DEV).eval()
    model.use_stratified_sampling = False
    wh = (24, 18)
    cam = torch.from_numpy(S.camera("plain", wh)).to(DEV)
    rays = F.generate_rays_nerfies(wh[1], wh[0], cam, 2.0, 4.5, image_id=3)
    mesh = gpu_mesh("sphere9")
    field = inference.render_image(model, rays, chunk=200, keys=("depth", "acc"))
    seen = HN.render_mesh(mesh, rays, cam, wh)
    acc_min = float(field["acc"].median())            # an untrained field: split its pixels so that both sides are non-empty
    for kw in (dict(), dict(acc_min=acc_min)):
        got = HN.mesh_depth_error(model, mesh, rays, cam, wh, chunk=200, **kw)
        want = HN.depth_agreement(seen["depth"], seen["face"], field["depth"], field["acc"], **kw)
        assert set(got) == {"abs_mean", "rmse", "iou", "n"}
        for k in got:
            assert torch.equal(got[k], want[k]) or (torch.isnan(got[k]) and torch.isnan(want[k])), k
    assert 0 < int(want["n"]) < wh[0] * wh[1] and float(want["rmse"]) >= float(want["abs_mean"]) > 0


def test_mesh_turntable_writes_the_orbit_as_a_gif(tmp_path):
    base = gpu_mesh("sphere17")
    mesh = dict(base, colors=torch.from_numpy(colours(base["vertices"].shape[0], "uint8")).to(DEV))
    path, wh, n = os.path.join(tmp_path, "turntable.gif"), (40, 30), 5
    cams = HN.mesh_turntable(mesh, path, n=n, image_wh=wh, elevation=15.0, background=(0.0, 0.0, 0.2))
    assert cams.shape == (n, 24)
    gif = inference.read_gif(path)
    assert len(gif["frames"]) == n and all(f.shape == (wh[1], wh[0], 3) for f in gif["frames"])
    frames = []
    for rec in cams:
        cam = torch.from_numpy(rec).to(DEV)
        extent = np.linalg.norm(rec[9:12].astype(np.float64) - S.SPHERE_CENTRE)
        img = HN.render_mesh(mesh, HN.camera_rays(cam, wh[0], wh[1], 0.0, 2 * extent), cam, wh, background=(0.0, 0.0, 0.2))
        assert (img["face"] >= 0).float().mean() > 0.1, "the mesh is in every frame"
        frames.append(img["rgb8"])
    palettes, indices = inference.quantize_frames(frames, "global")
    assert np.array_equal(gif["frames"][0], palettes[0].numpy()[indices[0].numpy()])
    assert not np.array_equal(gif["frames"][0], gif["frames"][2])


def test_camera_from_c2w_and_the_dataset_rays_agree_on_the_gpu():
    h, w, focal = 37, 50, 41.5
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
    c2w = torch.from_numpy(np.concatenate([rot, [[0.3], [-0.2], [0.7]]], axis=1).astype(np.float32)).to(DEV)
    want = F.generate_rays(h, w, focal, c2w, near=0.5, far=4.0, ndc=False)
    got = HN.camera_rays(HN.camera_from_c2w(c2w, focal, w, h), w, h, 0.5, 4.0)
    assert got.is_cuda and got.shape == want.shape
    assert float((got - want).abs().max()) <= 2e-6
