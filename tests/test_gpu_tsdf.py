"""GPU tests of depth fusion (csrc/hn_fusion.hip, geometry.fuse_depth / tsdf_isosurface / depth_images_from_field /
extract_mesh_fused) against the NumPy float32 restatement of its definition (tests/tsdf_restated.py): the volumes and the
face filter bit for bit, the fused surface of the closed-form sphere scene, the frustum walls of a single view, the
field path through a stub model, and the error returns.  Restated volumes are computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import isosurface_restated as I
import mesh_render_restated as R
import tsdf_restated as T
from gpu_common import DEV
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F

pytestmark = pytest.mark.gpu

WH = (64, 64)
SPACING32 = 1.6 / 31


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the shared scene arrays are read-only


def radial_error(points, radius=T.RADIUS, spacing=SPACING32):
    p = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points
    return np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - radius) / spacing


@functools.lru_cache(maxsize=None)
def fused_sphere(res, wh, views=None):
    cams, depths = T.sphere_scene(wh)
    if views is not None:
        cams, depths = cams[list(views)], depths[list(views)]
    return HN.fuse_depth(gpu(depths), cams, T.BOUNDS, res)


# ---- 1. bits against the restatement ---------------------------------------------------------------------------------------
ODD_SHAPE = (12, 10, 9)
ODD_BOUNDS = (-0.8, 0.6, -0.5, 0.7, -0.4, 0.5)
ODD_WH = (20, 14)
ODD_CENTRE = (0.0, 0.05, 0.0)
ODD_TRUNC = 0.3


@functools.lru_cache(maxsize=None)
def odd_scene():
    """Five cameras of 20 x 14 pixels around a lattice that is no multiple of any brick or block: two orbit cameras, a
    Nerfies-style record with skew, aspect and all five distortion coefficients, one inside the volume (lattice points lie
    behind it), one that looks mostly past the volume; sphere depths salted with +inf, 0, -1 and NaN pixels."""
    w, h = ODD_WH
    orbit = HN.orbit_cameras(ODD_CENTRE, 3.0, 5, 20.0, focal=22.0, image_wh=ODD_WH)[[1, 3]]
    cams = np.stack([orbit[0], orbit[1],
                     R.record((0.1, -0.05, -3.0), 24.0, w / 2 + 0.3, h / 2 - 0.2, aspect=1.1, skew=0.2, k=(-0.2, 0.05, 0.01),
                              p=(0.002, -0.003)),
                     R.record((0.05, 0.02, 0.0), 5.0, w / 2, h / 2),
                     R.record((2.5, 0.1, -3.0), 14.0, w / 2, h / 2)])
    depths = np.stack([T.sphere_depth(rec, ODD_WH, radius=0.4, centre=ODD_CENTRE) for rec in cams])
    rng = np.random.RandomState(7)
    for value in (np.inf, 0.0, -1.0, np.nan):
        depths[rng.randint(0, 5, 12), rng.randint(0, h, 12), rng.randint(0, w, 12)] = value
    return cams.astype(np.float32), depths.astype(np.float32)


@functools.lru_cache(maxsize=None)
def odd_restated():
    cams, depths = odd_scene()
    zero = np.zeros(ODD_SHAPE, dtype=np.float32)
    return T.integrate(zero, zero, ODD_BOUNDS, cams, depths, ODD_TRUNC)


def odd_gpu(batches):
    cams, depths = odd_scene()
    volume = None
    for rows in batches:
        volume = HN.fuse_depth(gpu(depths[rows]), cams[rows], ODD_BOUNDS, ODD_SHAPE, trunc=ODD_TRUNC, volume=volume)
    return volume


def test_volumes_equal_the_restatement_bit_for_bit():
    cams, depths = odd_scene()
    want_d, want_w = odd_restated()
    # the scene does exercise the rule: every weight from 0 to 5 but one or two, both signs, the free-space cap
    assert len(np.unique(want_w)) >= 4 and want_w.min() == 0 and (want_d < 0).any() and (want_d == 1).any()
    x, y, z = T.lattice_xyz(ODD_SHAPE, ODD_BOUNDS)
    assert (T.project(cams[3], x, y, z)[2] == 1).any(), "lattice points behind the camera inside the volume"
    u = T.project(cams[4], x, y, z)[0]
    assert (u < 0).mean() > 0.5 and (u > 0).any(), "the fifth camera looks mostly past the volume"
    got = odd_gpu([slice(0, 5)])
    assert got['tsdf'].shape == ODD_SHAPE and got['tsdf'].dtype == torch.float32 and got['tsdf'].device == torch.device(DEV)
    assert same_bits(got['weight'], want_w), "weight differs from the restatement"
    assert same_bits(got['tsdf'], want_d), "tsdf differs from the restatement"


def test_batches_and_a_second_run_give_the_same_bits():
    want_d, want_w = odd_restated()
    split = odd_gpu([slice(0, 3), slice(3, 5)])
    assert same_bits(split['tsdf'], want_d) and same_bits(split['weight'], want_w)
    again = odd_gpu([slice(0, 5)])
    assert same_bits(again['tsdf'], want_d) and same_bits(again['weight'], want_w)


def test_lattice_positions_are_those_of_grid_points():
    """The restatement takes its positions from isosurface_restated.lattice_points: those are hn_grid_points' bits, so the
    bit identity above also says the kernel computes where hn_grid_points puts the lattice."""
    pts = F.grid_points(ODD_SHAPE, ODD_BOUNDS, 0, int(np.prod(ODD_SHAPE)), DEV).cpu().numpy()
    assert same_bits(pts, I.lattice_points(ODD_SHAPE, ODD_BOUNDS))


# ---- 2. the face filter ----------------------------------------------------------------------------------------------------
def test_face_keep_equals_its_restatement():
    volume = fused_sphere(24, (48, 48), views=(T.FRONT_VIEW,))
    d, w = T.sphere_volume(24, (48, 48), views=(T.FRONT_VIEW,))
    assert same_bits(volume['tsdf'], d) and same_bits(volume['weight'], w)
    mesh = HN.tsdf_isosurface(volume, T.BOUNDS, observed_only=False)
    fkeep, vkeep = F.tsdf_face_keep(mesh['vertices'], mesh['faces'], volume['weight'], T.BOUNDS)
    want_f, want_v = T.face_keep(mesh['vertices'].cpu().numpy(), mesh['faces'].cpu().numpy(), w, T.BOUNDS)
    assert fkeep.dtype == torch.int32 and vkeep.dtype == torch.int32
    assert 0 < want_f.sum() < len(want_f) and 0 < want_v.sum() < len(want_v)
    assert same_bits(fkeep, want_f) and same_bits(vkeep, want_v)
    # a face with an id outside the mesh is dropped, and nothing is written for it
    faces = mesh['faces'].clone()
    faces[0, 1] = mesh['vertices'].shape[0]
    faces[1, 2] = -1
    fkeep2, vkeep2 = F.tsdf_face_keep(mesh['vertices'], faces, volume['weight'], T.BOUNDS)
    want_f2, want_v2 = T.face_keep(mesh['vertices'].cpu().numpy(), faces.cpu().numpy(), w, T.BOUNDS)
    assert fkeep2[:2].tolist() == [0, 0] and same_bits(fkeep2, want_f2) and same_bits(vkeep2, want_v2)


# ---- 3. the sphere from 24 views ----------------------------------------------------------------------------------------------
def test_fused_sphere_lies_on_the_sphere_closed_and_outward():
    volume = fused_sphere(32, WH)
    d, w = T.sphere_volume(32, WH)
    assert same_bits(volume['tsdf'], d) and same_bits(volume['weight'], w)
    mesh = HN.tsdf_isosurface(volume, T.BOUNDS)
    raw = HN.tsdf_isosurface(volume, T.BOUNDS, observed_only=False)
    v, n, f = (mesh[k].cpu().numpy() for k in ('vertices', 'normals', 'faces'))
    err = radial_error(v)
    print(f"fused sphere: {len(v)} vertices, {len(f)} faces, max radial error {err.max():.3f} spacings")
    assert len(v) > 1000 and err.max() <= 1.0
    check = I.check_mesh(v, f)
    assert check["closed"] and check["oriented"] and check["euler"] == 2 and check["volume"] > 0
    assert ((n * v).sum(axis=1) > 0).all()
    # observed_only drops no face here
    assert torch.equal(mesh['faces'], raw['faces']) and torch.equal(mesh['vertices'], raw['vertices'])
    assert torch.equal(mesh['vertex_index'], torch.arange(len(v), dtype=torch.int32, device=DEV))


def agreement_numpy(mesh_depth, mesh_face, field_depth):
    both = (mesh_face >= 0) & np.isfinite(field_depth)
    union = (mesh_face >= 0) | np.isfinite(field_depth)
    err = np.where(both, mesh_depth.astype(np.float64) - np.where(both, field_depth, 0).astype(np.float64), 0.0)
    return {"abs_mean": np.abs(err).sum() / both.sum(), "iou": both.sum() / union.sum(), "n": int(both.sum())}


def test_fused_sphere_renders_back_to_its_depth_images():
    """render_mesh's depth of the fused mesh against the depth images it was fused from, through depth_agreement: what the
    GPU reports equals, to 1e-6, what the restated lattice gives on the CPU (marching tetrahedra and the ray caster
    restated in NumPy), on the central 32 x 32 pixels (the sphere's image and a rim of sky) of one camera per elevation."""
    cams, depths = T.sphere_scene(WH)
    d, w = T.sphere_volume(32, WH)
    host = I.extract_isosurface(T.lattice(d, w), 0.0, T.BOUNDS)
    mesh = HN.tsdf_isosurface(fused_sphere(32, WH), T.BOUNDS)
    for view in (1, 12, 22):
        cam = gpu(cams[view])
        rays = HN.camera_rays(cam, WH[0], WH[1], 0.0, 6.0)
        pick = np.zeros((WH[1], WH[0]), dtype=bool)
        pick[16:48, 16:48] = True
        pick = pick.reshape(-1)
        want = R.cast(host["vertices"], host["faces"], rays.cpu().numpy()[pick])
        want = agreement_numpy(want["depth"], want["face"], depths[view].reshape(-1)[pick])
        seen = HN.render_mesh(mesh, rays, cam, WH, shading='none')
        field = gpu(depths[view]).reshape(-1)
        sel = gpu(pick)
        got = HN.depth_agreement(seen['depth'].reshape(-1)[sel], seen['face'].reshape(-1)[sel],
                                 torch.where(torch.isfinite(field), field, torch.zeros_like(field))[sel],
                                 torch.isfinite(field).float()[sel])
        print(f"view {view}: iou {want['iou']:.6f}, abs_mean {want['abs_mean']:.6f} over {want['n']} pixels")
        assert int(got['n']) == want['n'] and want['n'] > 200
        assert abs(float(got['iou']) - want['iou']) <= 1e-6
        assert abs(float(got['abs_mean']) - want['abs_mean']) <= 1e-6


# ---- 4. one view: frustum walls and the filter ----------------------------------------------------------------------------
def test_one_view_the_filter_removes_the_frustum_walls():
    volume = fused_sphere(32, WH, views=(T.FRONT_VIEW,))
    raw = HN.tsdf_isosurface(volume, T.BOUNDS, observed_only=False)
    kept = HN.tsdf_isosurface(volume, T.BOUNDS)

    def centroid_error(mesh):
        v = mesh['vertices'].cpu().numpy().astype(np.float64)
        return radial_error(v[mesh['faces'].cpu().numpy()].mean(axis=1))

    assert centroid_error(raw).max() > 3.0
    assert kept['faces'].shape[0] > 0 and centroid_error(kept).max() <= 1.5
    assert kept['faces'].shape[0] < 0.5 * raw['faces'].shape[0]
    index = kept['vertex_index'].long()
    assert kept['vertex_index'].dtype == torch.int32 and (index[1:] > index[:-1]).all()
    assert torch.equal(kept['vertices'], raw['vertices'][index]) and torch.equal(kept['normals'], raw['normals'][index])
    assert int(kept['faces'].max()) < kept['vertices'].shape[0] and int(kept['faces'].min()) == 0


# ---- 5. the field path, with a stub in the field's place ---------------------------------------------------------------------
class SphereField(torch.nn.Module):
    """What inference.render_image needs of a model: forward(ray_dict, extra) -> {level: {'depth', 'acc'}} of the analytic
    sphere: acc 1 and the distance on a hit, acc 0 on a miss, and acc 0.3 in a ring around the silhouette (the closest
    approach of the ray lies within 1.15 radii)."""
    RING = 1.15

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.frame_ids = set()

    def forward(self, ray_dict, extra):
        o, d = ray_dict["origins"].double(), ray_dict["directions"].double()
        self.frame_ids.update(ray_dict["metadata"]["warp"].reshape(-1).unique().tolist())
        b = (o * d).sum(-1)
        closest = torch.sqrt(((o - b[:, None] * d) ** 2).sum(-1))
        disc = b * b - ((o * o).sum(-1) - T.RADIUS ** 2)
        hit = disc >= 0
        t = -b - torch.sqrt(torch.where(hit, disc, torch.zeros_like(disc)))
        ring = ~hit & (closest <= self.RING * T.RADIUS)
        acc = hit.float() + 0.3 * ring.float()
        depth = (torch.where(hit, t, torch.zeros_like(b)) + 0.3 * torch.where(ring, -b, torch.zeros_like(b))).float()
        return {level: {"depth": depth, "acc": acc} for level in ("coarse", "fine")}


def test_depth_images_from_a_field_and_the_fused_mesh():
    model = SphereField().to(DEV)
    cams, depths = T.sphere_scene(WH)
    got = HN.depth_images_from_field(model, cams, WH, 17, 0.0, 6.0, chunk=1000)
    assert got.shape == (24, WH[1], WH[0]) and got.dtype == torch.float32 and got.device == torch.device(DEV)
    assert model.frame_ids == {17}
    got = got.cpu().numpy()

    def classes(view):
        """(hit, ring, free) pixel masks of the closed form; pixels whose ray passes within 1e-3 radii of either rim are in
        none of them (fp32 rays against float64 ones)."""
        rays = T.host_rays(cams[view], WH)
        o, dd = rays[:, 0:3], rays[:, 3:6]
        b = (o * dd).sum(-1)
        closest = np.linalg.norm(o - b[:, None] * dd, axis=1).reshape(WH[1], WH[0]) / T.RADIUS
        sure = (np.abs(closest - 1.0) > 1e-3) & (np.abs(closest - SphereField.RING) > 1e-3)
        return (closest < 1) & sure, (closest > 1) & (closest < SphereField.RING) & sure, (closest > SphereField.RING) & sure

    for view in (0, 13):
        hit, ring, free = classes(view)
        assert hit.sum() > 100 and ring.sum() > 20 and free.sum() > 100
        assert np.isinf(got[view][free]).all() and (got[view][ring] == 0).all()
        assert np.abs(got[view][hit] - depths[view][hit]).max() <= 1e-4
    # the thresholds are the caller's: with acc_min = 0.2 the ring is surface, and without `normalize` at depth, not depth / acc
    hit, ring, free = classes(0)
    loose = HN.depth_images_from_field(model, cams[:1], WH, 17, 0.0, 6.0, acc_min=0.2, normalize=False)[0].cpu().numpy()
    assert np.isinf(loose[free]).all() and np.abs(loose[hit] - depths[0][hit]).max() <= 1e-4
    assert (loose[ring] > 0.5).all() and (loose[ring] < 1.0).all()          # 0.3 times a distance near 3
    mesh = HN.extract_mesh_fused(model, T.BOUNDS, 32, 17, cams, WH, 0.0, 6.0, keep_largest=1, simplify=2, colors=None)
    assert 'vertex_cluster' in mesh and 'colors' not in mesh
    v, f = mesh['vertices'].cpu().numpy(), mesh['faces'].cpu().numpy()
    err = radial_error(v)
    print(f"extract_mesh_fused: {len(v)} vertices, {len(f)} faces, max radial error {err.max():.3f} spacings")
    assert len(f) > 500 and err.max() <= 1.0
    plain = HN.extract_mesh_fused(model, T.BOUNDS, 32, 17, cams, WH, 0.0, 6.0)
    assert plain['faces'].shape[0] > 2 * len(f) and radial_error(plain['vertices']).max() <= 1.0
    assert I.check_mesh(plain['vertices'].cpu().numpy(), plain['faces'].cpu().numpy())["closed"]


# ---- 6. error paths ---------------------------------------------------------------------------------------------------------
def test_error_returns_reach_python_without_a_launch():
    shape, b6 = (4, 5, 6), (C.c_float * 6)(*T.BOUNDS)
    tsdf, weight = (torch.zeros(shape, device=DEV) for _ in range(2))
    cams, depths = gpu(np.zeros((2, 24), dtype=np.float32)), torch.ones((2, 6, 8), device=DEV)
    stream = L.stream_handle()
    L.load()

    def integrate(**kw):
        a = dict(tsdf=L.ptr(tsdf), weight=L.ptr(weight), nx=4, ny=5, nz=6, bounds=b6, cams=L.ptr(cams), depths=L.ptr(depths),
                 n=2, h=6, w=8, trunc=0.5)
        a.update(kw)
        L.launch("hn_tsdf_integrate", a["tsdf"], a["weight"], a["nx"], a["ny"], a["nz"], a["bounds"], a["cams"], a["depths"],
                 a["n"], a["h"], a["w"], a["trunc"], stream)

    for kw in (dict(tsdf=None), dict(weight=None), dict(cams=None), dict(depths=None)):
        with pytest.raises(L.HnError, match="argument error -3"):
            integrate(**kw)
    for kw in (dict(bounds=None), dict(n=0), dict(h=0), dict(w=65536), dict(nx=1), dict(nx=700, ny=700, nz=700),
               dict(bounds=(C.c_float * 6)(0, 1, 0, 1, 1, 1)), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("inf")),
               dict(trunc=float("nan"))):
        with pytest.raises(L.HnError, match="argument error -2"):
            integrate(**kw)
    faces, vertices = torch.zeros((3, 3), dtype=torch.int32, device=DEV), torch.zeros((4, 3), device=DEV)
    fkeep, vkeep = torch.full((3,), 7, dtype=torch.int32, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV)

    def face_keep(**kw):
        a = dict(faces=L.ptr(faces), f=3, vertices=L.ptr(vertices), v=4, weight=L.ptr(weight), nx=4, ny=5, nz=6, bounds=b6,
                 fkeep=L.ptr(fkeep), vkeep=L.ptr(vkeep))
        a.update(kw)
        L.launch("hn_tsdf_face_keep", a["faces"], a["f"], a["vertices"], a["v"], a["weight"], a["nx"], a["ny"], a["nz"],
                 a["bounds"], a["fkeep"], a["vkeep"], stream)

    for kw in (dict(faces=None), dict(vertices=None), dict(weight=None), dict(fkeep=None), dict(vkeep=None)):
        with pytest.raises(L.HnError, match="argument error -3"):
            face_keep(**kw)
    for kw in (dict(f=0), dict(f=2 ** 31), dict(v=0), dict(v=-1), dict(nz=1), dict(bounds=None)):
        with pytest.raises(L.HnError, match="argument error -2"):
            face_keep(**kw)
    # the host layer refuses before the binding is reached
    with pytest.raises(ValueError, match="trunc"):
        F.tsdf_integrate(tsdf, weight, T.BOUNDS, cams, depths, 0.0)
    with pytest.raises(ValueError, match="depths"):
        F.tsdf_integrate(tsdf, weight, T.BOUNDS, cams, depths[:1], 0.5)
    with pytest.raises(ValueError, match="one device|GPU"):
        F.tsdf_integrate(tsdf, weight, T.BOUNDS, cams.cpu(), depths, 0.5)
    with pytest.raises(ValueError, match="shape"):
        HN.fuse_depth(depths, cams, T.BOUNDS, (4, 5, 7), volume={'tsdf': tsdf, 'weight': weight})
    torch.cuda.synchronize()
    assert not tsdf.any() and not weight.any() and (fkeep == 7).all() and (vkeep == 7).all(), "nothing was launched"
