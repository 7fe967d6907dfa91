"""Host tests of depth fusion (csrc/hn_fusion.hip, geometry.fuse_depth and friends), no GPU: the float32 restatement of the
definition (tests/tsdf_restated.py) against a float64 statement of the same rule, where the restated surface lies on the
closed-form sphere scene, argument validation of the public functions and the ops, and the binding's tables."""
import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import isosurface_restated as I
import tsdf_restated as T
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F

SPACING32 = 1.6 / 31


def test_float32_restatement_against_the_float64_statement():
    """16^3 lattice, 24 views of 32 x 32.  The weights are equal everywhere.  tsdf is compared at the lattice points none of
    whose views hangs, in float64, on less than 1e-4 (tsdf_restated._near_threshold): s within 1e-4 of -trunc, or u or v
    within 1e-4 of a pixel edge across which the outcome differs.  That last clause matters on this scene: lattice and
    cameras share their symmetry planes, so 5.2 % of the voxel-views project EXACTLY onto the central pixel edge of their
    image (the plane x = z for an azimuth of 45 degrees, and so on) — but the two pixels there are mirror images and hold
    the same depth, so the side float32 falls on changes nothing, and those points are compared like any other.  What
    remains excluded is 0.024 % of the voxel-views (cap: 2 %), 24 of the 4096 lattice points.
    Bound: the float32 tsdf differs from the float64 one by at most 3.8e-7 as measured with this NumPy and libm (s is a
    difference of two numbers near 3, each with up to 1.2e-7 of rounding, divided by trunc = 0.43; the running mean
    averages the views' errors instead of adding them); the assertion allows 4 times that, 1.6e-6, for other libm
    builds."""
    wh, shape = (32, 32), (16, 16, 16)
    cams, depths = T.sphere_scene(wh)
    zero = np.zeros(shape, dtype=np.float32)
    trunc = T.default_trunc(shape)
    d32, w32 = T.sphere_volume(16, wh)
    d64, w64, near = T.integrate(zero, zero, T.BOUNDS, cams, depths, trunc, dtype=np.float64, margin=1e-4)
    assert d32.dtype == np.float32 and w32.dtype == np.float32
    assert np.array_equal(w32.astype(np.float64), w64)
    share = near.sum() / (near.size * len(cams))
    clear = near == 0
    err = np.abs(d32.astype(np.float64) - d64)[clear].max()
    print(f"excluded voxel-views {share:.4%}, lattice points compared {clear.sum()} of {clear.size}, max |f32 - f64| {err:.3e}")
    assert share <= 0.02
    assert clear.sum() > 0.8 * clear.size
    assert err <= 1.6e-6
    assert (w64 > 0).all() and w64.max() < len(cams)      # every point is seen, none by the cameras it hides from


def test_restated_surface_lies_on_the_sphere():
    """32^3, 24 views of 64 x 64: the zero crossings of the restated lattice along all seven tetrahedron edge directions
    lie within 1.0 lattice spacing of the sphere (measured: 0.62 at most, 0.59 on the axis directions, as the float64
    prototype of the definition gave), and no crossing edge has a never-observed end."""
    d, w = T.sphere_volume(32, (64, 64))
    g = T.lattice(d, w)
    for dirs, count in ((I.DIRS[:3], 1656), (I.DIRS, None)):
        p, unseen = T.edge_crossings(g, w, T.BOUNDS, dirs)
        err = np.abs(np.linalg.norm(p, axis=1) - T.RADIUS) / SPACING32
        print(f"{len(dirs)} directions: {len(p)} crossings, max radial error {err.max():.3f} spacings")
        assert len(p) > 1000 and (count is None or len(p) == count)
        assert not unseen.any()
        assert err.max() <= 1.0


def test_restated_one_view_volume_has_frustum_walls_that_face_keep_removes():
    """One view (azimuth 0, elevation 0) at 32^3: 1568 axis crossings have a never-observed end, as the prototype found;
    the restated mesh has faces far from the sphere, and the faces face_keep keeps all lie within 1.5 spacings of it and
    are fewer than half."""
    d, w = T.sphere_volume(32, (64, 64), views=(T.FRONT_VIEW,))
    g = T.lattice(d, w)
    _, unseen = T.edge_crossings(g, w, T.BOUNDS, I.DIRS[:3])
    assert unseen.sum() == 1568
    mesh = I.extract_isosurface(g, 0.0, T.BOUNDS)
    fkeep, vkeep = T.face_keep(mesh["vertices"], mesh["faces"], w, T.BOUNDS)
    centroid = mesh["vertices"].astype(np.float64)[mesh["faces"]].mean(axis=1)
    err = np.abs(np.linalg.norm(centroid, axis=1) - T.RADIUS) / SPACING32
    assert err.max() > 3.0
    assert err[fkeep == 1].max() <= 1.5
    assert 0 < fkeep.sum() < 0.5 * len(fkeep)
    assert np.array_equal(np.flatnonzero(vkeep), np.unique(mesh["faces"][fkeep == 1]))
    # all 24 views: nothing is dropped
    d, w = T.sphere_volume(32, (64, 64))
    mesh = I.extract_isosurface(T.lattice(d, w), 0.0, T.BOUNDS)
    fkeep, vkeep = T.face_keep(mesh["vertices"], mesh["faces"], w, T.BOUNDS)
    assert fkeep.all() and vkeep.all()


def test_restated_depth_conventions():
    """+inf carves, anything not > 0 says nothing, a point behind the surface by more than trunc is left alone."""
    shape, wh = (5, 4, 3), (8, 6)
    bounds = (-0.5, 0.5, -0.4, 0.4, -0.3, 0.3)
    cam = HN.orbit_cameras((0.0, 0.0, 0.0), 3.0, 1, 0.0, focal=20.0, image_wh=wh)
    zero = np.zeros(shape, dtype=np.float32)
    for value, want_w, want_d in ((np.inf, 1.0, 1.0), (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (1.0, 0.0, 0.0),
                                  (6.0, 1.0, 1.0)):
        d, w = T.integrate(zero, zero, bounds, cam, np.full((1,) + wh[::-1], value, dtype=np.float32), 0.25)
        assert (w == want_w).all() and (d == want_d).all(), value
    d, w = T.integrate(zero, zero, bounds, cam, np.full((1,) + wh[::-1], 3.0, dtype=np.float32), 0.25)
    assert set(np.unique(w)) == {0.0, 1.0} and d.min() >= -1.0 and d.max() <= 1.0 and (d[w == 0] == 0).all()


# ---- argument validation, without a device ---------------------------------------------------------------------------------
CAMS = np.zeros((2, 24), dtype=np.float32)
B = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)


def depths(n=2, h=6, w=8, dtype=torch.float32):
    return torch.ones((n, h, w), dtype=dtype)


@pytest.mark.parametrize("kwargs, word", [
    (dict(depths=torch.ones((2, 6))), "depths"),
    (dict(depths=depths(dtype=torch.float64)), "depths"),
    (dict(depths=np.ones((2, 6, 8), dtype=np.float32)), "depths"),
    (dict(cameras=np.zeros((2, 23), dtype=np.float32)), "cameras"),
    (dict(cameras=np.zeros((2, 24), dtype=np.float64)), "cameras"),
    (dict(cameras=np.zeros((3, 24), dtype=np.float32)), "cameras"),
    (dict(cameras=np.zeros((0, 24), dtype=np.float32), depths=depths(0)), "cameras"),
    (dict(bounds=(-1.0, 1.0, -1.0, 1.0, 1.0, 1.0)), "bounds"),
    (dict(bounds=(-1.0, 1.0, -1.0, 1.0)), "bounds"),
    (dict(resolution=1), "at least 2"),
    (dict(resolution=(4, 4)), "three sides"),
    (dict(trunc=0.0), "trunc"),
    (dict(trunc=-0.1), "trunc"),
    (dict(trunc=float("inf")), "trunc"),
    (dict(trunc=float("nan")), "trunc"),
    (dict(ndc=True), "NDC"),
    (dict(volume={"tsdf": torch.zeros((4, 4, 4))}), "volume"),
    (dict(volume={"tsdf": torch.zeros((4, 4, 5)), "weight": torch.zeros((4, 4, 5))}), "shape"),
    (dict(volume={"tsdf": torch.zeros((4, 4, 4)), "weight": torch.zeros((4, 4, 4), dtype=torch.float64)}), "float32"),
    (dict(volume={"tsdf": torch.zeros((4, 4, 4)), "weight": torch.zeros((4, 4, 8))[:, :, ::2]}), "contiguous"),
    (dict(), "GPU"),          # everything in order, but on the host
])
def test_fuse_depth_refuses(kwargs, word):
    args = dict(depths=depths(), cameras=CAMS, bounds=B, resolution=4)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        HN.fuse_depth(**args)


class NoModel:
    def parameters(self):
        raise AssertionError("the arguments are checked before the model is touched")


@pytest.mark.parametrize("kwargs, word", [
    (dict(cameras=np.zeros((24,), dtype=np.float32)), "cameras"),
    (dict(cameras=np.zeros((2, 24), dtype=np.float64)), "cameras"),
    (dict(image_wh=(8,)), "image_wh"),
    (dict(image_wh=(0, 6)), "image sides"),
    (dict(image_wh=(8, 65536)), "image sides"),
    (dict(acc_min=0.05, acc_free=0.5), "thresholds"),
    (dict(acc_min=0.3, acc_free=0.3), "thresholds"),
    (dict(acc_free=-0.1), "thresholds"),
    (dict(acc_min=1.5), "thresholds"),
    (dict(ndc=True), "NDC"),
])
def test_depth_images_from_field_refuses(kwargs, word):
    args = dict(model=NoModel(), cameras=CAMS, image_wh=(8, 6), frame_id=0, near=0.1, far=4.0)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        HN.depth_images_from_field(**args)


@pytest.mark.parametrize("volume, word", [
    (None, "volume"),
    ({"tsdf": torch.zeros((4, 4, 4))}, "volume"),
    ({"tsdf": torch.zeros((4, 4)), "weight": torch.zeros((4, 4))}, "tsdf"),
    ({"tsdf": torch.zeros((4, 4, 4)), "weight": torch.zeros((4, 4, 3))}, "weight"),
    ({"tsdf": torch.zeros((4, 4, 4), dtype=torch.float16), "weight": torch.zeros((4, 4, 4))}, "float32"),
    ({"tsdf": torch.zeros((4, 4, 1)), "weight": torch.zeros((4, 4, 1))}, "at least 2"),
    ({"tsdf": torch.zeros((4, 4, 4)), "weight": torch.zeros((4, 4, 4))}, "GPU"),
])
def test_tsdf_isosurface_refuses(volume, word):
    with pytest.raises(ValueError, match=word):
        HN.tsdf_isosurface(volume, B)
    if volume is not None and word == "GPU":
        with pytest.raises(ValueError, match="bounds"):
            HN.tsdf_isosurface(volume, (0.0, 0.0, 0.0, 1.0, 0.0, 1.0))


@pytest.mark.parametrize("kwargs, word", [
    (dict(simplify=-1.0), "simplify"),
    (dict(simplify=(1.0, 2.0)), "simplify"),
    (dict(ndc=True), "NDC"),
    (dict(acc_min=0.1, acc_free=0.2), "thresholds"),
    (dict(image_wh=(8, 0)), "image sides"),
])
def test_extract_mesh_fused_refuses(kwargs, word):
    args = dict(model=NoModel(), bounds=B, resolution=4, frame_id=0, cameras=CAMS, image_wh=(8, 6), near=0.1, far=4.0)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        HN.extract_mesh_fused(**args)


def test_extract_mesh_fused_has_no_iso():
    with pytest.raises(TypeError, match="iso"):
        HN.extract_mesh_fused(NoModel(), B, 4, 0, CAMS, (8, 6), 0.1, 4.0, iso=10.0)


@pytest.mark.parametrize("kwargs, word", [
    (dict(tsdf=torch.zeros((4, 4))), "tsdf"),
    (dict(tsdf=torch.zeros((4, 4, 4), dtype=torch.float64)), "tsdf"),
    (dict(weight=torch.zeros((4, 4, 5))), "weight"),
    (dict(weight=torch.zeros((4, 4, 8))[:, :, ::2]), "weight"),
    (dict(bounds=(0.0, 1.0, 0.0, 1.0, 0.0, -1.0)), "bounds"),
    (dict(cams=torch.zeros((2, 23))), "cams"),
    (dict(cams=torch.zeros((24,))), "cams"),
    (dict(cams=torch.zeros((0, 24)), depths=depths(0)), "cams"),
    (dict(cams=torch.zeros((3, 24))), "depths"),
    (dict(depths=depths(dtype=torch.float16)), "depths"),
    (dict(depths=torch.ones((2, 6, 0))), "image sides"),
    (dict(trunc=0.0), "trunc"),
    (dict(trunc=float("nan")), "trunc"),
    (dict(trunc="wide"), "trunc"),
    (dict(), "GPU"),
])
def test_tsdf_integrate_refuses(kwargs, word):
    args = dict(tsdf=torch.zeros((4, 4, 4)), weight=torch.zeros((4, 4, 4)), bounds=B, cams=torch.zeros((2, 24)),
                depths=depths(), trunc=0.5)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        F.tsdf_integrate(**args)


@pytest.mark.parametrize("kwargs, word", [
    (dict(vertices=torch.zeros((5, 2))), "vertices"),
    (dict(vertices=torch.zeros((5, 3), dtype=torch.float64)), "vertices"),
    (dict(faces=torch.zeros((2, 3), dtype=torch.int64)), "faces"),
    (dict(faces=torch.zeros((2, 4), dtype=torch.int32)), "faces"),
    (dict(weight=torch.zeros((4, 4))), "weight"),
    (dict(weight=torch.zeros((4, 4, 4), dtype=torch.int32)), "weight"),
    (dict(bounds=(0.0, 1.0)), "bounds"),
    (dict(), "GPU"),
])
def test_tsdf_face_keep_refuses(kwargs, word):
    args = dict(vertices=torch.zeros((5, 3)), faces=torch.zeros((2, 3), dtype=torch.int32), weight=torch.zeros((4, 4, 4)),
                bounds=B)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        F.tsdf_face_keep(**args)


def test_binding_and_exports():
    names = {"hn_tsdf_integrate", "hn_tsdf_face_keep"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES) and "hn_fusion.hip" in L.SOURCES
    assert "hn_camera.h" in L.CSRC_HEADERS
    assert len(L.ARGTYPES["hn_tsdf_integrate"]) == 13 and len(L.ARGTYPES["hn_tsdf_face_keep"]) == 12
    for name in ("tsdf_integrate", "tsdf_face_keep"):
        assert name in HN.ops.mesh.__all__ and getattr(F, name) is getattr(HN.ops.mesh, name)
    for name in ("fuse_depth", "depth_images_from_field", "tsdf_isosurface", "extract_mesh_fused"):
        assert getattr(HN, name) is getattr(HN.geometry, name)
    assert "hn_fusion.hip" in HN.ops.__doc__


def test_extract_mesh_keeps_its_tail(monkeypatch):
    """extract_mesh and extract_mesh_fused go through one tail: filter, simplify in lattice spacings, colours."""
    calls = []
    mesh = {"vertices": torch.zeros((3, 3)), "normals": torch.zeros((3, 3)), "faces": torch.zeros((1, 3), dtype=torch.int32)}
    G = HN.geometry
    monkeypatch.setattr(G, "density_grid", lambda *a, **k: calls.append(("grid", k)) or "grid")
    monkeypatch.setattr(G, "extract_isosurface", lambda g, iso, b: calls.append(("iso", iso)) or dict(mesh))
    monkeypatch.setattr(G, "depth_images_from_field", lambda *a, **k: calls.append(("depths", k)) or "depths")
    monkeypatch.setattr(G, "fuse_depth", lambda *a, **k: calls.append(("fuse", a[4])) or "volume")
    monkeypatch.setattr(G, "tsdf_isosurface", lambda v, b: calls.append(("tsdf_iso", v)) or dict(mesh))
    monkeypatch.setattr(G, "filter_mesh", lambda m, min_faces, keep_largest: calls.append(("filter", min_faces, keep_largest)) or m)
    monkeypatch.setattr(G, "simplify_mesh", lambda m, cell, origin: calls.append(("simplify", cell, origin)) or m)
    monkeypatch.setattr(G, "vertex_colors", lambda model, v, n, fid, view, **k: calls.append(("colors", view, k)) or "colors")
    out = G.extract_mesh("model", B, 5, 3, iso=2.0, colors="normal", min_faces=7, keep_largest=1, simplify=2, chunk=99)
    assert out["colors"] == "colors"
    assert calls == [("grid", {"chunk": 99}), ("iso", 2.0), ("filter", 7, 1), ("simplify", [1.0, 1.0, 1.0], (-1.0, -1.0, -1.0)),
                     ("colors", "normal", {"chunk": 99})]
    del calls[:]
    out = G.extract_mesh_fused("model", B, 5, 3, CAMS, (8, 6), 0.1, 4.0, trunc=0.3, keep_largest=1, simplify=2, chunk=99,
                               acc_min=0.7)
    assert "colors" not in out
    assert calls == [("depths", {"chunk": 99, "acc_min": 0.7}), ("fuse", 0.3), ("tsdf_iso", "volume"), ("filter", None, 1),
                     ("simplify", [1.0, 1.0, 1.0], (-1.0, -1.0, -1.0))]
