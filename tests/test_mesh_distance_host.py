"""Host tests of the mesh distance (csrc/hn_mesh_distance.hip, geometry.sample_surface / point_mesh_distance /
mesh_distance), no GPU: the float32 restatement of the definition (tests/mesh_distance_restated.py) against float64 and
against closed forms, the sampling statistics of the restated sampler, the argument checks, the binding."""
import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import geometry as G

import mesh_distance_restated as R

F32 = np.float32
REFUSED = (ValueError, L.HnError)      # an argument error, or "needs the GPU", before any launch


def _mesh(v, f):
    return {'vertices': torch.from_numpy(np.ascontiguousarray(v, dtype=F32)), 'faces': torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32))}


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def test_fp32_distance_against_float64():
    """The float32 restatement against the float64 brute force: the 320-face unit icosphere, 300 hash-drawn points in
    [-1.5, 1.5]^3.  Measured: the largest distance error is 1.09e-7, about one ulp of the coordinates; the bound is
    8 * 2^-24 * 1.5 = 7.2e-7, a handful of roundings between coordinates of size <= 1.5 and the distance."""
    v, f = R.icosphere(2)
    assert f.shape == (320, 3)
    p = R.hash_points(7, 300)
    assert p.min() >= -1.5 and p.max() < 1.5
    lo, hi = R.point_mesh_distance(p, v, f), R.point_mesh_distance(p, v, f, dtype=np.float64)
    err = np.abs(lo['distance'].astype(np.float64) - hi['distance']).max()
    print(f"max |fp32 - fp64| distance = {err:.3e}")
    assert lo['distance'].dtype == F32 and hi['distance'].dtype == np.float64
    assert err < 8 * 2.0 ** -24 * 1.5
    assert np.abs(lo['closest'].astype(np.float64) - p).max() > 0.0 and np.isfinite(lo['closest']).all()


def test_concentric_cubes_are_exact():
    """Cubes of half-side 0.5 and 0.75: an inner vertex is 0.25 from three sides of the outer cube — six faces tie and
    the smallest id wins; an outer vertex is sqrt(3) * 0.25 from the inner cube's corner.  Both squares are exact in fp32."""
    (vi, fi), (vo, fo) = R.cube(0.5), R.cube(0.75)
    r = R.point_mesh_distance(vi, vo, fo)
    assert (r['distance'] * r['distance'] == F32(0.0625)).all() and (r['distance'] == F32(0.25)).all()
    _, d2 = R.closest_point(vi[7], vo[fo[:, 0]], vo[fo[:, 1]], vo[fo[:, 2]])
    assert (d2 == F32(0.0625)).sum() == 6 and d2.min() == F32(0.0625)
    assert r['face'][7] == 0 and (r['closest'][7] == np.array([0.75, 0.5, 0.5], dtype=F32)).all()
    r = R.point_mesh_distance(vo, vi, fi)
    _, d2 = R.closest_point(vo[:, None, :], vi[fi[:, 0]][None], vi[fi[:, 1]][None], vi[fi[:, 2]][None])
    assert (d2.min(axis=1) == F32(0.1875)).all()
    assert (r['distance'] == np.sqrt(F32(0.1875))).all() and (r['closest'] == vi).all()


@pytest.mark.parametrize("point, foot", [
    ((-1, -1, 1), (0, 0, 0)),          # vertex A
    ((6, -1, 2), (4, 0, 0)),           # vertex B
    ((-1, 6, -2), (0, 4, 0)),          # vertex C
    ((1, -3, 1), (1, 0, 0)),           # edge AB
    ((-2, 3, 0.5), (0, 3, 0)),         # edge AC
    ((4, 4, 3), (2, 2, 0)),            # edge BC
    ((1, 2, -5), (1, 2, 0)),           # interior
])
def test_every_voronoi_region_of_one_triangle(point, foot):
    v, f = R.one_triangle()
    for dtype in (F32, np.float64):
        r = R.point_mesh_distance(np.array([point]), v, f, dtype=dtype)
        assert (r['closest'][0] == np.array(foot, dtype=dtype)).all(), (dtype, r['closest'])
        assert r['face'][0] == 0
        assert r['distance'][0] == dtype(np.sqrt(((np.array(point, dtype=np.float64) - np.array(foot)) ** 2).sum()))


def test_degenerate_faces_never_give_nan():
    """Three collinear vertices: the distance to the segment; three equal vertices: the distance to the point."""
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=F32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    pts = np.array([[0.5, 1, 0], [1.5, 1, 0], [-3, 4, 0], [5, 0, 4], [1, 0, 0]], dtype=F32)
    r = R.point_mesh_distance(pts, line, f)
    assert (r['distance'] == np.array([1, 1, 5, 5, 0], dtype=F32)).all() and (r['face'] == 0).all()
    assert (r['closest'] == np.array([[0.5, 0, 0], [1.5, 0, 0], [0, 0, 0], [2, 0, 0], [1, 0, 0]], dtype=F32)).all()
    for order in ([0, 2, 1], [1, 0, 2], [2, 1, 0]):
        again = R.point_mesh_distance(pts, line, np.array([order], dtype=np.int32))
        assert (again['distance'] == r['distance']).all()
    dot = np.array([[1, 2, 3]] * 3, dtype=F32)
    r = R.point_mesh_distance(np.array([[1, 2, 3], [4, 6, 3], [1, 2, 5]], dtype=F32), dot, f)
    assert (r['distance'] == np.array([0, 5, 2], dtype=F32)).all() and (r['closest'] == dot).all()


def test_special_queries_and_max_distance():
    (vi, fi) = R.cube(0.5)
    pts = np.array([[0.75, 0.75, 0.75], [np.nan, 0, 0], [0.75, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [3, 0, 0]], dtype=F32)
    r = R.point_mesh_distance(pts, vi, fi, max_distance=0.25)
    assert r['face'].tolist() == [-1, -1, 0, -1, -1, -1]
    assert np.isinf(r['distance'][0]) and np.isnan(r['distance'][[1, 3, 4]]).all() and r['distance'][2] == F32(0.25)
    assert np.isinf(r['distance'][5]) and np.isnan(r['closest'][[0, 1, 3, 4, 5]]).all()
    empty = R.point_mesh_distance(pts, vi, np.zeros((0, 3), dtype=np.int32))
    assert np.isinf(empty['distance'][[0, 2, 5]]).all() and (empty['face'] == -1).all()


# ---- sampling ------------------------------------------------------------------------------------------------------------------
TWO = (np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 5, 5], [7, 5, 5], [5, 6, 5]], dtype=F32),
       np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32))


def test_samples_follow_the_areas():
    """Areas 3 : 1, n = 4096: the count on the large face is binomial(4096, 3/4), sigma = 27.7; within 5 sigma = 139."""
    s = R.sample_surface(*TWO, 4096, seed=0)
    assert R.face_weights(*TWO).tolist() == [6.0, 2.0]
    assert abs(int((s['face'] == 0).sum()) - 3072) <= 139
    assert s['points'].dtype == F32 and s['bary'].dtype == F32 and s['face'].dtype == np.int32
    on0 = s['points'][s['face'] == 0]
    assert (on0[:, 2] == 0).all() and (on0 >= 0).all() and (on0[:, 0] / 3 + on0[:, 1] / 2 <= 1 + 1e-6).all()


def test_barycentrics_are_a_partition_of_one():
    v, f = R.icosphere(1)
    s = R.sample_surface(v, f, 2000, seed=11)
    assert (s['bary'] >= 0).all()
    assert np.abs(s['bary'].astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
    assert (np.abs(np.linalg.norm(s['points'].astype(np.float64), axis=1) - 1.0) < 0.1).all()
    assert len(set(s['face'].tolist())) == 80


def test_seeds():
    v, f = R.icosphere(1)
    a, b, c = (R.sample_surface(v, f, 257, seed=s) for s in (5, 5, 6))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes()
    assert a['points'].tobytes() != c['points'].tobytes() and (a['face'] != c['face']).any()
    assert R.sample_surface(v, f, 100, seed=5)['points'].tobytes() == a['points'][:100].tobytes()      # sample k is a function of (seed, k)


def test_a_face_without_area_is_never_drawn():
    v = np.concatenate([TWO[0], np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=F32)])
    f = np.array([[6, 7, 8], [0, 1, 2], [6, 6, 6], [3, 4, 5], [7, 8, 6]], dtype=np.int32)
    assert R.face_weights(v, f).tolist() == [0.0, 6.0, 0.0, 2.0, 0.0]
    s = R.sample_surface(v, f, 3000, seed=2)
    assert set(s['face'].tolist()) == {1, 3}
    assert R.surface_cdf(v, f[[0, 2, 4]]).tolist() == [0, 0, 0]


def test_hashes_are_those_of_hashprng():
    import hashprng
    x = np.array([0, 1, 12345678901234567, 2 ** 64 - 1], dtype=np.uint64)
    assert [R.splitmix64(int(i)) for i in x] == [int(i) for i in hashprng._splitmix64(x)]
    assert R.mulhi64(2 ** 63, 6) == 3 and R.mulhi64(2 ** 64 - 1, 2 ** 40) == 2 ** 40 - 1


# ---- argument checks, before any launch -----------------------------------------------------------------------------------
CUBE = _mesh(*R.cube(0.5))
PTS = torch.zeros((4, 3), dtype=torch.float32)


@pytest.mark.parametrize("points", [PTS.double(), PTS[:, :2], PTS.reshape(-1), PTS.numpy(), None])
def test_point_mesh_distance_refuses_points(points):
    with pytest.raises(ValueError):
        G.point_mesh_distance(points, CUBE)


@pytest.mark.parametrize("mesh", [
    {'vertices': CUBE['vertices'].double(), 'faces': CUBE['faces']}, {'vertices': CUBE['vertices'], 'faces': CUBE['faces'].long()},
    {'vertices': CUBE['vertices'][:, :2], 'faces': CUBE['faces']}, {'vertices': CUBE['vertices'], 'faces': CUBE['faces'][:, :2]},
    {'vertices': CUBE['vertices']}, None])
def test_meshes_are_checked(mesh):
    for call in (lambda: G.point_mesh_distance(PTS, mesh), lambda: G.sample_surface(mesh, 10), lambda: G.build_distance_grid(mesh),
                 lambda: G.mesh_distance(mesh, CUBE), lambda: G.mesh_distance(CUBE, mesh)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("res", [0, 257, -1, (4, 4), (4, 0, 4), (4, 4, 300), 2.5, (1, 2, 3.5), "8", True])
def test_grid_resolution_outside_1_256(res):
    with pytest.raises(ValueError, match="grid_resolution"):
        G.point_mesh_distance(PTS, CUBE, grid_resolution=res)
    with pytest.raises(ValueError, match="grid_resolution"):
        G.build_distance_grid(CUBE, grid_resolution=res)


@pytest.mark.parametrize("max_distance", [-1.0, float("nan"), -0.001, "far"])
def test_max_distance_negative_or_nan(max_distance):
    with pytest.raises(ValueError, match="max_distance"):
        G.point_mesh_distance(PTS, CUBE, max_distance=max_distance)


@pytest.mark.parametrize("n", [0, -5, 2.5, None, 2 ** 31])
def test_sample_count(n):
    with pytest.raises(ValueError):
        G.sample_surface(CUBE, n)
    with pytest.raises(ValueError):
        G.mesh_distance(CUBE, CUBE, n_samples=n if n != 2 ** 31 else 0)


def test_meshes_without_surface():
    empty = {'vertices': CUBE['vertices'], 'faces': torch.zeros((0, 3), dtype=torch.int32)}
    with pytest.raises(ValueError):
        G.sample_surface(empty, 10)
    with pytest.raises(ValueError):
        G.mesh_distance(empty, CUBE)
    with pytest.raises(ValueError):
        G.mesh_distance(CUBE, empty)
    flat = {'vertices': torch.ones((3, 3), dtype=torch.float32), 'faces': torch.tensor([[0, 1, 2]], dtype=torch.int32)}
    with pytest.raises(REFUSED):      # W == 0: known only once the weights exist, which needs the GPU
        G.sample_surface(flat, 10)


def test_cpu_tensors_are_refused():
    for call in (lambda: G.point_mesh_distance(PTS, CUBE), lambda: G.sample_surface(CUBE, 10), lambda: G.build_distance_grid(CUBE, 4),
                 lambda: G.mesh_distance(CUBE, CUBE, 10)):
        with pytest.raises(L.HnError, match="no CPU fallback"):
            call()


def test_thresholds_are_checked():
    for bad in (-0.1, [0.1, float("nan")], ["x"]):
        with pytest.raises(ValueError, match="thresholds"):
            G.mesh_distance(CUBE, CUBE, 10, thresholds=bad)


def test_default_grid_resolution():
    rule = HN.ops.mesh.default_grid_resolution
    assert rule(400, (0, 0, 0), (1, 1, 1)) == (10, 10, 10)
    assert rule(400, (0, 0, 0), (2, 1, 0)) == (10, 5, 1)
    assert rule(10 ** 7, (0, 0, 0), (1, 1, 1e-4)) == (256, 256, 1)
    assert rule(1, (0, 0, 0), (1, 1, 1)) == (1, 1, 1) and rule(50, (1, 1, 1), (1, 1, 1)) == (1, 1, 1)


# ---- distance_colors (plain torch: runs anywhere) ----------------------------------------------------------------------------
def test_distance_colors():
    from hypernerf_torch_amd import inference
    lut = inference.jet_lut().flip(1)
    d = torch.tensor([0.0, 0.5, 1.0, 2.0, float("nan"), float("inf"), 0.999 / 255, 1.5 / 255], dtype=torch.float32)
    c = G.distance_colors(d, vmax=1.0)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (8, 3)
    assert (c[0] == lut[0]).all() and (c[6] == lut[0]).all() and (c[7] == lut[1]).all()
    assert (c[1] == lut[127]).all()
    for k in (2, 3, 4, 5):
        assert (c[k] == lut[255]).all()
    assert int(lut[0][2]) > int(lut[0][0]) and int(lut[255][0]) > int(lut[255][2])      # near is blue, far is red
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            G.distance_colors(d, bad)
    with pytest.raises(ValueError):
        G.distance_colors(d.reshape(2, 4), 1.0)


# ---- binding -----------------------------------------------------------------------------------------------------------------
def test_binding_knows_the_new_entries():
    names = {"hn_md_face_weights", "hn_md_sample", "hn_md_pack", "hn_md_cell_count", "hn_md_cell_fill", "hn_md_cell_keys",
             "hn_md_query"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES) and "hn_mesh_distance.hip" in L.SOURCES
    # the kernel file's limits and their host mirrors (the header's set of macros is pinned at ABI 340)
    import os
    import re
    src = open(os.path.join(L.CSRC, "hn_mesh_distance.hip")).read()
    macros = {k: int(v) for k, v in re.findall(r"^#define HN_MD_(MAX_RES|TRI_FLOATS|WEIGHT_BITS) (\d+)", src, flags=re.M)}
    assert macros == {"MAX_RES": 256, "TRI_FLOATS": 12, "WEIGHT_BITS": 24}
    M = HN.ops.mesh
    assert (M.MD_MAX_RES, M.MD_TRI_FLOATS, M.MD_WEIGHT_BITS) == (macros["MAX_RES"], macros["TRI_FLOATS"], macros["WEIGHT_BITS"])
    assert len(L.ARGTYPES["hn_md_query"]) == 18 and len(L.ARGTYPES["hn_md_sample"]) == 11
    assert "hn_mesh_distance.hip" in HN.ops.__doc__
    for name in ("surface_cdf", "sample_faces", "distance_grid", "grid_query", "default_grid_resolution"):
        assert name in HN.ops.mesh.__all__ and getattr(HN.functional, name) is getattr(HN.ops.mesh, name)
