"""CPU tests of the isosurface definition (tests/isosurface_restated.py, the NumPy float32 restatement of
csrc/hn_geometry.hip) on analytic fields, of the PLY files and of the argument checks that run before any kernel.

Expected figures of the sphere come from the marching-tetrahedra discretisation itself (second order: the chord error of
a piecewise-linear surface), measured once with an independent prototype: -1.56 % of the volume at 17^3, -0.39 % at 33^3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import isosurface_restated as R
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import geometry as G

UNIT = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)


def positions(shape, bounds=UNIT):
    shape = (shape,) * 3 if isinstance(shape, int) else shape
    return R.lattice_points(shape, bounds).astype(np.float64).reshape(shape + (3,))


def sphere(n):
    return (0.7071 - np.linalg.norm(positions(n) - np.array([0.013, -0.021, 0.007]), axis=-1)).astype(np.float32)


def torus(n):
    y = positions(n) - np.array([0.031, -0.017, 0.023])
    return (0.23 - np.sqrt((np.sqrt(y[..., 0] ** 2 + y[..., 1] ** 2) - 0.55) ** 2 + y[..., 2] ** 2)).astype(np.float32)


def two_spheres(n):
    x = positions(n)
    a = 0.3 - np.linalg.norm(x - np.array([0.45, 0.011, 0.023]), axis=-1)
    b = 0.3 - np.linalg.norm(x - np.array([-0.45, 0.011, 0.023]), axis=-1)
    return np.maximum(a, b).astype(np.float32)


def octahedron():
    i, j, k = np.meshgrid(*[np.arange(17)] * 3, indexing="ij")
    return (4 - abs(i - 8) - abs(j - 8) - abs(k - 8)).astype(np.float32), (0.0, 16.0, 0.0, 16.0, 0.0, 16.0)


PLANE_N = np.array([0.3, 0.5, -0.7])
PLANE_BOUNDS = (-1.0, 1.5, -0.7, 0.9, 0.1, 2.0)


def plane(shape, offset, bounds=PLANE_BOUNDS):
    return (positions(shape, bounds) @ PLANE_N + 0.0123 + offset).astype(np.float32)


def checked(f, iso, bounds):
    m = R.extract_isosurface(f, iso, bounds)
    assert m["vertices"].dtype == np.float32 and m["normals"].dtype == np.float32 and m["faces"].dtype == np.int32
    assert m["vertices"].shape == m["normals"].shape and m["faces"].shape[1] == 3
    if m["faces"].size:
        assert m["faces"].min() >= 0 and m["faces"].max() < m["vertices"].shape[0]
        assert np.unique(m["faces"]).size == m["vertices"].shape[0], "every vertex is used by a face"
    return m, R.check_mesh(m["vertices"], m["faces"])


def test_sphere_is_closed_oriented_and_converges():
    want = 4.0 / 3.0 * np.pi * 0.7071 ** 3
    err = {}
    for n in (17, 33):
        m, c = checked(sphere(n), 0.0, UNIT)
        assert c["closed"] and c["oriented"] and c["euler"] == 2 and c["volume"] > 0, (n, c)
        err[n] = (c["volume"] - want) / want
        # normals point outwards (towards lower f): along the radius
        radial = m["vertices"].astype(np.float64) - np.array([0.013, -0.021, 0.007])
        radial /= np.linalg.norm(radial, axis=1, keepdims=True)
        assert (np.einsum("ij,ij->i", m["normals"].astype(np.float64), radial) > 0.999).all()
        assert np.abs(np.linalg.norm(m["normals"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    print(f"sphere: relative volume error {err[17]:+.4%} at 17^3, {err[33]:+.4%} at 33^3")
    assert abs(err[33]) < 0.01
    assert abs(err[17]) >= 3.0 * abs(err[33])


def test_torus_and_two_spheres_topology():
    _, c = checked(torus(17), 0.0, UNIT)
    assert c["closed"] and c["oriented"] and c["euler"] == 0 and c["volume"] > 0, c
    _, c = checked(two_spheres(17), 0.0, UNIT)
    assert c["closed"] and c["oriented"] and c["euler"] == 4 and c["volume"] > 0, c


def test_lattice_values_equal_to_iso_give_a_closed_oriented_surface():
    """4 - |i-8| - |j-8| - |k-8|: lattice values exactly on the surface, so vertices coincide and triangles degenerate;
    the topology and the orientation come from integers and stay right, and the volume is that of the octahedron."""
    f, bounds = octahedron()
    m, c = checked(f, 0.0, bounds)
    assert c["closed"] and c["oriented"] and c["euler"] == 2, c
    assert abs(c["volume"] - 256.0 / 3.0) < 1e-4, c["volume"]
    a, b, cc = (m["vertices"][m["faces"][:, i]].astype(np.float64) for i in range(3))
    assert (np.linalg.norm(np.cross(b - a, cc - a), axis=1) == 0).any(), "the field is meant to produce degenerate triangles"


@pytest.mark.parametrize("shape,offset", [((5, 7, 9), 0.9), ((2, 2, 2), 0.6), ((33, 17, 9), 0.9)])
def test_plane_vertices_and_normals(shape, offset):
    """A linear field is interpolated exactly: every vertex on the plane and every normal the plane's, to 1e-6; a
    non-cubic grid (and the single cell) shows stride and edge-ownership mistakes."""
    f = plane(shape, offset)
    m, c = checked(f, 0.0, PLANE_BOUNDS)
    assert m["faces"].shape[0] > 0
    v = m["vertices"].astype(np.float64)
    assert np.abs(v @ PLANE_N + 0.0123 + offset).max() < 1e-6
    assert np.abs(m["normals"] - (-PLANE_N / np.linalg.norm(PLANE_N))).max() < 1e-6
    lo, hi = np.array(PLANE_BOUNDS[0::2]), np.array(PLANE_BOUNDS[1::2])
    assert (v >= lo - 1e-6).all() and (v <= hi + 1e-6).all()
    assert not c["closed"], "an open sheet has boundary edges"
    # every face winds with the plane's normal
    a, b, cc = (v[m["faces"][:, i]] for i in range(3))
    assert (np.cross(b - a, cc - a) @ (-PLANE_N) > 0).all()


def test_orderings():
    """Vertices ascend with their edge slot, faces with (cell, tetrahedron, triangle): checked on the single cell, where
    both are easy to enumerate by hand — and an empty surface gives zero-length arrays."""
    f = np.zeros((2, 2, 2), dtype=np.float32)
    f[0, 0, 0] = 1.0                                     # one inside corner: the origin
    m = R.extract_isosurface(f, 0.5, (0.0, 1.0, 0.0, 1.0, 0.0, 1.0))
    # the origin owns all 7 edge classes; slot order = direction class order
    want = 0.5 * R.DIRS.astype(np.float32)
    assert np.array_equal(m["vertices"], want)
    assert m["faces"].shape == (6, 3)                    # one triangle per tetrahedron, all six touch the origin
    for q, face in enumerate(m["faces"]):
        v = R.tet_corners(q)
        assert sorted(face.tolist()) == sorted(R.DIR_CLASS[tuple(v[t].tolist())] for t in (1, 2, 3))
    c = R.check_mesh(m["vertices"], m["faces"])
    assert c["volume"] > 0                               # open fan around the origin, normals away from it
    e = R.extract_isosurface(np.zeros((3, 4, 5), dtype=np.float32), 0.5, UNIT)
    assert e["vertices"].shape == (0, 3) and e["normals"].shape == (0, 3) and e["faces"].shape == (0, 3)
    nan = R.extract_isosurface(np.full((3, 3, 3), np.nan, dtype=np.float32), 0.0, UNIT)
    assert nan["faces"].shape == (0, 3), "NaN is outside"


def test_lattice_points_restated():
    shape, bounds = (5, 7, 9), (-1.0, 1.5, -0.7, 0.9, 0.1, 2.0)
    p = R.lattice_points(shape, bounds)
    assert p.shape == (5 * 7 * 9, 3) and p.dtype == np.float32
    assert np.array_equal(p[0], np.float32([-1.0, -0.7, 0.1]))
    assert np.allclose(p[-1], [1.5, 0.9, 2.0], atol=1e-6)
    assert np.array_equal(p[(2 * 7 + 3) * 9 + 4], R.lattice_points(shape, bounds, (2 * 7 + 3) * 9 + 4, 1)[0])
    tail = R.lattice_points(shape, bounds, 300, 40)      # 15 real points, then the last one repeated
    assert np.array_equal(tail[:15], p[300:]) and (tail[15:] == p[-1]).all()


def test_ply_round_trip(tmp_path):
    m = R.extract_isosurface(sphere(9), 0.0, UNIT)
    path = os.path.join(tmp_path, "sphere.ply")
    G.write_ply(path, torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]), m["normals"])
    back = HN.read_ply(path)
    assert all(np.array_equal(back[k], m[k]) and back[k].dtype == m[k].dtype for k in ("vertices", "normals", "faces"))
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {m['vertices'].shape[0]}"]
    assert "property list uchar int vertex_indices" in head and "property float nx" in head
    G.write_ply(path, m["vertices"], m["faces"])                          # without normals
    back = G.read_ply(path)
    assert back["normals"] is None and np.array_equal(back["vertices"], m["vertices"]) and np.array_equal(back["faces"], m["faces"])
    G.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))   # empty mesh
    back = G.read_ply(path)
    assert back["vertices"].shape == (0, 3) and back["faces"].shape == (0, 3) and back["normals"].shape == (0, 3)
    with pytest.raises(ValueError):
        G.write_ply(path, m["vertices"], m["faces"], m["normals"][:-1])
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        G.read_ply(path)


def test_argument_errors_need_no_gpu():
    ok = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError, match="at least 2"):
        HN.extract_isosurface(torch.zeros(4, 1, 4), 0.0, UNIT)
    with pytest.raises(ValueError, match="nx, ny, nz"):
        HN.extract_isosurface(torch.zeros(4, 4), 0.0, UNIT)
    with pytest.raises(ValueError, match="float32"):
        HN.extract_isosurface(ok.double(), 0.0, UNIT)
    with pytest.raises(ValueError, match="contiguous"):
        HN.extract_isosurface(torch.zeros(4, 4, 8)[:, :, ::2], 0.0, UNIT)
    with pytest.raises(ValueError, match="GPU"):
        HN.extract_isosurface(ok, 0.0, UNIT)
    with pytest.raises(ValueError, match="hi > lo"):
        HN.extract_isosurface(ok, 0.0, (-1.0, 1.0, 0.5, 0.5, -1.0, 1.0))
    with pytest.raises(ValueError, match="hi > lo"):
        HN.extract_isosurface(ok, 0.0, (1.0, -1.0, -1.0, 1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="xmin, xmax"):
        HN.extract_isosurface(ok, 0.0, (0.0, 1.0))
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):                  # 7 * 700^3 > 2^31 - 1 (no memory is touched)
        HN.extract_isosurface(torch.zeros(1).expand(700, 700, 700), 0.0, UNIT)
    assert 7 * 674 ** 3 <= F.INT32_MAX < 7 * 675 ** 3
    F.check_lattice((674, 674, 674), UNIT, "limit")
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):
        F.check_lattice((675, 675, 675), UNIT, "limit")
    m = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="at least 2"):
        HN.density_grid(m, UNIT, (8, 1, 8), 0)
    with pytest.raises(ValueError, match="hi > lo"):
        HN.density_grid(m, (0.0, 0.0, 0.0, 1.0, 0.0, 1.0), 8, 0)
    with pytest.raises(ValueError, match="chunk"):
        HN.density_grid(m, UNIT, 8, 0, chunk=0)
    with pytest.raises(L.HnError):                                          # a model on the CPU: no CPU fallback
        HN.density_grid(m, UNIT, 4, 0)


def test_c_abi_refuses_bad_lattices_before_any_launch():
    """The entry points of csrc/hn_geometry.hip check their arguments on the host: status -2, no launch, no GPU needed."""
    HN.build()
    lib = L.load()
    assert {"hn_grid_points", "hn_density_activate", "hn_iso_mark", "hn_iso_vertices", "hn_iso_faces"} <= set(L.EXPORTS)
    bounds = (C.c_float * 6)(*UNIT)
    flat = (C.c_float * 6)(-1.0, 1.0, 0.0, 0.0, -1.0, 1.0)
    one = C.c_void_p(16)                                                    # never dereferenced: refused first
    assert lib.hn_grid_points(4, 1, 4, bounds, 0, 16, one, None) == -2
    assert lib.hn_grid_points(4, 4, 4, flat, 0, 16, one, None) == -2
    assert lib.hn_grid_points(4, 4, 4, bounds, 64, 16, one, None) == -2    # start past the lattice
    assert lib.hn_grid_points(4, 4, 4, bounds, 0, 0, one, None) == -2
    assert lib.hn_grid_points(4, 4, 4, bounds, 0, 16, None, None) == -2
    assert lib.hn_grid_points(700, 700, 700, bounds, 0, 16, one, None) == -2
    assert lib.hn_iso_mark(one, 1, 4, 4, 0.0, one, one, None) == -2
    assert lib.hn_iso_mark(one, 700, 700, 700, 0.0, one, one, None) == -2
    assert lib.hn_iso_mark(None, 4, 4, 4, 0.0, one, one, None) == -2
    assert lib.hn_iso_vertices(one, 4, 4, 4, flat, 0.0, one, one, one, one, one, None) == -2
    assert lib.hn_iso_vertices(one, 4, 4, 4, bounds, 0.0, one, None, one, one, one, None) == -2
    assert lib.hn_iso_faces(one, 4, 4, 4, 0.0, None, None, None, None, None) == -2       # count pass without counts
    assert lib.hn_iso_faces(one, 4, 4, 4, 0.0, None, None, None, one, None) == -2        # emit pass without slots
    assert lib.hn_density_activate(None, None, 4, 0, 0.0, None, one, None) == -2
    assert lib.hn_density_activate(one, None, 4, 0, 0.0, bounds, one, None) == -2        # a box needs the points


def test_query_points_surface_without_a_gpu():
    """NerfModel.query_points exists, refuses CPU tensors (no CPU fallback) and malformed points."""
    from hypernerf_torch_amd.hypernerf import models
    emb = {"warp": list(range(10)), "camera": [0], "appearance": list(range(10)), "time": list(range(10))}
    m = models.NerfModel(emb, n_samples_coarse=8, n_samples_fine=8, hyper_slice_method="bendy_sheet")
    assert "no_grad" in models.NerfModel.query_points.__doc__
    with pytest.raises(L.HnError):
        m.query_points(torch.zeros(2, 4, 3), {k: torch.zeros(2, dtype=torch.long) for k in ("warp", "time")})
