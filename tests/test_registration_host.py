"""Host tests of the registration (csrc/hn_registration.hip, geometry.register_mesh / transform_mesh /
aligned_mesh_distance), no GPU: both solves — the restated ones (tests/registration_restated.py) and the product's
(ops.registration) — recover exact transforms from exact moments, composition and the matrix round trip, the restated
summation order against a plain sum, the argument checks, the binding."""
import math
import os
import re

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import geometry as G

import mesh_distance_restated as MD
import registration_restated as R

F32 = np.float32
OPS = HN.ops.registration
REFUSED = (ValueError, L.HnError)


def _mesh(v, f):
    return {'vertices': torch.from_numpy(np.ascontiguousarray(v, dtype=F32)), 'faces': torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32))}


def _hash_unit(seed, shape):
    """float64 values in [-1, 1) from splitmix64, 24 bits each."""
    n = int(np.prod(shape))
    key = MD.splitmix64(seed)
    u = np.array([MD.splitmix64((key + i) & MD.M64) >> 40 for i in range(n)], dtype=np.float64) * 2.0 ** -24
    return (2.0 * u - 1.0).reshape(shape)


def _exact_point_sums(p, q):
    s = np.zeros(R.SUMS)
    s[0], s[1] = len(p), ((p - q) ** 2).sum()
    s[2:5], s[5:8] = p.sum(0), q.sum(0)
    s[8:17] = (q[:, :, None] * p[:, None, :]).sum(0).reshape(9)
    s[17], s[18] = (p * p).sum(), (q * q).sum()
    return s


def _exact_plane_sums(p, q, n):
    r = ((p - q) * n).sum(1)
    jac = np.concatenate([np.cross(p, n), n, (p * n).sum(1, keepdims=True)], axis=1)
    s = np.zeros(R.SUMS)
    s[0], s[1], s[2] = len(p), ((p - q) ** 2).sum(), (r * r).sum()
    s[3:31] = (jac.T @ jac)[np.triu_indices(7)]
    s[31:38] = jac.T @ r
    return s


TRANSFORMS = {'rigid': (1.0, R.axis_angle((1, 2, 3), 10), np.array([0.05, -0.03, 0.02])),
              'far': (1.0, R.axis_angle((-2, 1, 0.5), 140), np.array([-3.0, 0.5, 2.0])),
              'grow': (1.2, R.axis_angle((1, 2, 3), 25), np.array([0.15, -0.1, 0.1])),
              'shrink': (1 / 1.2, R.axis_angle((3, -1, 2), 25), np.array([0.15, -0.1, 0.1]))}


# ---- the solves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [R.solve_point, OPS.solve_point], ids=["restated", "product"])
@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_point_solve_recovers_the_transform(name, solve):
    """q = s R p + t exactly (float64): the closed form returns (s, R, t) in one step, whatever the angle."""
    s, rot, t = TRANSFORMS[name]
    p = _hash_unit(11, (200, 3))
    q = s * p @ rot.T + t
    got = solve(_exact_point_sums(p, q), s != 1.0)
    assert abs(got[0] - s) < 1e-12 and np.abs(got[1] - rot).max() < 1e-12 and np.abs(got[2] - t).max() < 1e-12
    assert solve(_exact_point_sums(p, q), False)[0] == 1.0


@pytest.mark.parametrize("solve", [R.solve_point, OPS.solve_point], ids=["restated", "product"])
def test_point_solve_corrects_a_reflection(solve):
    """Coplanar points mirrored through their plane fit a reflection as well as a rotation: diag(1, 1, det(U V^T)) picks the
    rotation."""
    p = _hash_unit(12, (50, 3))
    p[:, 2] = 0.0
    rot = R.axis_angle((0, 0, 1), 30)
    got = solve(_exact_point_sums(p, p @ rot.T), False)
    assert np.linalg.det(got[1]) == pytest.approx(1.0, abs=1e-12) and np.abs(got[1] - rot).max() < 1e-12


@pytest.mark.parametrize("solve", [R.solve_plane, OPS.solve_plane], ids=["restated", "product"])
@pytest.mark.parametrize("with_scale", [False, True])
def test_plane_solve_recovers_a_small_transform(solve, with_scale):
    """Residuals that are exactly linear in (omega, t', sigma): r = -J x for hash-drawn points and unit normals.  The normal
    equations then return x to rounding: float64, error under 1e-12."""
    p = _hash_unit(13, (300, 3))
    n = _hash_unit(14, (300, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    x = np.array([0.01, -0.02, 0.015, 0.03, -0.01, 0.02, 0.05 if with_scale else 0.0])
    jac = np.concatenate([np.cross(p, n), n, (p * n).sum(1, keepdims=True)], axis=1)
    q = p + (jac @ x)[:, None] * n                      # (p - q) . n = -J x
    got = solve(_exact_plane_sums(p, q, n), with_scale)
    assert abs(got[0] - (1.0 + x[6])) < 1e-12
    assert np.abs(got[1] - R.rodrigues(x[:3])).max() < 1e-12 and np.abs(got[2] - x[3:6]).max() < 1e-12


@pytest.mark.parametrize("solve", [R.solve_plane, OPS.solve_plane], ids=["restated", "product"])
def test_plane_solve_of_a_planar_target_is_finite_and_minimal(solve):
    """Every normal is +z: the 7 x 7 matrix has rank 3 (rotation about x and y, translation along z).  lstsq gives the
    minimum-norm step: nothing in the plane, no spin about z."""
    p = _hash_unit(15, (100, 3))
    n = np.tile([0.0, 0.0, 1.0], (100, 1))
    q = p.copy()
    q[:, 2] = 0.25
    got = solve(_exact_plane_sums(p, q, n), False)
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert abs(got[2][0]) < 1e-12 and abs(got[2][1]) < 1e-12 and abs(got[1][1, 0] - got[1][0, 1]) < 1e-12

def test_composition_and_matrix_round_trip():
    a, b = TRANSFORMS['grow'], TRANSFORMS['shrink']
    for compose, matrix in ((R.compose, R.matrix_of), (OPS.compose_similarity, OPS.similarity_matrix)):
        assert np.abs(matrix(*compose(a, b)) - matrix(*a) @ matrix(*b)).max() < 1e-15
    s, rot, t = OPS.check_similarity(OPS.similarity_matrix(*a), "test")
    assert abs(s - a[0]) < 1e-12 and np.abs(rot - a[1]).max() < 1e-12 and (t == a[2]).all()
    s, rot, t = OPS.split_similarity(torch.from_numpy(OPS.similarity_matrix(*b)))
    assert abs(s - b[0]) < 1e-12 and np.abs(rot - b[1]).max() < 1e-12
    x = _hash_unit(16, (3,))
    assert np.abs(OPS.rodrigues(x) - R.rodrigues(x)).max() < 1e-15 and np.abs(OPS.rodrigues(x * 1e-9) - np.eye(3)).max() < 2e-9
    for deg in (0.0, 1e-6, 10.0, 179.0):
        assert OPS.rotation_angle(R.axis_angle((1, 2, 3), deg)) == pytest.approx(math.radians(deg), abs=1e-15, rel=1e-9)
        assert R.angle_of(R.axis_angle((1, 2, 3), deg)) == pytest.approx(math.radians(deg), abs=1e-15, rel=1e-9)


# ---- the restated sums ----------------------------------------------------------------------------------------------------
def _query_inputs(n, seed=3):
    """Points around bumpy(1), their brute-force nearest points, and a tau inside the range of the distances."""
    v, f = R.bumpy(1)
    p = MD.hash_points(seed, n, -1.2, 1.2)
    q = MD.point_mesh_distance(p, v, f, max_distance=0.6)
    return p, q, R.pack_triangles(v, f), np.sort(q['distance'][np.isfinite(q['distance'])])[n // 3]


@pytest.mark.parametrize("mode", ['point', 'plane'])
def test_restated_order_agrees_with_a_plain_sum(mode):
    """The documented order against NumPy's own float64 column sums of the same terms: within the bound N * 2^-50 * sum
    |term|; and the order is a function of n_blocks — other block counts give other last bits, the same count the same."""
    p, q, tri, tau = _query_inputs(700)
    inlier, terms = R.moment_terms(p, q['closest'], q['distance'], q['face'], tri, tau, mode)
    assert 100 < inlier.sum() < 600 and np.isnan(q['closest'][~np.isfinite(q['distance'])]).all()
    plain = terms[inlier].sum(axis=0)
    bound = R.moments_bound(p, q['closest'], q['distance'], q['face'], tri, tau, mode)
    width = R.POINT_SUMS if mode == 'point' else R.SUMS
    results = [R.moments(p, q['closest'], q['distance'], q['face'], tri, tau, mode, nb) for nb in (1, 2, 3, None, 2)]
    for got in results:
        assert np.isfinite(got).all() and (np.abs(got - plain)[:width] <= bound[:width]).all() and (got[width:] == 0).all()
        assert got[0] == inlier.sum()
    assert results[1].tobytes() == results[4].tobytes()
    assert len({r.tobytes() for r in results[:3]}) > 1
    assert R.default_blocks(700) == 1 and R.default_blocks(2049) == 2 and R.default_blocks(10 ** 7) == 512


def test_bumpy_has_no_symmetry():
    v, f = R.bumpy(2)
    assert v.dtype == F32 and f.shape == (320, 3) and v.shape == (162, 3)
    ext = v.max(0) - v.min(0)
    assert ext[0] > ext[1] > ext[2] > 0.9
    for flip in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1)):      # the ellipsoid's symmetries
        far = MD.point_mesh_distance(v * np.array(flip, dtype=F32), v, f)['distance'].max()
        assert far > 0.05


# ---- argument checks, before any launch -----------------------------------------------------------------------------------
A = _mesh(*R.bumpy(1))
B = _mesh(*MD.cube(0.5))
PTS = torch.zeros((8, 3), dtype=torch.float32)
EMPTY = {'vertices': A['vertices'], 'faces': torch.zeros((0, 3), dtype=torch.int32)}


@pytest.mark.parametrize("kw", [
    dict(n_samples=0), dict(n_samples=2.5), dict(n_samples=True), dict(seed="x"), dict(method='icp'), dict(method=None),
    dict(trim=0.0), dict(trim=1.5), dict(trim=float("nan")), dict(trim="most"), dict(max_distance=-1.0),
    dict(max_distance=float("nan")), dict(max_iterations=0), dict(max_iterations=2.5), dict(tol=0.0), dict(tol=-1e-5),
    dict(tol=float("inf")), dict(grid_resolution=0), dict(grid_resolution=(4, 4)), dict(init='center'),
    dict(init=np.eye(3)), dict(init=np.diag([1.0, 1.0, -1.0, 1.0])), dict(init=np.diag([1.0, 2.0, 1.0, 1.0])),
    dict(init=np.zeros((4, 4))), dict(init=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1]]),
], ids=str)
def test_register_mesh_refuses_arguments(kw):
    with pytest.raises(ValueError, match="register_mesh"):
        G.register_mesh(A, B, **kw)
    with pytest.raises(ValueError, match="register_mesh"):
        G.aligned_mesh_distance(A, B, register=kw)


@pytest.mark.parametrize("source, target", [
    (EMPTY, B), (A, EMPTY), (None, B), (A, None), ({'vertices': A['vertices']}, B), (PTS.double(), B), (PTS[:, :2], B),
    (PTS[:0], B), ({'vertices': A['vertices'].double(), 'faces': A['faces']}, B), (A, {'cell_begin': None}),
    (A, {'cell_begin': None, 'num_faces': 0})])
def test_register_mesh_refuses_meshes(source, target):
    with pytest.raises(ValueError):
        G.register_mesh(source, target)


def test_cpu_tensors_are_refused():
    """With everything in range the first thing that needs the device says so: no CPU fallback."""
    for call in (lambda: G.register_mesh(A, B), lambda: G.register_mesh(PTS, B), lambda: G.register_mesh(A, B, init=np.eye(4)),
                 lambda: G.transform_mesh(A, np.eye(4)), lambda: G.aligned_mesh_distance(A, B),
                 lambda: OPS.transform_points(PTS, 1.0, np.eye(3), np.zeros(3))):
        with pytest.raises(L.HnError, match="no CPU fallback"):
            call()


@pytest.mark.parametrize("matrix", [np.diag([1.0, 1.0, -1.0, 1.0]), np.diag([1.0, 1.5, 1.0, 1.0]), np.zeros((4, 4)), np.eye(3),
                                    np.full((4, 4), np.nan), None, "identity"], ids=str)
def test_transform_mesh_refuses_matrices(matrix):
    with pytest.raises(ValueError, match="transform_mesh"):
        G.transform_mesh(A, matrix)


def test_transform_mesh_checks_the_mesh():
    with pytest.raises(ValueError):
        G.transform_mesh({'vertices': A['vertices']}, np.eye(4))
    with pytest.raises(ValueError, match="normals"):
        G.transform_mesh(dict(A, normals=A['vertices'][:5]), np.eye(4))
    with pytest.raises(ValueError):
        G.aligned_mesh_distance(A, B, register="plane")
    with pytest.raises(ValueError, match="not finite"):
        OPS.transform_points(PTS, 1e39, np.eye(3), np.zeros(3))


def test_moments_and_threshold_refuse_arguments():
    q = {'closest': PTS, 'distance': PTS[:, 0].contiguous(), 'face': torch.zeros(8, dtype=torch.int32)}
    tri, tau = torch.zeros((4, 12)), torch.ones(1)
    for bad in (dict(mode='both'), dict(n_blocks=0), dict(n_blocks=OPS.REG_MAX_BLOCKS + 1), dict(n_blocks=1.5)):
        kw = dict(mode='point', n_blocks=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="registration_moments"):
            OPS.registration_moments(PTS, q, tri, tau, **kw)
    for bad_q in ({'closest': PTS}, dict(q, face=q['face'].long()), dict(q, distance=q['distance'][:4])):
        with pytest.raises(ValueError, match="registration_moments"):
            OPS.registration_moments(PTS, bad_q, tri, tau, 'plane')
    with pytest.raises(ValueError, match="registration_moments"):
        OPS.registration_moments(PTS, q, tri[:, :9], tau, 'plane')
    with pytest.raises(L.HnError, match="no CPU fallback"):
        OPS.registration_moments(PTS, q, tri, tau, 'plane')
    for trim in (0.0, 1.01, -1.0):
        with pytest.raises(ValueError, match="trim"):
            OPS.trim_threshold(q['distance'], trim)
    d = torch.tensor([0.5, float("inf"), 0.25, float("nan"), 1.0, 0.75])
    assert OPS.trim_threshold(d, 1.0).tolist() == [float("inf")]
    assert OPS.trim_threshold(d, 0.5).tolist() == [0.5] and OPS.trim_threshold(d, 0.51).tolist() == [0.75]      # plain torch
    assert OPS.trim_threshold(d, 0.01).tolist() == [0.25] == [float(R.trim_tau(d.numpy(), 0.01))]
    assert [float(R.trim_tau(d.numpy(), t)) for t in (0.5, 0.51, 1.0)] == [0.5, 0.75, float("inf")]


# ---- binding -----------------------------------------------------------------------------------------------------------------
def test_binding_knows_the_new_entries():
    names = {"hn_reg_transform", "hn_reg_moments"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES) and "hn_registration.hip" in L.SOURCES
    assert len(L.ARGTYPES["hn_reg_transform"]) == 6 and len(L.ARGTYPES["hn_reg_moments"]) == 13
    HN.build()
    lib = L.load()
    assert lib.hn_version() == 340
    assert not [k for k in L.CONSTANTS if k.startswith("HN_REG_")]          # no new macro in the header
    # the kernel file's limits and their host mirrors
    src = open(os.path.join(L.CSRC, "hn_registration.hip")).read()
    macros = {k: int(v) for k, v in re.findall(r"^#define HN_REG_(THREADS|MAX_BLOCKS|POINT_SUMS|SUMS|PARAMS) +(\d+)", src, flags=re.M)}
    assert macros == {"THREADS": 256, "MAX_BLOCKS": 1024, "POINT_SUMS": 19, "SUMS": 38, "PARAMS": 13}
    assert (OPS.REG_THREADS, OPS.REG_MAX_BLOCKS, OPS.REG_POINT_SUMS, OPS.REG_SUMS, OPS.REG_PARAMS) == \
        tuple(macros[k] for k in ("THREADS", "MAX_BLOCKS", "POINT_SUMS", "SUMS", "PARAMS"))
    assert (R.THREADS, R.MAX_BLOCKS, R.POINT_SUMS, R.SUMS) == (OPS.REG_THREADS, OPS.REG_MAX_BLOCKS, OPS.REG_POINT_SUMS, OPS.REG_SUMS)
    assert OPS.REG_SUMS == 3 + 28 + 7 and OPS.REG_POINT_SUMS == 2 + 3 + 3 + 9 + 2
    for n in (1, 2048, 2049, 10 ** 5, 10 ** 6, 10 ** 9):
        assert OPS.default_moment_blocks(n) == R.default_blocks(n) <= OPS.REG_MAX_BLOCKS
    assert "hn_registration.hip" in HN.ops.__doc__
    for name in ("transform_points", "registration_moments", "trim_threshold", "solve_point", "solve_plane"):
        assert name in OPS.__all__ and getattr(HN.functional, name) is getattr(OPS, name)
    for name in ("register_mesh", "transform_mesh", "aligned_mesh_distance"):
        assert callable(getattr(G, name))


def test_status_codes_before_any_launch():
    """-2 for sizes out of range, -3 for NULL pointers: answered on the host, nothing reaches a device."""
    HN.build()
    lib = L.load()
    import ctypes
    params = (ctypes.c_float * 13)(1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0)
    bad = (ctypes.c_float * 13)(1, 0, 0, 0, 1, 0, 0, 0, 1, float("nan"), 0, 0, 0)
    assert lib.hn_reg_transform(None, 0, params, 0, None, None) == -2
    assert lib.hn_reg_transform(None, 2 ** 31, params, 0, None, None) == -2
    assert lib.hn_reg_transform(None, 4, None, 0, None, None) == -2
    assert lib.hn_reg_transform(None, 4, bad, 0, None, None) == -2
    assert lib.hn_reg_transform(None, 4, params, 2, None, None) == -2
    assert lib.hn_reg_transform(None, 4, params, 1, None, None) == -3
    none = [None] * 4
    assert lib.hn_reg_moments(*none, 0, None, 4, None, 0, 1, None, None, None) == -2
    assert lib.hn_reg_moments(*none, 4, None, 0, None, 0, 1, None, None, None) == -2
    assert lib.hn_reg_moments(*none, 4, None, 4, None, 2, 1, None, None, None) == -2
    assert lib.hn_reg_moments(*none, 4, None, 4, None, 0, 0, None, None, None) == -2
    assert lib.hn_reg_moments(*none, 4, None, 4, None, 1, 1025, None, None, None) == -2
    assert lib.hn_reg_moments(*none, 4, None, 4, None, 1, 1024, None, None, None) == -3
