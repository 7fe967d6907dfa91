"""GPU tests of the registration (csrc/hn_registration.hip, geometry.register_mesh / transform_mesh /
aligned_mesh_distance): both kernels against the NumPy restatement of the definition (tests/registration_restated.py), bit
for bit — the fp32 transform, the float64 sums in their documented order at every size, block count and threshold — and
the loop on shapes with a known answer: rigid and similarity recovery, the slow point-to-point method, trimming against a
floater, a planar target, and the aligned distance."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_distance_restated as MD
import registration_restated as R
from gpu_common import DEV
from hypernerf_torch_amd import geometry as G
from hypernerf_torch_amd import ops
from test_gpu_mesh_distance import with_degenerate

pytestmark = pytest.mark.gpu

F32 = np.float32
OPS = ops.registration
SIZES = (1, 63, 64, 65, 257, 1000)
CASES = {'a': (1.0, 10.0, (0.05, -0.03, 0.02), False), 'b': (1.2, 25.0, (0.15, -0.1, 0.1), True),
         'c': (1 / 1.2, 25.0, (0.15, -0.1, 0.1), True)}


def _dev(v, f):
    return {'vertices': torch.from_numpy(np.array(v, dtype=F32)).to(DEV), 'faces': torch.from_numpy(np.array(f, dtype=np.int32)).to(DEV)}


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _truth(name):
    s, deg, t, with_scale = CASES[name]
    return s, R.axis_angle((1, 2, 3), deg), np.array(t, dtype=np.float64), with_scale


@functools.lru_cache(maxsize=None)
def pair(name):
    """(source mesh, target mesh) of a case: bumpy(2) and its vertices under the case's transform, float64 then cast."""
    v, f = R.bumpy(2)
    s, rot, t, _ = _truth(name)
    return (v, f), (R.moved_copy(v, s, rot, t), f)


def _errors(res, name):
    s, rot, t, _ = _truth(name)
    return (math.degrees(R.angle_of(np.asarray(res['rotation']) @ rot.T)), float(np.linalg.norm(np.asarray(res['translation']) - t)),
            abs(res['scale'] - s))


def _recovered(res, name):
    deg, dt, ds = _errors(res, name)
    print(f"case {name}: {res['iterations']} iterations, converged {res['converged']}, rotation {deg:.3e} deg, translation "
          f"{dt:.3e}, scale {ds:.3e}, rms {[round(h['rms'], 9) for h in res['history']]}")
    assert res['converged'] and res['iterations'] <= 12
    assert deg <= 1e-3 and dt <= 1e-5 and ds <= 1e-5


# ---- hn_reg_transform -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def transform_points_in():
    p = MD.hash_points(31, 1000, -2.0, 2.0)
    p[5] = 0.0
    p[3] = (np.nan, 0.5, 0.5)
    p[64] = (0.25, -np.inf, 1.0)
    p[999] = (np.inf, np.nan, 0.0)
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1000))
def test_transform_matches_the_restatement(n):
    p = transform_points_in()[:n]
    for s, deg, t in ((1.2, 25.0, (0.15, -0.1, 0.1)), (1.0, 0.0, (0, 0, 0)), (1 / 1.2, 170.0, (-3.0, 2.0, 0.7))):
        rot = R.axis_angle((1, 2, 3), deg)
        got = OPS.transform_points(_t(p), s, rot, t).cpu().numpy()
        want = R.transform(p, s, rot, t)
        assert got.tobytes() == want.tobytes(), (n, s, deg, np.flatnonzero((got != want).any(axis=1))[:5])
        got = OPS.transform_points(_t(p), s, rot, t, direction=True).cpu().numpy()
        want = R.transform(p, s, rot, t, direction=True)
        assert got.tobytes() == want.tobytes(), (n, "direction", np.flatnonzero((got != want).any(axis=1))[:5])
    if n > 64:
        assert np.isnan(want[3]).all() and np.isnan(want[64]).all() and (want[5] == 0).all() and np.isfinite(want[6]).all()
        norms = np.linalg.norm(want[np.isfinite(want).all(axis=1)].astype(np.float64), axis=1)
        assert ((np.abs(norms - 1.0) <= 2.0 ** -22) | (norms == 0)).all() and (norms == 0).sum() == 1


# ---- hn_reg_moments -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moment_inputs(target):
    """1000 points around a mesh with their brute-force nearest points (float32 NumPy, max_distance 0.3 of the mesh's
    longest side: some queries are rejected and carry +inf, -1, NaN), the packed triangles, and a threshold that equals one
    of the distances."""
    v, f = R.bumpy(1) if target == 'bumpy' else with_degenerate()
    lo, hi = v.min(axis=0), v.max(axis=0)
    near = (v[np.arange(40) % len(v)].astype(np.float64) * 1.07 + 0.01).astype(F32)
    wide = (MD.hash_points(41, 960, -0.3, 1.3) * (hi - lo)[None] + lo[None]).astype(F32)
    p = np.concatenate([near, wide]).astype(F32)
    q = MD.point_mesh_distance(p, v, f, max_distance=0.3 * float((hi - lo).max()))
    finite = np.sort(q['distance'][np.isfinite(q['distance'])])
    tau = finite[len(finite) // 2]
    rejected = ~np.isfinite(q['distance'])
    assert 50 < rejected.sum() < 900 and (q['face'][rejected] == -1).all() and np.isnan(q['closest'][rejected]).all()
    assert (q['distance'] < tau).sum() > 100 and (q['distance'] == tau).sum() >= 1 and (q['distance'][~rejected] > tau).sum() > 100
    for a in (p, q['closest'], q['distance'], q['face']):
        a.setflags(write=False)
    return p, q, R.pack_triangles(v, f), tau


def _moments_on_device(p, q, tri, tau, mode, n_blocks, n):
    query = {'closest': _t(q['closest'][:n]), 'distance': _t(q['distance'][:n]), 'face': _t(q['face'][:n])}
    return OPS.registration_moments(_t(p[:n]), query, _t(tri), torch.full((1,), float(tau), dtype=torch.float32, device=DEV),
                                    mode, n_blocks)


def _check_moments(target, mode, n):
    p, q, tri, tau_eq = moment_inputs(target)
    counts = []
    for tau in (tau_eq, F32(np.inf)):
        for n_blocks in (1, 2, 3, None):
            got = _moments_on_device(p, q, tri, tau, mode, n_blocks, n)
            again = _moments_on_device(p, q, tri, tau, mode, n_blocks, n)
            assert torch.equal(got.view(torch.int64), again.view(torch.int64)), "two runs differ"
            got = got.cpu().numpy()
            want = R.moments(p[:n], q['closest'][:n], q['distance'][:n], q['face'][:n], tri, tau, mode, n_blocks)
            if got.tobytes() != want.tobytes():
                bound = R.moments_bound(p[:n], q['closest'][:n], q['distance'][:n], q['face'][:n], tri, tau, mode)
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"{target} {mode} n={n} blocks={n_blocks} tau={tau}: sums {bad.tolist()} differ, got "
                                     f"{got[bad[:4]]}, want {want[bad[:4]]}, |diff| / bound {np.abs(got - want)[bad[:4]] / bound[bad[:4]]}")
            assert np.isfinite(got).all()
            counts.append(got[0])
    return counts


@pytest.mark.parametrize("n", SIZES)
def test_point_moments_match_the_restatement(n):
    """Bit for bit: every product of two float32 values is exact in float64, so only the additions round, and their order
    is the documented one."""
    counts = _check_moments('bumpy', 'point', n)
    p, q, tri, tau = moment_inputs('bumpy')
    d = q['distance'][:n]
    assert counts[0] == (d <= tau).sum() and counts[4] == np.isfinite(d).sum() and counts[0] >= 1
    if n == 1000:
        assert counts[0] < counts[4] < n


@pytest.mark.parametrize("target", ['bumpy', 'degenerate'])
@pytest.mark.parametrize("n", SIZES)
def test_plane_moments_match_the_restatement(target, n):
    """Bit for bit, the normal's sqrt and divisions included.  Points whose nearest face has no area ('degenerate': faces
    0, 2 and 4) are excluded: the count is below the point-mode count of the same inputs."""
    counts = _check_moments(target, 'plane', n)
    if target == 'degenerate' and n == 1000:
        p, q, tri, tau = moment_inputs(target)
        on_flat = np.isin(q['face'], (0, 2, 4))
        assert on_flat.sum() > 50 and counts[4] == (np.isfinite(q['distance']) & ~on_flat).sum()
        point = _moments_on_device(p, q, tri, F32(np.inf), 'point', None, n).cpu().numpy()
        assert point[0] == np.isfinite(q['distance']).sum() > counts[4]


def test_default_block_count_at_a_larger_size():
    """60000 points: the default launch has 30 workgroups, every thread more than one point.  Against the restatement, both
    modes; the inputs are the 1000 of the other tests repeated."""
    p, q, tri, tau = moment_inputs('bumpy')
    reps = 60
    big = {k: np.concatenate([a] * reps) for k, a in q.items()}
    bp = np.concatenate([p] * reps)
    assert OPS.default_moment_blocks(len(bp)) == 30
    for mode in ('point', 'plane'):
        got = _moments_on_device(bp, big, tri, tau, mode, None, len(bp)).cpu().numpy()
        want = R.moments(bp, big['closest'], big['distance'], big['face'], tri, tau, mode)
        assert got.tobytes() == want.tobytes(), (mode, np.flatnonzero(got != want))


# ---- the loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_plane_method_recovers_the_transform(name):
    (sv, sf), (tv, tf) = pair(name)
    res = G.register_mesh(_dev(sv, sf), _dev(tv, tf), n_samples=1500, seed=5, method='plane', with_scale=_truth(name)[3])
    _recovered(res, name)
    assert np.abs(res['matrix'] - R.matrix_of(res['scale'], res['rotation'], res['translation'])).max() == 0
    assert res['inliers'] == 1500 and len(res['history']) == res['iterations'] and res['rms'] == res['history'][-1]['rms']
    assert res['rms'] < 1e-5 < res['history'][0]['rms']
    again = G.register_mesh(_dev(sv, sf), G.build_distance_grid(_dev(tv, tf)), n_samples=1500, seed=5, method='plane',
                            with_scale=_truth(name)[3])
    assert (again['matrix'] == res['matrix']).all() and again['history'] == res['history']      # a grid for a target; same bits


def test_point_method_is_slow_but_monotone():
    """Point to point creeps along a smooth surface: 30 iterations bring 10 degrees down to about 2.  The
    rms never grows by more than 1 % in a step."""
    (sv, sf), (tv, tf) = pair('a')
    res = G.register_mesh(_dev(sv, sf), _dev(tv, tf), n_samples=1500, seed=5, method='point', max_iterations=30)
    deg, dt, _ = _errors(res, 'a')
    rms = [h['rms'] for h in res['history']]
    print(f"point to point: {res['iterations']} iterations, rotation {deg:.3f} deg, translation {dt:.3e}, rms {rms[0]:.5f} -> {rms[-1]:.5f}")
    assert all(b <= 1.01 * a for a, b in zip(rms, rms[1:]))
    assert deg < 5.0 and res['scale'] == 1.0 and res['iterations'] <= 30


def test_trimming_sets_a_floater_aside():
    """bumpy(2) with a small sphere beside it (9 % of the samples) against the plain target: trim = 0.8 recovers the
    transform, trim = 1 is pulled more than 5 degrees off.  The first iteration's inliers are the samples within the
    ceil(0.8 * 1500)-th smallest distance, ties included."""
    (sv, sf), (tv, tf) = pair('a')
    fv, ff = R.with_floater(sv, sf)
    src, tgt = _dev(fv, ff), _dev(tv, tf)
    samples = G.sample_surface(src, 1500, seed=5)
    share = float((samples['face'] >= len(sf)).float().mean())
    assert 0.05 < share < 0.15
    res = G.register_mesh(src, tgt, n_samples=1500, seed=5, method='plane', trim=0.8)
    _recovered(res, 'a')
    d = G.point_mesh_distance(samples['points'], tgt)['distance'].cpu().numpy()
    tau = np.sort(d)[math.ceil(0.8 * 1500) - 1]
    assert res['history'][0]['inliers'] == (d <= tau).sum() >= 1200
    assert all(1200 <= h['inliers'] <= 1210 for h in res['history']) and res['inliers'] == res['history'][-1]['inliers']
    off = G.register_mesh(src, tgt, n_samples=1500, seed=5, method='plane', trim=1.0)
    deg = _errors(off, 'a')[0]
    print(f"trim 1.0: {off['iterations']} iterations, converged {off['converged']}, rotation {deg:.2f} deg off")
    assert deg > 5.0 and off['inliers'] == 1500


def test_planar_target_gives_a_finite_step():
    """A flat target leaves sliding and spinning in the plane free: the normal equations have rank 3, the minimum-norm
    solution moves only what the residuals see."""
    qv, qf = MD.planar_quad()
    src = R.moved_copy(qv, 1.0, R.axis_angle((1, 0, 0), 5.0), (0.0, 0.0, 0.05))
    res = G.register_mesh(_dev(src, qf), _dev(qv, qf), n_samples=1500, seed=5, method='plane')
    print(f"planar: {res['iterations']} iterations, converged {res['converged']}, rms {res['history'][0]['rms']:.5f} -> {res['rms']:.3e}")
    assert np.isfinite(res['matrix']).all() and np.isfinite(res['rms']) and res['rms'] < res['history'][0]['rms']
    assert res['inliers'] == 1500


def test_too_few_inliers_name_the_iteration():
    (sv, sf), (tv, tf) = pair('a')
    far = R.moved_copy(sv, 1.0, np.eye(3), (5.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="iteration 1 .* 0 inliers"):
        G.register_mesh(_dev(far, sf), _dev(tv, tf), n_samples=500, max_distance=0.1)
    pts = G.sample_surface(_dev(sv, sf), 5, seed=1)['points']
    with pytest.raises(ValueError, match="iteration 1 .* 5 inliers"):
        G.register_mesh(pts, _dev(tv, tf))
    assert G.register_mesh(pts, _dev(tv, tf), method='point', max_iterations=2)['inliers'] == 5


def test_inits():
    """A (4, 4) init near the answer converges at once; 'centroid' brings a far-off copy within reach."""
    (sv, sf), (tv, tf) = pair('b')
    s, rot, t, _ = _truth('b')
    res = G.register_mesh(_dev(sv, sf), _dev(tv, tf), n_samples=1500, seed=5, with_scale=True, init=R.matrix_of(s, rot, t))
    assert res['converged'] and res['iterations'] <= 2
    _recovered(res, 'b')
    away = R.moved_copy(tv, 1.0, np.eye(3), (4.0, -3.0, 2.0))
    with pytest.raises(ValueError, match="inliers"):
        G.register_mesh(_dev(sv, sf), _dev(away, tf), n_samples=1500, seed=5, with_scale=True, max_distance=1.0)
    res = G.register_mesh(_dev(sv, sf), _dev(away, tf), n_samples=1500, seed=5, with_scale=True, max_distance=1.0, init='centroid')
    assert res['converged'] and abs(res['scale'] - s) <= 1e-5
    assert np.linalg.norm(res['translation'] - (t + np.array([4.0, -3.0, 2.0]))) <= 1e-5


# ---- transform_mesh / aligned_mesh_distance ---------------------------------------------------------------------------------
def test_aligned_distance():
    (sv, sf), (tv, tf) = pair('b')
    a, b = _dev(sv, sf), _dev(tv, tf)
    normals = (sv / np.linalg.norm(sv, axis=1, keepdims=True)).astype(F32)
    normals[7] = 0.0
    a['normals'] = _t(normals)
    a['colors'] = torch.arange(3 * len(sv), dtype=torch.uint8, device=DEV).reshape(-1, 3)
    apart = G.mesh_distance(a, b, n_samples=20000, seed=3)
    rep = G.aligned_mesh_distance(a, b, register=dict(n_samples=1500, seed=5, with_scale=True), n_samples=20000, seed=3)
    print(f"chamfer: unaligned {apart['chamfer']:.4f}, aligned {rep['chamfer']:.3e}")
    assert apart['chamfer'] > 1e-2 and rep['chamfer'] < 1e-5
    _recovered(rep['alignment'], 'b')
    moved = G.transform_mesh(a, rep['alignment']['matrix'])
    assert moved['faces'] is a['faces'] and moved['colors'] is a['colors'] and set(moved) == set(a)
    again = G.mesh_distance(moved, b, n_samples=20000, seed=3)
    assert again == {k: v for k, v in rep.items() if k != 'alignment'}
    s, rot, t = OPS.split_similarity(rep['alignment']['matrix'])
    assert moved['vertices'].cpu().numpy().tobytes() == R.transform(sv, s, rot, t).tobytes()
    got = moved['normals'].cpu().numpy()
    assert got.tobytes() == R.transform(normals, 1.0, rot, np.zeros(3), direction=True).tobytes()
    lengths = np.linalg.norm(got.astype(np.float64), axis=1)
    assert (got[7] == 0).all() and np.abs(np.delete(lengths, 7) - 1.0).max() <= 2.0 ** -22
    assert float((moved['vertices'] - b['vertices']).abs().max()) < 1e-4      # 1e-3 deg at radius 1.5, 1e-5 each of t and s
    with pytest.raises(ValueError, match="determinant"):
        G.transform_mesh(a, np.diag([1.0, 1.0, -1.0, 1.0]))
