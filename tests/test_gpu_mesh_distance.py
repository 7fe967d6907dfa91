"""GPU tests of the mesh distance (csrc/hn_mesh_distance.hip, geometry.sample_surface / point_mesh_distance /
mesh_distance / distance_colors): the kernels against the NumPy float32 restatement of the definition
(tests/mesh_distance_restated.py), bit for bit — samples, distances, closest points, face ids — at every grid
resolution, with the queries sorted or not; special values, max_distance, the statistics of mesh_distance, and a bound
that follows from the simplifier's definition."""
import functools

import numpy as np
import pytest
import torch

import mesh_distance_restated as R
from gpu_common import DEV
from hypernerf_torch_amd import geometry as G

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 63, 64, 65, 1000)
RESOLUTIONS = (1, 2, 3, 7, 17, (5, 1, 9), None)


def _dev(v, f):
    return {'vertices': torch.from_numpy(np.array(v, dtype=F32)).to(DEV), 'faces': torch.from_numpy(np.array(f, dtype=np.int32)).to(DEV)}


def _same_bits(got: torch.Tensor, want: np.ndarray, what=""):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.reshape(got.shape[0], -1).view(np.uint32 if got.itemsize == 4 else np.uint8)
                              != want.reshape(want.shape[0], -1).view(np.uint32 if want.itemsize == 4 else np.uint8)).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} rows differ, first {bad[:5]}: got {got[bad[:5]]}, want {want[bad[:5]]}")


def _same_result(got, want, what=""):
    _same_bits(got['face'], want['face'], what + " face")
    _same_bits(got['distance'], want['distance'], what + " distance")
    _same_bits(got['closest'], want['closest'], what + " closest")


def big_and_small():
    """One triangle across the whole box [0, 1]^3 — it is listed in most cells of a 17^3 grid — next to two small spheres."""
    v0, f0 = np.array([[0, 0, 0], [1, 1, 0], [0.5, 0.5, 1]], dtype=F32), np.array([[0, 1, 2]], dtype=np.int32)
    v1, f1 = R.icosphere(1, 0.06)
    v2, f2 = R.icosphere(0, 0.03)
    return (np.concatenate([v0, v1 + F32([0.2, 0.75, 0.3]), v2 + F32([0.85, 0.2, 0.7])]).astype(F32),
            np.concatenate([f0, f1 + 3, f2 + 3 + len(v1)]).astype(np.int32))


def with_degenerate():
    """Two triangles of areas 3 and 1 among faces without area (collinear, a point): ids 1 and 3 carry the surface."""
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 5, 5], [7, 5, 5], [5, 6, 5], [1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=F32)
    return v, np.array([[6, 7, 8], [0, 1, 2], [6, 6, 6], [3, 4, 5], [7, 8, 6]], dtype=np.int32)


MESHES = {'triangle': R.one_triangle, 'cube': lambda: R.cube(0.5), 'ico80': lambda: R.icosphere(1),
          'ico320': lambda: R.icosphere(2), 'quad': R.planar_quad, 'big_small': big_and_small, 'degenerate': with_degenerate}


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f = MESHES[name]()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def queries(name):
    """1000 query points for a mesh, the edge cases first so that the short prefixes hold some: its vertices; points on the
    cell boundaries lo + i * cell of the tested resolutions; the box centre and points with at least 3 empty shells around
    them; points up to 10 box sizes outside on every side; hash-drawn points inside the box and around it."""
    v, _ = mesh(name)
    lo, hi = v.min(axis=0), v.max(axis=0)
    size = np.maximum(hi - lo, F32(0.5) * (hi - lo).max()).astype(F32)
    mid = ((lo + hi) / 2).astype(F32)
    parts = [mid[None], v[:40]]
    for r in (2, 3, 7, 17, 9):
        cell = ((hi - lo) / F32(r)).astype(F32)
        i = np.arange(r + 1, dtype=F32)[:, None]
        edge = (lo[None] + (i * cell[None]).astype(F32)).astype(F32)
        parts += [edge, np.stack([edge[:, 0], edge[::-1, 1], mid[2] + 0 * edge[:, 2]], axis=-1)]
    for axis in range(3):
        for sign in (-1, 1):
            for k in (0.6, 1.5, 10.0):
                p = mid.copy()
                p[axis] += F32(sign * k) * size[axis]
                parts.append(p[None])
    parts.append(np.stack([mid + F32(s * 10) * size for s in (-1, 1)]))
    near = R.hash_points(21, 400, 0.0, 1.0) * (hi - lo)[None] + lo[None]
    wide = R.hash_points(22, 1000, -1.0, 2.0) * size[None] + (mid - size / 2)[None]
    far = R.hash_points(23, 40, -10.0, 10.0) * size[None] + mid[None]
    pts = np.concatenate(parts + [far, near, wide]).astype(F32)[:1000]
    assert pts.shape == (1000, 3)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float32 brute force over all 1000 queries, once per mesh; a prefix of the queries has the prefix of it."""
    v, f = mesh(name)
    out = R.point_mesh_distance(queries(name), v, f)
    for a in out.values():
        a.setflags(write=False)
    return out


def _prefix(ref, n):
    return {k: a[:n] for k, a in ref.items()}


# ---- sampling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ['cube', 'ico320', 'degenerate'])
def test_samples_match_the_restatement(name, n):
    v, f = mesh(name)
    got = G.sample_surface(_dev(v, f), n, seed=n + 3)
    want = R.sample_surface(v, f, n, seed=n + 3)
    _same_bits(got['face'], want['face'], "face")
    _same_bits(got['bary'], want['bary'], "bary")
    _same_bits(got['points'], want['points'], "points")
    if name == 'degenerate':
        assert set(want['face'].tolist()) <= {1, 3}


def test_samples_are_reproducible_and_seeded():
    m = _dev(*mesh('ico320'))
    a, b, c = G.sample_surface(m, 5000, seed=9), G.sample_surface(m, 5000, seed=9), G.sample_surface(m, 5000, seed=10)
    for k in a:
        assert torch.equal(a[k], b[k])
    assert not torch.equal(a['points'], c['points'])
    assert torch.equal(G.sample_surface(m, 100, seed=9)['points'], a['points'][:100])
    assert torch.equal(G.sample_surface(m, 10, seed=-1)['face'], G.sample_surface(m, 10, seed=2 ** 64 - 1)['face'])


def test_sampling_refuses_bad_meshes():
    v, f = mesh('cube')
    bad = _dev(v, f)
    bad['faces'] = bad['faces'].clone()
    bad['faces'][5, 1] = 8
    with pytest.raises(ValueError, match="vertex id"):
        G.sample_surface(bad, 10)
    with pytest.raises(ValueError, match="vertex id"):
        G.point_mesh_distance(torch.zeros((3, 3), device=DEV), bad)
    flat = _dev(np.ones((3, 3), dtype=F32), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="area"):
        G.sample_surface(flat, 10)
    nan = _dev(v.copy(), f)
    nan['vertices'][3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        G.point_mesh_distance(torch.zeros((3, 3), device=DEV), nan)


# ---- point distance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", RESOLUTIONS, ids=str)
@pytest.mark.parametrize("name", ['triangle', 'cube', 'ico80', 'ico320', 'quad', 'big_small'])
def test_distance_matches_brute_force(name, res):
    v, f = mesh(name)
    got = G.point_mesh_distance(torch.from_numpy(queries(name).copy()).to(DEV), _dev(v, f), grid_resolution=res)
    _same_result(got, reference(name), f"{name} R={res}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("res", [1, 7, None], ids=str)
def test_distance_at_every_size(res, n):
    v, f = mesh('ico80')
    pts = torch.from_numpy(queries('ico80')[:n].copy()).to(DEV)
    for sort in (True, False):
        got = G.point_mesh_distance(pts, _dev(v, f), grid_resolution=res, sort_queries=sort)
        _same_result(got, _prefix(reference('ico80'), n), f"n={n} R={res} sort={sort}")


def test_the_query_sets_hold_the_edge_cases():
    """What the bit-equality tests above rest on: queries on cell boundaries, mesh vertices (distance 0), points 10 box
    sizes out, and queries whose cell has at least 3 empty shells around it on the 17^3 grid of the sphere."""
    v, f = mesh('ico320')
    q, ref = queries('ico320'), reference('ico320')
    assert (ref['distance'][1:41] == 0).all() and (ref['face'][1:41] >= 0).all()
    assert (np.abs(q).max(axis=1) > 9.0).sum() >= 8
    cell = F32(2.0 / 17)
    assert ((ref['distance'] > 4 * np.sqrt(3) * cell) & (np.abs(q).max(axis=1) < 1)).sum() >= 1      # e.g. the centre
    grid = G.build_distance_grid(_dev(v, f), 17)
    assert grid['resolution'] == (17, 17, 17) and grid['cell_begin'].shape[0] == 17 ** 3 + 1
    begin, pair_face = grid['cell_begin'].cpu().numpy(), grid['pair_face'].cpu().numpy()
    assert begin[0] == 0 and begin[-1] == pair_face.shape[0] and (np.diff(begin) >= 0).all()
    assert (np.diff(begin) == 0).mean() > 0.5                                                          # most cells are empty
    for c in np.flatnonzero(np.diff(begin) > 1)[:50]:
        assert (np.diff(pair_face[begin[c]:begin[c + 1]]) > 0).all()                                   # ids ascend within a cell
    big = G.build_distance_grid(_dev(*mesh('big_small')), 17)
    assert int((big['pair_face'] == 0).sum()) > 17 * 17                                              # the big triangle is in many cells
    assert G.build_distance_grid(_dev(*mesh('quad')), 7)['resolution'] == (7, 7, 1)                  # the zero-extent axis


def test_sorted_unsorted_and_repeated_runs_give_equal_bits():
    v, f = mesh('ico320')
    pts = torch.from_numpy(queries('ico320').copy()).to(DEV).repeat(20, 1)                                  # 20000 queries, many blocks
    grid = G.build_distance_grid(_dev(v, f))
    runs = [G.point_mesh_distance(pts, grid, sort_queries=s) for s in (True, False, True, False)]
    for r in runs[1:]:
        for k in r:
            assert torch.equal(r[k].view(torch.int32), runs[0][k].view(torch.int32)), k
    _same_result({k: t[-1000:] for k, t in runs[0].items()}, reference('ico320'), "tail")


def test_special_values_do_not_disturb_their_neighbours():
    v, f = mesh('ico320')
    q = queries('ico320')[:256].copy()
    want = {k: a[:256].copy() for k, a in reference('ico320').items()}
    holes = {3: (np.nan, 0, 0), 64: (0, np.inf, 0), 65: (0, 0, -np.inf), 130: (np.nan, np.nan, np.nan), 255: (np.inf, np.nan, 1)}
    for i, p in holes.items():
        q[i] = p
        want['distance'][i], want['face'][i], want['closest'][i] = np.nan, -1, np.nan
    for res in (1, 7, None):
        for sort in (True, False):
            got = G.point_mesh_distance(torch.from_numpy(q).to(DEV), _dev(v, f), grid_resolution=res, sort_queries=sort)
            _same_result(got, want, f"R={res} sort={sort}")
    again = R.point_mesh_distance(q, v, f)
    assert again['distance'].tobytes() == want['distance'].tobytes()


def test_an_empty_mesh_is_infinitely_far():
    m = {'vertices': torch.zeros((4, 3), device=DEV), 'faces': torch.zeros((0, 3), dtype=torch.int32, device=DEV)}
    got = G.point_mesh_distance(torch.from_numpy(queries('cube')[:70].copy()).to(DEV), m)
    assert torch.isinf(got['distance']).all() and (got['distance'] > 0).all() and (got['face'] == -1).all()
    assert torch.isnan(got['closest']).all()
    none = G.point_mesh_distance(torch.zeros((0, 3), device=DEV), _dev(*mesh('cube')))
    assert none['distance'].shape == (0,) and none['closest'].shape == (0, 3)


@pytest.mark.parametrize("res", [1, 3, 17, None], ids=str)
def test_max_distance(res):
    """Every query within max_distance keeps its brute-force result, the rest get +inf, -1, NaN; the cube's closed form puts
    queries exactly at the threshold 0.25 (the corners of the cube of half-side 0.75 are farther, sqrt(0.1875))."""
    v, f = mesh('cube')
    outer, _ = R.cube(0.75)
    at = np.array([[0.75, 0.5, 0.5], [0.75, 0, 0], [0, -0.75, 0.25], [-0.5, 0.5, 0.75]], dtype=F32)
    q = np.concatenate([at, outer, queries('cube')])[:1000]
    want = R.point_mesh_distance(q, v, f, max_distance=0.25)
    full = R.point_mesh_distance(q, v, f)
    assert (want['distance'][:4] == F32(0.25)).all() and np.isinf(want['distance'][4:12]).all()
    inside = full['distance'] <= F32(0.25)
    assert 100 < inside.sum() < 900
    assert want['distance'][inside].tobytes() == full['distance'][inside].tobytes() and (want['face'][~inside] == -1).all()
    for sort in (True, False):
        got = G.point_mesh_distance(torch.from_numpy(q).to(DEV), _dev(v, f), max_distance=0.25, grid_resolution=res,
                                    sort_queries=sort)
        _same_result(got, want, f"R={res} sort={sort}")
    zero = G.point_mesh_distance(torch.from_numpy(q).to(DEV), _dev(v, f), max_distance=0.0, grid_resolution=res)
    _same_result(zero, R.point_mesh_distance(q, v, f, max_distance=0.0), "max_distance=0")


# ---- mesh_distance -----------------------------------------------------------------------------------------------------------
def _check_stats(out):
    """Every statistic against NumPy's float64 reduction of the returned fp32 distances, to 1e-12 relative."""
    ab, ba = (out[k].cpu().numpy().astype(np.float64) for k in ('distances_ab', 'distances_ba'))
    want = {'a_to_b': ab, 'b_to_a': ba}
    for side, d in want.items():
        for key, val in (('mean', d.mean()), ('rms', np.sqrt((d * d).mean())), ('max', d.max())):
            assert isinstance(out[side][key], float)
            assert out[side][key] == pytest.approx(val, rel=1e-12, abs=0), (side, key)
    assert out['chamfer'] == pytest.approx((ab.mean() + ba.mean()) / 2, rel=1e-12, abs=0)
    assert out['chamfer_l2'] == pytest.approx(((ab * ab).mean() + (ba * ba).mean()) / 2, rel=1e-12, abs=0)
    assert out['hausdorff'] == max(ab.max(), ba.max())
    for tau, s in out.get('thresholds', {}).items():
        p, r = (ab <= tau).mean(), (ba <= tau).mean()
        assert s['precision'] == pytest.approx(p, rel=1e-12, abs=0) and s['recall'] == pytest.approx(r, rel=1e-12, abs=0)
        assert s['fscore'] == pytest.approx(2 * p * r / (p + r) if p + r > 0 else 0.0, rel=1e-12, abs=0)
    assert out['n'] == (ab.size, ba.size)


def test_mesh_distance_of_concentric_cubes():
    a, b = _dev(*R.cube(0.5)), _dev(*R.cube(0.75))
    out = G.mesh_distance(a, b, n_samples=20000, seed=4, thresholds=[0.5, 0.3, 0.2], with_vertices=True, return_distances=True)
    assert out['n'] == (20008, 20008)
    assert out['b_to_a']['max'] == float(np.sqrt(F32(0.1875)))
    assert out['hausdorff'] == out['b_to_a']['max']
    # every point of the inner cube is 0.25 from the outer one: fewer than sixteen roundings of values below 1, 6e-8 each
    assert float((out['distances_ab'] - 0.25).abs().max()) <= 1e-6
    assert out['a_to_b']['mean'] == pytest.approx(0.25, abs=1e-6) and out['a_to_b']['rms'] == pytest.approx(0.25, abs=1e-6)
    assert out['thresholds'][0.5] == {'precision': 1.0, 'recall': 1.0, 'fscore': 1.0}
    # no point of either cube is nearer than 0.25 to the other: at 0.2 both shares are 0 and the F-score takes its P + R == 0
    # branch; between 0.25 and sqrt(0.1875) all of the inner cube, and the part of the outer one away from its edges, is within
    assert out['thresholds'][0.2] == {'precision': 0.0, 'recall': 0.0, 'fscore': 0.0}
    at = out['thresholds'][0.3]
    assert at['precision'] == 1.0 and 0.0 < at['recall'] < 1.0 and 0.0 < at['fscore'] < 1.0
    _check_stats(out)
    plain = G.mesh_distance(a, b, n_samples=20000, seed=4)
    assert 'thresholds' not in plain and 'distances_ab' not in plain and plain['n'] == (20000, 20000)
    assert plain['a_to_b']['mean'] == pytest.approx(0.25, abs=1e-6)
    assert G.mesh_distance(a, b, n_samples=20000, seed=4) == plain


def test_mesh_distance_to_itself():
    a = _dev(*R.icosphere(2))
    out = G.mesh_distance(a, a, n_samples=20000, seed=1, thresholds=1e-6, with_vertices=True, return_distances=True)
    assert out['hausdorff'] < 1e-6 and float(out['distances_ab'].max()) < 1e-6 and float(out['distances_ba'].max()) < 1e-6
    assert out['thresholds'][1e-6]['fscore'] == 1.0
    assert not torch.equal(out['distances_ab'][:100], out['distances_ba'][:100])      # b is sampled with seed + 1
    _check_stats(out)


@pytest.mark.parametrize("placement", ['mean', 'quadric'])
def test_against_the_simplifier(placement):
    """A representative stays inside its cell and its cell holds an original vertex, which lies on the original mesh: every
    vertex of simplify_mesh(mesh, cell) is within the cell's diagonal cell * sqrt(3) of the original mesh; and the
    Chamfer distance between the two grows with the cell."""
    v, f = R.icosphere(3)
    assert f.shape == (1280, 3)
    m = _dev(v, f)
    m['normals'] = m['vertices'] / m['vertices'].norm(dim=1, keepdim=True)
    chamfer = []
    for cell in (0.1, 0.2, 0.4):
        small = G.simplify_mesh(m, cell, placement=placement)
        assert 0 < small['faces'].shape[0] <= 1280          # cells of 0.1 are finer than the sphere's edges: little or nothing merges
        d = G.point_mesh_distance(small['vertices'], m)['distance']
        print(f"cell {cell}: {small['faces'].shape[0]} faces, max vertex distance {float(d.max()):.4f}, "
              f"bound {cell * np.sqrt(3):.4f}")
        assert float(d.max()) <= cell * np.sqrt(3) * (1 + 1e-5)
        chamfer.append(G.mesh_distance(m, small, n_samples=20000, seed=2)['chamfer'])
    print("chamfer", chamfer)
    assert 0 <= chamfer[0] < chamfer[1] < chamfer[2]


# ---- distance_colors ---------------------------------------------------------------------------------------------------------
def test_distance_colors_on_the_device():
    from hypernerf_torch_amd import inference
    lut = inference.jet_lut().flip(1)
    v, f = mesh('cube')
    d = G.point_mesh_distance(torch.from_numpy(R.cube(0.75)[0]).to(DEV), _dev(v, f))['distance']
    d = torch.cat([torch.zeros(1, device=DEV), d, torch.tensor([float("nan"), float("inf"), 0.3], device=DEV)])
    c = G.distance_colors(d, vmax=0.3)
    assert c.device == d.device and c.dtype == torch.uint8 and tuple(c.shape) == (12, 3)
    c = c.cpu()
    assert (c[0] == lut[0]).all() and (c[1:] == lut[255]).all()
