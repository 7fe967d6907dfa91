"""CPU tests of mesh simplification by vertex clustering: the properties of the definition (tests/simplify_restated.py,
the NumPy float32 restatement of csrc/hn_simplify.hip) on isosurfaces of analytic fields, what quadric placement buys
over the mean, the float32 solve against a float64 one, meshes made by hand, and the argument checks of
geometry.simplify_mesh / extract_mesh that run before any kernel."""
import functools

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import isosurface_restated as R
import simplify_restated as S
import test_isosurface_host as HT
from hypernerf_torch_amd import _lib as L

FIELDS = {"sphere9": (HT.sphere, 9), "sphere17": (HT.sphere, 17), "sphere33": (HT.sphere, 33), "torus33": (HT.torus, 33),
          "two_spheres25": (HT.two_spheres, 25)}
FACTORS = (0.25, 1, 2, 3, 4)
ORIGIN = (-1.0, -1.0, -1.0)


@functools.lru_cache(maxsize=None)
def fine(name):
    build, n = FIELDS[name]
    return R.extract_isosurface(build(n), 0.0, HT.UNIT), 2.0 / (n - 1)


@functools.lru_cache(maxsize=None)
def simplified(name, k, placement="quadric"):
    mesh, spacing = fine(name)
    return S.simplify_mesh(mesh, k * spacing, ORIGIN, placement)


@pytest.mark.parametrize("k", FACTORS)
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_properties_of_the_definition(name, k):
    mesh, spacing = fine(name)
    out = simplified(name, k)
    v, f, vc = out["vertices"], out["faces"], out["vertex_cluster"]
    assert v.dtype == np.float32 and f.dtype == np.int32 and vc.dtype == np.int32 and out["normals"].shape == v.shape
    assert f.shape[0] > 0 and f.min() == 0 and f.max() == v.shape[0] - 1 and np.unique(f).size == v.shape[0]
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all(), "every face starts with its smallest vertex"
    triple = np.stack([f[:, 0], f[:, 1:].min(axis=1), f[:, 1:].max(axis=1)], axis=1).astype(np.int64)
    order = np.lexsort((triple[:, 2], triple[:, 1], triple[:, 0]))
    assert np.array_equal(triple[order], triple), "the sorted triples ascend"
    # the boundary of the face chain stays zero, and no oriented face occurs twice on these meshes
    assert S.edge_balance(mesh["faces"]) and S.edge_balance(f)
    assert S.max_net_multiplicity(f) == 1
    c = R.check_mesh(v, f)
    print(f"{name} k={k}: V {mesh['vertices'].shape[0]} -> {v.shape[0]}, F {mesh['faces'].shape[0]} -> {f.shape[0]}, "
          f"closed {c['closed']} oriented {c['oriented']} euler {c['euler']}")
    if name.startswith("sphere"):
        assert c["closed"] and c["oriented"] and c["euler"] == 2 and c["volume"] > 0, c
    if name == "two_spheres25":
        assert c["euler"] == 4, c
    # vertex_cluster against the outputs
    clusters = S.cluster_vertices(mesh["vertices"], k * spacing, ORIGIN)
    cid = clusters["vertex_cluster"]
    assert vc.shape == (mesh["vertices"].shape[0],) and vc.max() == v.shape[0] - 1 and vc.min() >= -1
    assert np.array_equal(np.unique(vc[vc >= 0]), np.arange(v.shape[0])), "every output vertex has members"
    for a, b in ((cid, vc), (vc[vc >= 0], cid[vc >= 0])):        # one cluster <-> one output vertex (or -1)
        pairs = np.unique(np.stack([np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)], axis=1), axis=0)
        assert np.unique(pairs[:, 0]).size == pairs.shape[0]
    kept = np.unique(cid[vc >= 0])
    assert np.array_equal(np.argsort(kept), np.arange(kept.size)) and np.array_equal(vc[vc >= 0], np.searchsorted(kept, cid[vc >= 0]))
    unused = clusters["cluster_keys"].size - v.shape[0]
    assert unused == np.unique(cid[vc < 0]).size
    if name in ("sphere9", "sphere17") and k == 3:
        assert unused == 1, "the case that needs the cancellation leaves one cluster without a face"
    # a quadric position stays inside the cell of its cluster
    idx = S.cell_indices(mesh["vertices"], k * spacing, ORIGIN)
    lo = np.float32(-1.0) + (idx.astype(np.float32) * np.float32(k * spacing)).astype(np.float32)
    hi = (lo + np.float32(k * spacing)).astype(np.float32)
    inside = vc >= 0
    assert (v[vc[inside]] >= lo[inside]).all() and (v[vc[inside]] <= hi[inside]).all()


@pytest.mark.parametrize("name", ["sphere9", "sphere17"])
def test_k3_needs_the_cancellation(name):
    """Without cancelling opposite pairs the collapsed sphere is not a closed oriented surface; with it, it is."""
    mesh, spacing = fine(name)
    clusters = S.cluster_vertices(mesh["vertices"], 3 * spacing, ORIGIN)
    f = clusters["vertex_cluster"].astype(np.int64)[mesh["faces"]]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    before = R.check_mesh(np.zeros((clusters["cluster_keys"].size, 3)), f)
    after = R.check_mesh(simplified(name, 3)["vertices"], simplified(name, 3)["faces"])
    print(f"{name}: {f.shape[0]} faces survive the collapse, {after['n_faces']} the cancellation")
    assert not (before["closed"] and before["oriented"])
    assert after["closed"] and after["oriented"] and after["euler"] == 2


def test_torus_k2_is_balanced():
    out = simplified("torus33", 2)
    c = R.check_mesh(out["vertices"], out["faces"])
    print(f"torus33 k=2: closed {c['closed']} oriented {c['oriented']} euler {c['euler']}")
    assert S.edge_balance(out["faces"])


def test_a_cell_of_40_spacings_gives_the_empty_mesh():
    for name in ("sphere9", "sphere33", "torus33"):
        mesh, spacing = fine(name)
        out = S.simplify_mesh(mesh, 40 * spacing, ORIGIN)
        assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and out["normals"].shape == (0, 3)
        assert (out["vertex_cluster"] == -1).all() and out["vertex_cluster"].shape == (mesh["vertices"].shape[0],)


def test_quadric_placement_loses_less_volume_than_the_mean():
    mesh, _ = fine("sphere33")
    full = R.check_mesh(mesh["vertices"], mesh["faces"])["volume"]
    for k in (2, 3, 4):
        loss = {}
        for placement in ("quadric", "mean"):
            out = simplified("sphere33", k, placement)
            loss[placement] = 1.0 - R.check_mesh(out["vertices"], out["faces"])["volume"] / full
        print(f"sphere33 k={k}: volume lost, quadric {loss['quadric']:.2%} mean {loss['mean']:.2%}")
        assert 0.0 < loss["quadric"] < loss["mean"], (k, loss)


@pytest.mark.parametrize("name,k", [("sphere33", 2), ("sphere33", 4), ("torus33", 3), ("two_spheres25", 4), ("sphere17", 1)])
def test_fp32_quadric_against_a_float64_solve(name, k):
    """The float32 statement's positions stay within 1e-3 * cell of a float64 solve of the same system: cond(A) <=
    (1 + 0.1) / 0.1 = 11, at most about 150 members, every term <= sqrt(3) * cell, so the worst-case linear bound is
    11 * 150 * 2^-24 * sqrt(3) = 1.7e-4 * cell; 1e-3 leaves a factor of five."""
    mesh, spacing = fine(name)
    cell = np.float32(k * spacing)
    clusters = S.cluster_vertices(mesh["vertices"], cell, ORIGIN)
    got = S.reduce_clusters(mesh["vertices"], mesh["normals"], None, clusters, cell, ORIGIN)["vertices"]
    p, n = mesh["vertices"].astype(np.float64), mesh["normals"].astype(np.float64)
    cid, ckeys = clusters["vertex_cluster"], clusters["cluster_keys"]
    members = np.diff(clusters["starts"])
    assert members.max() <= 150
    worst = 0.0
    for c in range(ckeys.size):
        pc, nc = p[cid == c], n[cid == c]
        mean = pc.mean(axis=0)
        a = nc.T @ nc + 0.1 * len(pc) * np.eye(3)
        x = mean + np.linalg.solve(a, (nc * ((pc - mean) * nc).sum(axis=1, keepdims=True)).sum(axis=0))
        idx = np.array([(int(ckeys[c]) >> (21 * axis)) & (2 ** 21 - 1) for axis in range(3)], dtype=np.float64)
        lo = -1.0 + idx * float(cell)
        x = np.clip(x, lo, lo + float(cell))
        worst = max(worst, float(np.abs(got[c].astype(np.float64) - x).max()))
    print(f"{name} k={k}: {ckeys.size} clusters, up to {members.max()} members, max |fp32 - fp64| = {worst / float(cell):.2e} cells")
    assert worst <= 1e-3 * float(cell)


def test_hand_made_mesh():
    mesh, cell, origin, expect = S.hand_made()
    for placement in ("mean", "quadric"):
        out = S.simplify_mesh(mesh, cell, origin, placement)
        assert np.array_equal(out["faces"], expect["faces"]), out["faces"]
        assert np.array_equal(out["vertex_cluster"], expect["vertex_cluster"]), out["vertex_cluster"]
        assert out["vertices"].shape == (4, 3) and out["normals"].shape == (4, 3) and out["colors"].shape == (4, 3)
        assert out["colors"].dtype == np.uint8
    assert S.cluster_vertices(mesh["vertices"], cell, origin)["cluster_keys"].size == expect["n_clusters"]
    out = S.simplify_mesh(mesh, cell, origin, "mean")
    v, col = mesh["vertices"], mesh["colors"].astype(np.int64)
    two = np.float32(2)
    assert np.array_equal(out["vertices"][0], ((np.float32(0) + v[0]) + v[1]) / two)
    assert np.array_equal(out["vertices"][3], v[6])
    assert np.array_equal(out["colors"][1], (2 * (col[2] + col[3]) + 2) // 4)
    # origin None = the minimum of the vertices: other cells, and still a valid mesh
    shifted = S.simplify_mesh(mesh, cell, None, "mean")
    assert shifted["faces"].shape[1] == 3 and shifted["vertex_cluster"].shape == (9,)


def cpu_mesh(**over):
    mesh, _, _, _ = S.hand_made()
    m = {k: torch.from_numpy(a.copy()) for k, a in mesh.items()}
    m.update(over)
    return {k: t for k, t in m.items() if t is not None}


@pytest.mark.parametrize("cell", [0.0, -1.0, float("nan"), float("inf"), (1.0, 0.0, 1.0), (1.0, 2.0), "wide", 1e-50])
def test_bad_cells_are_refused(cell):
    with pytest.raises(ValueError, match="cell"):
        HN.simplify_mesh(cpu_mesh(), cell)


def test_argument_checks_run_before_any_kernel(monkeypatch):
    monkeypatch.setattr(L, "launch", lambda *a, **k: pytest.fail("a kernel was launched"))
    with pytest.raises(ValueError, match="origin"):
        HN.simplify_mesh(cpu_mesh(), 1.0, origin=(0.0, 0.25, 0.0))              # above the minimum 0.2 along y
    with pytest.raises(ValueError, match="origin"):
        HN.simplify_mesh(cpu_mesh(), 1.0, origin=(0.0, 0.0))
    with pytest.raises(ValueError, match="origin"):
        HN.simplify_mesh(cpu_mesh(), 1.0, origin=(0.0, float("nan"), 0.0))
    # an extent of 2^21 cells: the vertices span 5.3 along every axis
    with pytest.raises(ValueError, match=r"2\*\*21"):
        HN.simplify_mesh(cpu_mesh(), 5.3 / 2 ** 21, origin=(0.2, 0.2, 0.1))
    with pytest.raises(ValueError, match=r"2\*\*21"):
        HN.simplify_mesh(cpu_mesh(), (1.0, 1.0, 2.0 ** -21), origin=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="normals"):
        HN.simplify_mesh(cpu_mesh(normals=None), 1.0)
    with pytest.raises(ValueError, match="placement"):
        HN.simplify_mesh(cpu_mesh(), 1.0, placement="median")
    with pytest.raises(ValueError, match="regularization"):
        HN.simplify_mesh(cpu_mesh(), 1.0, regularization=-0.5)
    with pytest.raises(ValueError, match="finite"):
        HN.simplify_mesh(cpu_mesh(vertices=torch.full((9, 3), float("nan"))), 1.0)
    m = cpu_mesh()
    for over in (dict(vertices=m["vertices"].double()), dict(vertices=m["vertices"].reshape(-1)), dict(vertices=m["vertices"][:, :2]),
                 dict(faces=m["faces"].long()), dict(faces=m["faces"][:, :2]), dict(faces=m["faces"].numpy()),
                 dict(normals=m["normals"][:5]), dict(normals=m["normals"].double()),
                 dict(colors=m["colors"][:5]), dict(colors=m["colors"].to(torch.int32)), dict(colors=m["colors"].double())):
        with pytest.raises(ValueError, match="|".join(over)):
            HN.simplify_mesh(cpu_mesh(**over), 1.0)
    # a mesh that passes every check still needs the GPU: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        HN.simplify_mesh(cpu_mesh(), 1.0)
    with pytest.raises(ValueError, match="GPU"):
        HN.simplify_mesh(cpu_mesh(normals=None), 1.0, placement="mean")


@pytest.mark.parametrize("simplify", [0, -2.0, float("nan"), float("inf"), (1.0, 2.0), (1.0, -1.0, 1.0), "coarse"])
def test_extract_mesh_refuses_a_bad_simplify_before_it_touches_the_model(simplify):
    with pytest.raises(ValueError, match="simplify"):
        HN.extract_mesh(None, HT.UNIT, 9, 0, simplify=simplify)


def test_entry_points_are_declared_and_built():
    names = {"hn_simplify_extent", "hn_simplify_keys", "hn_simplify_reduce", "hn_simplify_face_keys", "hn_simplify_face_net",
             "hn_simplify_face_emit", "hn_simplify_relabel"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES) and "hn_simplify.hip" in L.SOURCES
    assert HN.simplify_mesh is HN.geometry.simplify_mesh
    lib = L.load()
    # refused before any launch: NULL pointers, zero sizes, a cell side that is not positive
    import ctypes as C
    one, zero = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(0.0, 0.0, 0.0)
    assert lib.hn_simplify_extent(None, 4, None, 1, None) == -2
    assert lib.hn_simplify_keys(None, 4, zero, one, None, None) == -2
    assert lib.hn_simplify_keys(None, 0, zero, one, None, None) == -2
    assert lib.hn_simplify_reduce(None, None, None, 0, None, None, None, 0, 0, zero, one, 0.1, 1, None, None, None, None) == -2
    assert lib.hn_simplify_face_keys(None, 0, None, 0, None, None, None, None) == -2
    assert lib.hn_simplify_face_net(None, None, None, None, 0, None, None) == -2
    assert lib.hn_simplify_face_emit(None, None, None, None, None, 0, 0, 0, None, None, None) == -2
    assert lib.hn_simplify_relabel(None, 0, None, None, 0, None, None) == -2
