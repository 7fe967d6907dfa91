"""GPU tests of mesh simplification by vertex clustering (csrc/hn_simplify.hip, geometry.simplify_mesh) against the NumPy
float32 restatement (tests/simplify_restated.py), on fp32 meshes that extract_isosurface made on the GPU from analytic
grids.  Every comparison is for identical arrays: integers (keys, vertex_cluster, faces) as they are, floats (positions,
normals, fp32 colours) by their bits — the library is built with contraction off, every operation of the definition is
one correctly rounded fp32 operation, and the summation order is part of the definition."""
import functools
import os

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import isosurface_restated as R
import mesh_components_restated as MC
import simplify_restated as S
import test_isosurface_host as HT
from gpu_common import DEV
from hypernerf_torch_amd import functional as F

pytestmark = pytest.mark.gpu

ORIGIN = (-1.0, -1.0, -1.0)
GRIDS = {"sphere9": (HT.sphere, 9), "sphere17": (HT.sphere, 17), "two_spheres25": (HT.two_spheres, 25), "torus33": (HT.torus, 33)}
CASES = [("sphere9", 0.25), ("sphere9", 1), ("sphere9", 3), ("sphere17", 3), ("two_spheres25", 2), ("torus33", 2)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = bits(got) == bits(want)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} entries differ, first at {np.argwhere(~same)[0].tolist()}"


def to_gpu(mesh):
    return {k: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for k, a in mesh.items()}


def to_host(mesh):
    return {k: t.cpu().numpy() for k, t in mesh.items()}


@functools.lru_cache(maxsize=None)
def gpu_mesh(name):
    """(the GPU's isosurface as tensors, the same arrays on the host, the lattice spacing)."""
    build, n = GRIDS[name]
    mesh = HN.extract_isosurface(torch.from_numpy(build(n)).to(DEV), 0.0, HT.UNIT)
    assert mesh["faces"].shape[0] > 0
    return mesh, to_host(mesh), 2.0 / (n - 1)


def with_colors(mesh, host, dtype):
    if dtype is None:
        return dict(mesh), dict(host)
    c = S.hashed_colors(host["vertices"].shape[0], dtype)
    return dict(mesh, colors=torch.from_numpy(c).to(DEV)), dict(host, colors=c)


def assert_mesh_same(out, ref, what):
    assert set(out) == set(ref), (what, sorted(out), sorted(ref))
    for k in sorted(ref):
        assert out[k].is_cuda and out[k].is_contiguous()
        assert_same(out[k], ref[k], f"{what}: {k}")


@pytest.mark.parametrize("colors", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("name,k", CASES)
def test_simplify_matches_the_restatement(name, k, placement, colors):
    mesh, host, spacing = gpu_mesh(name)
    mesh, host = with_colors(mesh, host, colors)
    cell = k * spacing
    ref = S.simplify_mesh(host, cell, ORIGIN, placement)
    out = HN.simplify_mesh(mesh, cell, ORIGIN, placement)
    print(f"{name} k={k} {placement}: V {host['vertices'].shape[0]} -> {ref['vertices'].shape[0]}, "
          f"F {host['faces'].shape[0]} -> {ref['faces'].shape[0]}")
    assert ref["faces"].shape[0] > 0
    assert_mesh_same(out, ref, f"{name} k={k} {placement}")
    assert S.edge_balance(out["faces"].cpu().numpy())
    if name == "torus33":
        assert host["vertices"].shape[0] == 5768


@pytest.mark.parametrize("name,k", CASES)
def test_stages_match_the_restatement(name, k):
    """cluster_vertices, reduce_clusters (EVERY cluster, the ones that lose their faces included) and cluster_faces."""
    mesh, host, spacing = gpu_mesh(name)
    mesh, host = with_colors(mesh, host, np.float32)
    cell = k * spacing
    ref = S.cluster_vertices(host["vertices"], cell, ORIGIN)
    got = F.cluster_vertices(mesh["vertices"], cell, ORIGIN)
    for key in ("keys", "cluster_keys", "vertex_cluster", "order", "starts"):
        assert_same(got[key], ref[key], f"{name} k={k}: {key}")
    for placement in ("quadric", "mean"):
        want = S.reduce_clusters(host["vertices"], host["normals"], host["colors"], ref, cell, ORIGIN, placement)
        rep = F.reduce_clusters(mesh["vertices"], mesh["normals"], mesh["colors"], got, cell, ORIGIN, placement)
        assert_mesh_same(rep, want, f"{name} k={k} {placement} (all clusters)")
    faces, used = F.cluster_faces(mesh["faces"], got["vertex_cluster"], ref["cluster_keys"].size, return_used=True)
    want = S.cluster_faces(host["faces"], ref["vertex_cluster"])
    assert_same(faces, want, f"{name} k={k}: cluster faces")
    mark = np.zeros(ref["cluster_keys"].size, dtype=np.int32)
    mark[want.reshape(-1)] = 1
    assert_same(used, mark, f"{name} k={k}: used clusters")
    if (name, k) in (("sphere9", 3), ("sphere17", 3)):
        assert int((mark == 0).sum()) == 1


def line_strip(t):
    """A strip of t triangles over t + 2 vertices laid along x with unit spacing (y, z inside [0, 0.5))."""
    n = t + 2
    v = S.hashed_colors(n, np.float32, 11) * np.float32(0.5)
    v[:, 0] = np.arange(n, dtype=np.float32)
    return {"vertices": v.astype(np.float32), "faces": MC.strip(t), "normals": S.hashed_normals(n, 5),
            "colors": S.hashed_colors(n, np.uint8 if t % 2 else np.float32, 9)}


@pytest.mark.parametrize("t", [1, 62, 63, 64, 254, 255, 256, 4099])
def test_kernel_boundaries_on_strips(t):
    """A cell of 1 gives t + 2 singleton clusters (launch sizes around the wave and the workgroup), a cell of t + 3 one
    cluster of t + 2 members (the sequential walk).  Through reduce_clusters: the one-cluster mesh has no face left."""
    host = line_strip(t)
    mesh = to_gpu(host)
    for cell, n_clusters in ((1.0, t + 2), (float(t + 3), 1)):
        ref = S.cluster_vertices(host["vertices"], cell, 0.0)
        got = F.cluster_vertices(mesh["vertices"], cell, 0.0)
        assert ref["cluster_keys"].size == n_clusters
        for key in ("keys", "cluster_keys", "vertex_cluster", "order", "starts"):
            assert_same(got[key], ref[key], f"t={t} cell={cell}: {key}")
        for placement in ("quadric", "mean"):
            want = S.reduce_clusters(host["vertices"], host["normals"], host["colors"], ref, cell, 0.0, placement)
            rep = F.reduce_clusters(mesh["vertices"], mesh["normals"], mesh["colors"], got, cell, 0.0, placement)
            assert_mesh_same(rep, want, f"t={t} cell={cell} {placement}")
        assert_same(F.cluster_faces(mesh["faces"], got["vertex_cluster"], n_clusters),
                    S.cluster_faces(host["faces"], ref["vertex_cluster"]), f"t={t} cell={cell}: faces")
    out = HN.simplify_mesh(mesh, float(t + 3), (0.0, 0.0, 0.0))
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and bool((out["vertex_cluster"] == -1).all())
    assert_mesh_same(HN.simplify_mesh(mesh, 1.0, (0.0, 0.0, 0.0)), S.simplify_mesh(host, 1.0, (0.0, 0.0, 0.0)), f"t={t}")


@pytest.mark.parametrize("n", [1, 63, 65, 2047, 2048, 2049, 3 * 2048 + 5])
def test_vertex_extent(n):
    """The extent read that guards the key layout: sizes around the wave and the 2048-vertex tile; NaN and inf are seen."""
    v = (S.hashed_colors(n, np.float32, 21) * np.float32(6.0) - np.float32(3.0)).astype(np.float32)
    lo, hi = F.vertex_extent(torch.from_numpy(v).to(DEV))
    assert_same(np.asarray(lo, dtype=np.float32), v.min(axis=0), f"n={n}: minimum")
    assert_same(np.asarray(hi, dtype=np.float32), v.max(axis=0), f"n={n}: maximum")
    faces = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    for bad in (float("nan"), float("inf"), float("-inf")):
        w = v.copy()
        w[n - 1, 1] = bad
        lo, hi = F.vertex_extent(torch.from_numpy(w).to(DEV))
        assert not np.isfinite(np.asarray(lo + hi)).all()
        with pytest.raises(ValueError, match="finite"):
            HN.simplify_mesh({"vertices": torch.from_numpy(w).to(DEV), "faces": faces}, 1.0, placement="mean")


def test_keys_past_32_bits():
    mesh, host, _ = gpu_mesh("sphere9")
    cell = 2.0 / (2 ** 21 - 1)
    ref_clusters = S.cluster_vertices(host["vertices"], cell, ORIGIN)
    got = F.cluster_vertices(mesh["vertices"], cell, ORIGIN)
    assert int(ref_clusters["keys"].max()) > 2 ** 42 and int(ref_clusters["keys"].min()) > 2 ** 32
    for key in ("keys", "cluster_keys", "vertex_cluster", "order", "starts"):
        assert_same(got[key], ref_clusters[key], key)
    for placement in ("quadric", "mean"):
        assert_mesh_same(HN.simplify_mesh(mesh, cell, ORIGIN, placement), S.simplify_mesh(host, cell, ORIGIN, placement), placement)
    v = host["vertices"].shape[0]
    assert ref_clusters["cluster_keys"].size == v, "the restatement gives one cluster per vertex here"
    # one cluster per vertex: the output is the input under the permutation by key
    out = to_host(HN.simplify_mesh(mesh, cell, ORIGIN, "mean"))
    vc = out["vertex_cluster"]
    assert np.array_equal(np.sort(vc), np.arange(v))
    assert np.array_equal(out["vertices"][vc], host["vertices"] + np.float32(0))
    assert np.abs(out["normals"][vc] - host["normals"]).max() <= 2.0 ** -22
    canon = lambda f: np.unique(np.stack([np.roll(r, -int(np.argmin(r))) for r in f]), axis=0)      # rows, sorted
    assert out["faces"].shape == host["faces"].shape and np.array_equal(canon(out["faces"]), canon(vc[host["faces"]]))


def test_hand_made_mesh():
    host, cell, origin, expect = S.hand_made()
    mesh = to_gpu(host)
    for placement in ("mean", "quadric"):
        out = HN.simplify_mesh(mesh, cell, origin, placement)
        assert_same(out["faces"], expect["faces"], "faces")
        assert_same(out["vertex_cluster"], expect["vertex_cluster"], "vertex_cluster")
        assert_mesh_same(out, S.simplify_mesh(host, cell, origin, placement), placement)
    # origin None = the minimum of the vertices; no normals: placement 'mean' only
    bare = {k: mesh[k] for k in ("vertices", "faces")}
    out = HN.simplify_mesh(bare, cell, None, "mean")
    assert_mesh_same(out, S.simplify_mesh({k: host[k] for k in ("vertices", "faces")}, cell, None, "mean"), "origin None")
    with pytest.raises(ValueError, match="normals"):
        HN.simplify_mesh(bare, cell)


def test_two_runs_give_equal_bits_and_other_keys_are_dropped():
    mesh, host, spacing = gpu_mesh("torus33")
    mesh, _ = with_colors(mesh, host, np.uint8)
    mesh["vertex_index"] = torch.arange(host["vertices"].shape[0], dtype=torch.int32, device=DEV)
    a = HN.simplify_mesh(mesh, 2 * spacing, ORIGIN)
    b = HN.simplify_mesh(mesh, 2 * spacing, ORIGIN)
    assert sorted(a) == ["colors", "faces", "normals", "vertex_cluster", "vertices"]
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr(), k
    assert torch.equal(a["vertices"].view(torch.int32), b["vertices"].view(torch.int32))


def test_empty_input_and_total_collapse():
    empty = {"vertices": torch.zeros((0, 3), device=DEV), "normals": torch.zeros((0, 3), device=DEV),
             "faces": torch.zeros((0, 3), dtype=torch.int32, device=DEV), "colors": torch.zeros((0, 3), dtype=torch.uint8, device=DEV)}
    out = HN.simplify_mesh(empty, 0.5)
    assert out["vertices"].shape == (0, 3) and out["normals"].shape == (0, 3) and out["faces"].shape == (0, 3)
    assert out["colors"].shape == (0, 3) and out["colors"].dtype == torch.uint8 and out["vertex_cluster"].shape == (0,)
    assert out["faces"].dtype == torch.int32 and out["vertex_cluster"].dtype == torch.int32 and out["vertices"].is_cuda
    mesh, host, spacing = gpu_mesh("sphere9")
    out = HN.simplify_mesh(mesh, 40 * spacing, ORIGIN)
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and out["normals"].shape == (0, 3)
    assert out["vertex_cluster"].shape == (host["vertices"].shape[0],) and bool((out["vertex_cluster"] == -1).all())
    no_faces = dict(mesh, faces=torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert HN.simplify_mesh(no_faces, spacing, ORIGIN)["vertices"].shape == (0, 3)


def test_filter_then_simplify_then_ply(tmp_path):
    mesh, host, spacing = gpu_mesh("two_spheres25")
    kept = HN.filter_mesh(mesh, keep_largest=1)
    assert "vertex_index" in kept and 0 < kept["faces"].shape[0] < mesh["faces"].shape[0]
    kept["colors"] = torch.from_numpy(S.hashed_colors(kept["vertices"].shape[0], np.uint8)).to(DEV)
    out = HN.simplify_mesh(kept, 2 * spacing, ORIGIN)
    assert "vertex_index" not in out
    assert_mesh_same(out, S.simplify_mesh({k: v for k, v in to_host(kept).items() if k != "vertex_index"}, 2 * spacing, ORIGIN), "kept")
    c = R.check_mesh(out["vertices"].cpu().numpy(), out["faces"].cpu().numpy())
    assert c["closed"] and c["oriented"] and c["euler"] == 2, c
    path = os.path.join(tmp_path, "simplified.ply")
    HN.write_ply(path, out["vertices"], out["faces"], out["normals"], out["colors"])
    back = HN.read_ply(path)
    for k in ("vertices", "normals", "faces", "colors"):
        assert np.array_equal(bits(back[k]), bits(out[k].cpu().numpy())), k


def test_extract_mesh_with_simplify_is_the_composition():
    import test_gpu_geometry as TG
    HN.set_precision("fp32")
    kw, warp_kind, _ = TG.QUERY_CASES["bendy_fused"]
    m, _ = TG.small_model(kw, warp_kind, 149)
    bounds, res, frame = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), (9, 8, 10), 3
    grid = HN.density_grid(m, bounds, res, frame, chunk=256)
    iso = float(grid.median())
    fine = HN.extract_isosurface(grid, iso, bounds)
    assert fine["faces"].shape[0] > 0
    # without the keyword: what it returned before there was one
    for plain in (HN.extract_mesh(m, bounds, res, frame, iso=iso, chunk=256),
                  HN.extract_mesh(m, bounds, res, frame, iso=iso, chunk=256, simplify=None)):
        assert sorted(plain) == ["faces", "normals", "vertices"]
        for k in plain:
            assert torch.equal(plain[k], fine[k]), k
    # with it: extract, filter, simplify, colours along the new normals
    for factor, cell in ((2, [2 * 2.0 / 8, 2 * 2.0 / 7, 2 * 2.0 / 9]), ((1, 2, 1.5), [2.0 / 8, 2 * 2.0 / 7, 1.5 * 2.0 / 9])):
        mesh = HN.extract_mesh(m, bounds, res, frame, iso=iso, chunk=256, keep_largest=1, colors="normal", simplify=factor)
        hand = HN.simplify_mesh(HN.filter_mesh(fine, keep_largest=1), cell, origin=(-1.0, -1.0, -1.0))
        hand["colors"] = HN.vertex_colors(m, hand["vertices"], hand["normals"], frame, chunk=256)
        print(f"simplify={factor}: V {fine['vertices'].shape[0]} -> {mesh['vertices'].shape[0]}, "
              f"F {fine['faces'].shape[0]} -> {mesh['faces'].shape[0]}")
        assert sorted(mesh) == sorted(hand) == ["colors", "faces", "normals", "vertex_cluster", "vertices"]
        for k in hand:
            assert torch.equal(mesh[k], hand[k]), k
        assert mesh["colors"].dtype == torch.uint8 and mesh["colors"].shape == mesh["vertices"].shape
