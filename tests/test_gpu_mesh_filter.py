"""GPU tests (MI355X) of the mesh post-processing: connected components (hn_cc_*), component sizes, filter_mesh
(hn_mesh_keep / hn_mesh_compact / hn_gather_rows), view directions (hn_vertex_viewdirs) and vertex colours, against the
NumPy statement tests/mesh_components_restated.py and tests/field_restated.py.

Tolerances.  Labels, sizes, faces and vertex_index are integers with a scheduling-free definition: identical.  Filtered
per-vertex arrays are gathers: identical bits.  A direction is a sum of three squares, a square root and a division in
fp32, each rounded once on both sides, on values of at most 1: 8 * 2^-23 allows a few half-ulp roundings.  Float colours
against the field restatement: what tests/test_gpu_geometry.py applies to query_points' rgb in fp32 mode (1e-4
element-wise); against query_points itself and across chunk sizes: identical bits."""
import functools

import numpy as np
import pytest
import torch

import field_restated as FR
import hashprng as H
import hypernerf_torch_amd as HN
import isosurface_restated as R
import mesh_components_restated as M
import test_gpu_geometry as TG
import test_isosurface_host as HT
from gpu_common import DEV, assert_close, rays_for
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import modules
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture
def fp32():
    HN.set_precision("fp32")
    yield
    HN.set_precision("bf16")


def gpu_labels(faces, v):
    """Labels, sizes and round count of the GPU for a NumPy face list; two runs must give the same bits."""
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).reshape(-1, 3).to(DEV)
    labels, rounds = F.mesh_components(f, v, return_rounds=True)
    again = HN.mesh_components(f, v)
    assert labels.dtype == torch.int32 and labels.shape == (v,) and labels.device == f.device
    assert torch.equal(labels, again), "labels differ between two runs"
    sizes = HN.component_sizes(labels, f)
    assert sizes.dtype == torch.int32 and sizes.shape == (v,) and torch.equal(sizes, HN.component_sizes(labels, f))
    assert rounds <= v + 1
    return labels.cpu().numpy(), sizes.cpu().numpy(), rounds


def check_against_restatement(faces, v, what):
    labels, sizes, rounds = gpu_labels(faces, v)
    want = M.mesh_components(faces, v)
    print(f"{what}: V {v} F {len(faces)} components {len(set(want.tolist()))} rounds {rounds}")
    assert np.array_equal(labels, want), what
    assert np.array_equal(sizes, M.component_sizes(want, faces)), what
    return rounds


@pytest.mark.parametrize("t", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_strip_labels(t):
    """Triangle strips across the wave-64 and workgroup-256 boundaries, ids ascending, descending (the minimum has to
    travel the whole chain: the worst case for the round count) and shuffled along the strip."""
    for order in ("ascending", "descending", "shuffled"):
        rounds = check_against_restatement(M.strip(t, order, seed=t), t + 2, f"strip {t} {order}")
        assert rounds <= t + 3


def test_label_edge_cases():
    both = np.concatenate([M.strip(300, "descending", stride=2), M.strip(300, "shuffled", 5, offset=1, stride=2)])
    check_against_restatement(both, 604, "two interleaved strips")
    check_against_restatement(M.strip(100, "shuffled", 7), 102 + 70, "strip + 70 unreferenced vertices")
    s = M.strip(130, "shuffled", 9)
    check_against_restatement(np.concatenate([s, s[::-1], s[:17]]), 132, "duplicated faces")
    check_against_restatement(np.array([[2, 2, 0], [5, 3, 5], [6, 6, 6]], dtype=np.int32), 8, "repeated vertices")
    empty = np.zeros((0, 3), dtype=np.int32)
    labels, sizes, rounds = gpu_labels(empty, 5)
    assert labels.tolist() == [0, 1, 2, 3, 4] and sizes.tolist() == [0] * 5 and rounds == 0
    labels, sizes, rounds = gpu_labels(empty, 0)
    assert labels.shape == (0,) and sizes.shape == (0,)


def test_out_of_range_id_is_refused_and_touches_nothing_outside():
    v = 300
    faces = M.strip(v - 2, "shuffled", 11)
    faces[123, 1] = v                                                       # one id equal to V
    f = torch.from_numpy(faces).to(DEV)
    buf = torch.full((v + 512,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="outside"):
        F.mesh_components(f, v, out=buf[256:256 + v])
    torch.cuda.synchronize()
    assert (buf[:256] == -7).all() and (buf[256 + v:] == -7).all(), "the canary around parent[] was written"
    faces[123, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        HN.mesh_components(torch.from_numpy(faces).to(DEV), v)
    mesh = {"vertices": torch.zeros(v, 3, device=DEV), "normals": torch.zeros(v, 3, device=DEV), "faces": f}
    with pytest.raises(ValueError, match="outside"):
        HN.filter_mesh(mesh, keep_largest=1)
    with pytest.raises(ValueError, match="outside"):
        HN.mesh_components(torch.zeros((2, 3), dtype=torch.int32, device=DEV), 0)


FIELDS = {      # name -> (grid, iso, bounds, components, Euler characteristic of ONE component | None for an open sheet)
    "sphere17": (lambda: HT.sphere(17), 0.0, HT.UNIT, 1, 2),
    "torus17": (lambda: HT.torus(17), 0.0, HT.UNIT, 1, 0),
    "plane_5x7x9": (lambda: HT.plane((5, 7, 9), 0.9), 0.0, HT.PLANE_BOUNDS, 1, None),
    "octahedron17": (lambda: HT.octahedron()[0], 0.0, HT.octahedron()[1], 1, 2),
    "two_spheres17": (lambda: HT.two_spheres(17), 0.0, HT.UNIT, 2, 2),
    "blobs33": (lambda: M.blobs(33), 0.0, HT.UNIT, 27, 2),
}


@functools.lru_cache(maxsize=None)
def gpu_mesh(name):
    """The GPU's own mesh of a field (with made-up colours), on the device and as NumPy, with the restatement's labels and
    sizes of that mesh: computed once, shared, never modified."""
    build, iso, bounds, _, _ = FIELDS[name]
    mesh = HN.extract_isosurface(torch.from_numpy(build()).to(DEV), iso, bounds)
    nv = mesh["vertices"].shape[0]
    mesh["colors"] = torch.from_numpy((np.arange(3 * nv) * 11 % 256).astype(np.uint8).reshape(nv, 3)).to(DEV)
    host = {k: t.cpu().numpy() for k, t in mesh.items()}
    labels = M.mesh_components(host["faces"], nv)
    return mesh, host, labels, M.component_sizes(labels, host["faces"])


def assert_filtered_equal(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (what, k)                  # bit for bit, NaN and -0 included
        assert got[k].is_contiguous() and got[k].device == torch.device(DEV)


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_components_and_filter_on_extractor_output(name):
    _, _, _, n_comp, euler = FIELDS[name]
    mesh, host, want_labels, want_sizes = gpu_mesh(name)
    nv = host["vertices"].shape[0]
    labels, sizes, rounds = gpu_labels(host["faces"], nv)
    print(f"{name}: V {nv} F {host['faces'].shape[0]} rounds {rounds}")
    assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
    assert len(set(labels.tolist())) == n_comp
    per = sorted((int(s) for s in want_sizes if s > 0), reverse=True)
    combos = [dict(keep_largest=1), dict(min_faces=1), dict(min_faces=per[0] + 1), dict(keep_largest=0)]
    if name == "blobs33":
        small, mid, big = sorted(set(per))
        assert per.count(small) == per.count(mid) == per.count(big) == 9
        # thresholds between the size classes, and cuts in the middle of a class: ties go to the smaller label
        combos += [dict(min_faces=mid), dict(min_faces=big), dict(keep_largest=11), dict(keep_largest=9),
                   dict(keep_largest=26), dict(min_faces=mid, keep_largest=4), dict(min_faces=big, keep_largest=20),
                   dict(min_faces=small, keep_largest=27), dict(keep_largest=1000)]
    for kw in combos:
        got = HN.filter_mesh(mesh, **kw)
        want = M.filter_mesh(host, **kw)
        assert_filtered_equal(got, want, f"{name} {kw}")
        assert torch.equal(HN.filter_mesh(mesh, **kw)["faces"], got["faces"])
        kept = {int(want_labels[i]) for i in want["vertex_index"]}
        c = R.check_mesh(want["vertices"], want["faces"])
        if euler is not None:             # a filtered watertight mesh stays watertight; chi adds up over the components
            assert c["closed"] and c["oriented"] and c["euler"] == euler * len(kept), (name, kw, c, len(kept))
        if want["faces"].shape[0]:
            assert np.unique(want["faces"]).size == want["vertices"].shape[0]
    assert HN.filter_mesh(mesh) is mesh
    # filtering a filtered mesh: vertex_index then names the vertices of the mesh that went in
    if n_comp > 1:
        twice = HN.filter_mesh(HN.filter_mesh(mesh, keep_largest=n_comp - 1), keep_largest=1)
        assert_filtered_equal(twice, M.filter_mesh(M.filter_mesh(host, keep_largest=n_comp - 1), keep_largest=1), name)


def test_filter_mesh_empty_and_loose_vertices():
    empty = HN.extract_isosurface(torch.zeros((5, 6, 7), device=DEV), 0.5, HT.UNIT)
    out = HN.filter_mesh(empty, keep_largest=1)
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and out["vertex_index"].shape == (0,)
    assert out["vertex_index"].dtype == torch.int32 and out["faces"].dtype == torch.int32
    # a strip with 70 loose vertices in front: they go, and the ids shift by 70
    faces = M.strip(50, "shuffled", 3, offset=70)
    v = torch.from_numpy(H.uniform(3, "loose", (122, 3), -1.0, 1.0).numpy()).to(DEV)
    mesh = {"vertices": v, "normals": -v, "faces": torch.from_numpy(faces).to(DEV)}
    out = HN.filter_mesh(mesh, min_faces=1)
    assert out["vertex_index"].tolist() == list(range(70, 122)) and torch.equal(out["vertices"], v[70:])
    assert np.array_equal(out["faces"].cpu().numpy(), faces - 70)
    none = HN.filter_mesh(mesh, min_faces=51)
    assert none["vertices"].shape == (0, 3) and none["normals"].shape == (0, 3) and none["faces"].shape == (0, 3)


def test_vertex_viewdirs_vs_float32_restatement():
    n = 200
    cam = (0.25, -0.5, 0.125)
    v = H.uniform(17, "vd_v", (n, 3), -1.0, 1.0).numpy().astype(np.float32)
    nrm = H.uniform(17, "vd_n", (n, 3), -1.0, 1.0).numpy().astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[3] = 0.0
    nrm[64] = 0.0
    nrm[n - 1] = (0.0, -0.0, 0.0)
    nrm[5] *= np.float32(1e-3)                                               # not unit: normalised all the same
    v[7] = cam
    v[63] = np.float32(cam) + np.float32([1e-6, 0.0, 0.0])
    v[65] = np.float32(cam) + np.float32([0.0, -1e3, 1e3])
    v[n - 1] = cam
    vd, nd = torch.from_numpy(v).to(DEV), torch.from_numpy(nrm).to(DEV)
    tol = 8.0 * 2.0 ** -23
    worst = 0.0
    for camera in (None, cam):
        for start, count in ((0, 1), (0, 63), (0, 64), (1, 65), (0, n), (n - 3, 10), (n - 1, 64)):   # the last two pad
            got = F.vertex_viewdirs(vd, nd, start, count, camera)
            assert got.shape == (count, 3) and got.dtype == torch.float32
            got = got.cpu().numpy()
            want = M.vertex_viewdirs(v, nrm, start, count, camera)
            worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
            fallback = (want == np.float32([0, 0, 1])).all(axis=1)
            assert np.array_equal(got[fallback], want[fallback])
            assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    print(f"vertex_viewdirs: max abs error {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol
    head_on = F.vertex_viewdirs(vd, nd, 0, n, None).cpu().numpy()
    assert all(np.array_equal(head_on[i], [0, 0, 1]) for i in (3, 64, n - 1))
    seen = F.vertex_viewdirs(vd, nd, 0, n, cam).cpu().numpy()
    assert all(np.array_equal(seen[i], [0, 0, 1]) for i in (7, n - 1))
    assert np.array_equal(seen[63], [1, 0, 0])
    with pytest.raises(ValueError):
        F.vertex_viewdirs(vd, nd, n, 4, None)


def no_viewdirs_model(seed):
    """The "nowarp" model of test_gpu_geometry with use_viewdirs=False: its colour branch is built without view channels."""
    kw, warp_kind, _ = TG.QUERY_CASES["nowarp"]
    m, _ = TG.small_model(kw, warp_kind, seed)
    m.use_viewdirs = False
    for name in ("nerf_mlps_coarse", "nerf_mlps_fine"):
        old = getattr(m, name)
        setattr(m, name, modules.NerfMLP(
            in_ch=old.in_ch, trunk_depth=old.trunk_depth, trunk_width=old.trunk_width,
            rgb_branch_depth=old.rgb_branch_depth, rgb_branch_width=old.rgb_branch_width, rgb_channels=old.rgb_channels,
            alpha_channels=old.alpha_channels, skips=old.skips, hidden_activation=old.hidden_activation,
            rgb_activation=old.rgb_activation, alpha_condition_dim=old.alpha_condition_dim, rgb_condition_dim=0,
            norm=old.norm))
    sd = H.fill_state_dict({k: tuple(t.shape) for k, t in m.state_dict().items()}, seed)
    m.load_state_dict(sd)
    return m.to(DEV), sd


COLOUR_CASES = ["bendy_fused", "se3_axis", "no_viewdirs"]


@pytest.mark.parametrize("case", COLOUR_CASES)
def test_vertex_colors(case, fp32):
    seed, n, frame = 163, 9, 23
    if case == "no_viewdirs":
        m, sd = no_viewdirs_model(seed)
    else:
        kw, warp_kind, _ = TG.QUERY_CASES[case]
        m, sd = TG.small_model(kw, warp_kind, seed)
    v = H.uniform(seed, "vc_v", (n, 3), -0.9, 0.9)
    nrm = H.uniform(seed, "vc_n", (n, 3), -1.0, 1.0)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    nrm[4] = 0.0                                                             # looks along (0, 0, 1)
    cam = (0.3, -1.7, 0.6)
    vd, nd = v.to(DEV), nrm.to(DEV)
    ids = torch.full((n,), frame, dtype=torch.int64)
    meta = {k: ids.to(DEV) for k in ("warp", "camera", "appearance", "time")}
    floats = {}
    for view in ("normal", cam):
        camera = None if view == "normal" else cam
        rgb = HN.vertex_colors(m, vd, nd, frame, view=view, dtype=torch.float32)
        assert rgb.shape == (n, 3) and rgb.dtype == torch.float32 and rgb.device == vd.device
        assert getattr(m, "_level_state", None) is None
        # the plumbing: query_points on the same points and directions, bit for bit
        dirs = F.vertex_viewdirs(vd, nd, 0, n, camera)
        direct = m.query_points(vd.view(n, 1, 3), meta, level="fine", viewdirs=dirs)["rgb"].view(n, 3)
        assert torch.equal(rgb, direct), (case, view)
        # the directions arrive where the view encoder reads them: the field restated on the CPU
        want_dirs = torch.from_numpy(M.vertex_viewdirs(v.numpy(), nrm.numpy(), 0, n, camera))
        with torch.no_grad():
            if case == "no_viewdirs":
                cfg = O.ModelCfg(n_samples_coarse=8, n_samples_fine=8, **TG.QUERY_CASES["nowarp"][0])
                ref = O.nerf_mlp(sd, "nerf_mlps_fine", O.posenc_orig(v.view(n, 1, 3), cfg.xyz_f), None, None)[0].view(n, 3)
            else:
                kw, warp_kind, _ = TG.QUERY_CASES[case]
                cfg = O.ModelCfg(n_samples_coarse=8, n_samples_fine=8, warp_kind=warp_kind, **kw)
                ref = FR.query_points(sd, cfg, "fine", v.view(n, 1, 3), want_dirs, ids)["rgb"].view(n, 3)
        assert_close(rgb, ref, 1e-4, f"vertex_colors {case} {view if view == 'normal' else 'camera'}")
        # uint8: the truncation of the GPU's own floats exactly, within one level of the restatement's
        u8 = HN.vertex_colors(m, vd, nd, frame, view=view)
        assert u8.dtype == torch.uint8 and torch.equal(u8, (rgb * 255).to(torch.uint8))
        assert int((u8.cpu().int() - (ref * 255).to(torch.uint8).int()).abs().max()) <= 1
        for chunk in (1, 7):
            assert torch.equal(HN.vertex_colors(m, vd, nd, frame, view=view, chunk=chunk, dtype=torch.float32), rgb), chunk
            assert torch.equal(HN.vertex_colors(m, vd, nd, frame, view=view, chunk=chunk), u8), chunk
        floats[view] = rgb
    other = HN.vertex_colors(m, vd, nd, frame + 1, view=cam, dtype=torch.float32)
    coarse = HN.vertex_colors(m, vd, nd, frame, view=cam, level="coarse", dtype=torch.float32)
    assert not torch.equal(coarse, floats[cam])
    if case == "no_viewdirs":
        assert torch.equal(floats["normal"], floats[cam])                   # the direction is ignored
    else:
        assert not torch.equal(floats["normal"], floats[cam])               # ... and otherwise it matters
        assert not torch.equal(other, floats[cam])                          # another frame, another colour
    as_tensor = HN.vertex_colors(m, vd, nd, frame, view=torch.tensor(cam), dtype=torch.float32)
    assert torch.equal(as_tensor, floats[cam])
    assert HN.vertex_colors(m, vd[:0], nd[:0], frame).shape == (0, 3)


def test_extract_mesh_defaults_return_todays_mesh(fp32):
    kw, warp_kind, _ = TG.QUERY_CASES["bendy_fused"]
    m, _ = TG.small_model(kw, warp_kind, 149)
    bounds, res, frame = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), (9, 8, 10), 3
    grid = HN.density_grid(m, bounds, res, frame, chunk=256)
    iso = float(grid.median())
    ref = HN.extract_isosurface(grid, iso, bounds)
    mesh = HN.extract_mesh(m, bounds, res, frame, iso=iso, chunk=256)
    assert sorted(mesh) == ["faces", "normals", "vertices"]
    for k in ("vertices", "normals", "faces"):
        assert torch.equal(mesh[k], ref[k]) and mesh[k].dtype == ref[k].dtype, k


def test_extract_mesh_filters_then_colours(fp32, tmp_path):
    kw, warp_kind, _ = TG.QUERY_CASES["bendy_fused"]
    m, _ = TG.small_model(kw, warp_kind, 149)
    bounds, res, frame = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0), (9, 8, 10), 3
    grid = HN.density_grid(m, bounds, res, frame, chunk=256)
    iso = float(grid.median())
    ref = HN.extract_isosurface(grid, iso, bounds)
    for colors, filt in (("normal", dict(keep_largest=1)), ((0.1, 0.2, -2.5), dict(min_faces=3)), ("normal", {})):
        mesh = HN.extract_mesh(m, bounds, res, frame, iso=iso, colors=colors, chunk=256, **filt)
        want = HN.filter_mesh(ref, **filt)
        assert sorted(mesh) == sorted(list(want) + ["colors"])
        for k in want:
            assert torch.equal(mesh[k], want[k]), k
        host = M.filter_mesh({k: t.cpu().numpy() for k, t in ref.items()}, **filt)
        assert np.array_equal(mesh["faces"].cpu().numpy(), host["faces"]) and mesh["faces"].shape[0] > 0
        assert mesh["colors"].dtype == torch.uint8 and mesh["colors"].shape == mesh["vertices"].shape
        assert torch.equal(mesh["colors"], HN.vertex_colors(m, want["vertices"], want["normals"], frame, view=colors))
        assert float(mesh["colors"].float().std()) > 0
    path = str(tmp_path / "mesh.ply")
    HN.write_ply(path, mesh["vertices"], mesh["faces"], mesh["normals"], mesh["colors"])
    back = HN.read_ply(path)
    for k in ("vertices", "normals", "faces", "colors"):
        assert np.array_equal(back[k], mesh[k].cpu().numpy()), k


@pytest.mark.parametrize("case", ["bendy_fused", "se3_axis"])
def test_forward_is_undisturbed_by_vertex_colors(case, fp32):
    """Same model, same rays, same draws: forward before and after vertex_colors gives the same bits."""
    kw, warp_kind, _ = TG.QUERY_CASES[case]
    seed, b, nc, nf = 167, 12, 8, 8
    m, _ = TG.small_model(kw, warp_kind, seed, nc, nf)
    o, d, idx = rays_for(seed, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1).to(DEV), "u": H.uniform(seed, "u", (b, nf), 0, 1).to(DEV),
           "noise_coarse": (H.normal(seed, "n1", (b, nc, 1)) * 0.7).to(DEV),
           "noise_fine": (H.normal(seed, "n2", (b, nc + nf, 1)) * 0.7).to(DEV)}
    before = m(rays, {}, rng=rng)
    state = getattr(m, "_level_state", None)
    v = H.uniform(seed, "vc_v", (11, 3), -0.9, 0.9).to(DEV)
    for level in ("coarse", "fine"):
        HN.vertex_colors(m, v, -v, 5, level=level, chunk=4)
        HN.vertex_colors(m, v, None, 5, view=(0.0, 0.0, 3.0), level=level, render_opts={"dust_threshold": 0.1})
    assert getattr(m, "_level_state", None) is state
    after = m(rays, {}, rng=rng)
    for lvl in ("coarse", "fine"):
        for k in ("points", "warped_points", "rgb", "depth", "med_depth", "acc", "weights", "med_points"):
            assert torch.equal(before[lvl][k], after[lvl][k]), f"{case} {lvl}/{k}"
