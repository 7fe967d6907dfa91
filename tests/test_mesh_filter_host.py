"""CPU tests of the mesh post-processing: the NumPy restatement (tests/mesh_components_restated.py) against cases worked
out by hand, the coloured PLY layout and the byte-identity of colourless files, and the argument checks that run before
any kernel (Python entry points and the C ABI of csrc/hn_geometry.hip)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import isosurface_restated as R
import mesh_components_restated as M
import test_isosurface_host as HT
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import geometry as G

# three components and a loose vertex, by hand:
#   A = {0, 1, 2, 4}  faces (0,1,2) (2,1,4)       label 0, 2 faces
#   B = {3, 5, 7}     face  (7,5,3)               label 3, 1 face
#   C = {6, 8, 10}    faces (10,8,6) (6,8,10)     label 6, 2 faces (a duplicated face, reversed)
#   vertex 9 is referenced by nobody              label 9, 0 faces
HAND_FACES = np.array([[0, 1, 2], [7, 5, 3], [10, 8, 6], [2, 1, 4], [6, 8, 10]], dtype=np.int32)
HAND_LABELS = [0, 0, 0, 3, 0, 3, 6, 3, 6, 9, 6]
HAND_SIZES = [2, 0, 0, 1, 0, 0, 2, 0, 0, 0, 0]


def hand_mesh():
    v = np.arange(33, dtype=np.float32).reshape(11, 3)
    return {"vertices": v, "normals": -v, "faces": HAND_FACES.copy(), "colors": (np.arange(33) % 251).astype(np.uint8).reshape(11, 3)}


def test_labels_and_sizes_by_hand():
    labels = M.mesh_components(HAND_FACES, 11)
    assert labels.dtype == np.int32 and labels.tolist() == HAND_LABELS
    assert M.component_sizes(labels, HAND_FACES).tolist() == HAND_SIZES
    # a face with a repeated vertex connects the two it names; no face, no connection
    assert M.mesh_components(np.array([[2, 2, 0]]), 4).tolist() == [0, 1, 0, 3]
    assert M.mesh_components(np.zeros((0, 3), np.int32), 5).tolist() == [0, 1, 2, 3, 4]
    assert M.mesh_components(np.zeros((0, 3), np.int32), 0).shape == (0,)
    with pytest.raises(ValueError):
        M.mesh_components(np.array([[0, 1, 4]]), 4)
    for t in (1, 2, 65):
        for order in ("ascending", "descending", "shuffled"):
            assert (M.mesh_components(M.strip(t, order, seed=t), t + 2) == 0).all(), (t, order)
    # two interleaved strips: even ids and odd ids
    both = np.concatenate([M.strip(5, "descending", stride=2), M.strip(5, "shuffled", 3, offset=1, stride=2)])
    assert M.mesh_components(both, 14).tolist() == [0, 1] * 7


def test_filter_rules_by_hand():
    mesh = hand_mesh()
    assert M.filter_mesh(mesh) is mesh
    # keep_largest=1: A and C tie at two faces, the smaller label (A) wins
    one = M.filter_mesh(mesh, keep_largest=1)
    assert one["vertex_index"].tolist() == [0, 1, 2, 4] and one["vertex_index"].dtype == np.int32
    assert one["faces"].tolist() == [[0, 1, 2], [2, 1, 3]] and one["faces"].dtype == np.int32
    for k in ("vertices", "normals", "colors"):
        assert np.array_equal(one[k], mesh[k][[0, 1, 2, 4]]) and one[k].dtype == mesh[k].dtype
    # keep_largest=2: A and C; faces keep their order and are re-indexed: 6 -> 4, 8 -> 5, 10 -> 6
    two = M.filter_mesh(mesh, keep_largest=2)
    assert two["vertex_index"].tolist() == [0, 1, 2, 4, 6, 8, 10]
    assert two["faces"].tolist() == [[0, 1, 2], [6, 5, 4], [2, 1, 3], [4, 5, 6]]
    # min_faces alone; the loose vertex 9 goes as soon as any filter is active
    assert M.filter_mesh(mesh, min_faces=2)["vertex_index"].tolist() == [0, 1, 2, 4, 6, 8, 10]
    assert M.filter_mesh(mesh, min_faces=0)["vertex_index"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert M.filter_mesh(mesh, keep_largest=99)["vertex_index"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    # both: at least one face AND among the three largest = everything but 9; min_faces=2 AND the 3 largest = A, C
    assert M.filter_mesh(mesh, min_faces=2, keep_largest=3)["vertex_index"].tolist() == [0, 1, 2, 4, 6, 8, 10]
    # keep_largest=1 picks A; min_faces=3 then leaves nothing: B is NOT promoted into the gap
    none = M.filter_mesh(mesh, min_faces=3, keep_largest=1)
    assert none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3) and none["vertex_index"].shape == (0,)
    assert none["colors"].shape == (0, 3) and none["colors"].dtype == np.uint8
    assert M.filter_mesh(mesh, keep_largest=0)["faces"].shape == (0, 3)


def test_filtered_restated_sphere_stays_watertight():
    m = R.extract_isosurface(HT.two_spheres(17), 0.0, HT.UNIT)
    labels = M.mesh_components(m["faces"], m["vertices"].shape[0])
    assert len(set(labels.tolist())) == 2
    one = M.filter_mesh(m, keep_largest=1)
    c = R.check_mesh(one["vertices"], one["faces"])
    assert c["closed"] and c["oriented"] and c["euler"] == 2 and c["volume"] > 0
    assert np.array_equal(one["vertices"], m["vertices"][one["vertex_index"]])


def test_blobs_field_has_27_components_in_three_size_classes():
    f = M.blobs()
    m = R.extract_isosurface(f, 0.0, HT.UNIT)
    labels = M.mesh_components(m["faces"], m["vertices"].shape[0])
    sizes = M.component_sizes(labels, m["faces"])
    per = sorted(int(s) for s in sizes if s > 0)
    assert len(per) == 27 and len(set(per)) == 3 and all(per.count(s) == 9 for s in set(per)), per
    small, mid, big = sorted(set(per))
    assert len(M.kept_components(labels, sizes, min_faces=mid)) == 18
    # ties between equal blobs: keep_largest=11 takes the 9 big ones and the two mid ones with the smallest labels
    kept = M.kept_components(labels, sizes, keep_largest=11)
    mids = sorted(l for l in set(labels.tolist()) if sizes[l] == mid)
    assert sorted(kept) == sorted([l for l in set(labels.tolist()) if sizes[l] == big] + mids[:2])


def test_viewdirs_restated():
    v = np.float32([[1, 2, 3], [0.5, 0.5, 0.5], [0, 0, 2]])
    n = np.float32([[0, 0, -2], [0, 0, 0], [3, 0, 4]])
    d = M.vertex_viewdirs(v, n, 0, 3)
    assert d.dtype == np.float32 and np.array_equal(d, np.float32([[0, 0, 1], [0, 0, 1], [-0.6, 0, -0.8]]))
    d = M.vertex_viewdirs(v, n, 1, 4, camera=(0.5, 0.5, 0.5))          # v == c, then (0,0,2) - c, then padding
    want = np.float32([-0.5, -0.5, 1.5]) / np.sqrt(np.float32(2.75))
    assert np.array_equal(d[0], [0, 0, 1]) and np.allclose(d[1], want, atol=1e-7) and (d[2:] == d[1]).all()


def test_ply_colours_round_trip_and_colourless_bytes(tmp_path):
    m = R.extract_isosurface(HT.sphere(9), 0.0, HT.UNIT)
    nv, nf = m["vertices"].shape[0], m["faces"].shape[0]
    colors = (np.arange(3 * nv) * 7 % 256).astype(np.uint8).reshape(nv, 3)
    path = os.path.join(tmp_path, "c.ply")
    for normals in (m["normals"], None):
        G.write_ply(path, torch.from_numpy(m["vertices"]), m["faces"], normals, torch.from_numpy(colors))
        blob = open(path, "rb").read()
        head, body = blob.split(b"end_header\n", 1)
        names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
        assert head.decode("ascii").split("\n")[:-1] == (
            ["ply", "format binary_little_endian 1.0", f"element vertex {nv}"] + [f"property float {n}" for n in names]
            + ["property uchar red", "property uchar green", "property uchar blue", f"element face {nf}",
               "property list uchar int vertex_indices"])
        width = len(names)
        assert len(body) == nv * (4 * width + 3) + 13 * nf
        # record 5, decoded by hand
        rec = body[5 * (4 * width + 3):6 * (4 * width + 3)]
        floats = struct.unpack("<" + "f" * width, rec[:4 * width])
        assert floats[:3] == tuple(m["vertices"][5].tolist()) and tuple(rec[4 * width:]) == tuple(colors[5].tolist())
        back = HN.read_ply(path)
        assert np.array_equal(back["colors"], colors) and back["colors"].dtype == np.uint8
        assert np.array_equal(back["vertices"], m["vertices"]) and np.array_equal(back["faces"], m["faces"])
        assert (back["normals"] is None) if normals is None else np.array_equal(back["normals"], normals)
    # a colourless file is, byte for byte, what it was before colours existed: header, float block, face records
    for normals in (m["normals"], None):
        G.write_ply(path, m["vertices"], m["faces"], normals)
        names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
        want = ("\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {nv}"]
                          + [f"property float {n}" for n in names]
                          + [f"element face {nf}", "property list uchar int vertex_indices", "end_header"]) + "\n").encode("ascii")
        cols = [m["vertices"]] + ([normals] if normals is not None else [])
        want += np.concatenate(cols, axis=1).astype("<f4").tobytes()
        want += b"".join(b"\x03" + struct.pack("<3i", *face) for face in m["faces"].tolist())
        assert open(path, "rb").read() == want
        assert G.read_ply(path)["colors"] is None
    G.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, np.zeros((0, 3), np.uint8))
    back = G.read_ply(path)
    assert back["colors"].shape == (0, 3) and back["vertices"].shape == (0, 3) and back["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="uint8"):
        G.write_ply(path, m["vertices"], m["faces"], None, colors.astype(np.float32))
    with pytest.raises(ValueError, match="colors for"):
        G.write_ply(path, m["vertices"], m["faces"], None, colors[:-1])


def test_argument_errors_need_no_gpu():
    faces = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        HN.mesh_components(faces, 4)
    with pytest.raises(ValueError, match="int32"):
        HN.mesh_components(faces.long(), 4)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        HN.mesh_components(torch.zeros((2, 4), dtype=torch.int32), 4)
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):
        HN.mesh_components(faces, 2 ** 31)
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):
        HN.mesh_components(faces, -1)
    with pytest.raises(ValueError, match="labels"):
        HN.component_sizes(torch.zeros(4), faces)
    mesh = {"vertices": torch.zeros(4, 3), "normals": torch.zeros(4, 3), "faces": faces}
    assert HN.filter_mesh(mesh) is mesh                                     # nothing to do, nothing touched
    with pytest.raises(ValueError, match="GPU"):
        HN.filter_mesh(mesh, keep_largest=1)
    m = torch.nn.Linear(1, 1)
    v = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="dtype"):
        HN.vertex_colors(m, v, v, 0, dtype=torch.float16)
    with pytest.raises(ValueError, match="chunk"):
        HN.vertex_colors(m, v, v, 0, chunk=0)
    with pytest.raises(ValueError, match="view"):
        HN.vertex_colors(m, v, v, 0, view="camera")
    with pytest.raises(ValueError, match="three components"):
        HN.vertex_colors(m, v, v, 0, view=(0.0, 1.0))
    with pytest.raises(ValueError, match="needs normals"):
        HN.vertex_colors(m, v, None, 0)
    with pytest.raises(L.HnError):                                          # a model on the CPU: no CPU fallback
        HN.vertex_colors(m, v, v, 0)
    assert {"mesh_components", "component_sizes", "filter_mesh", "vertex_colors"} <= set(dir(HN))


def test_c_abi_refuses_bad_meshes_before_any_launch():
    """Status -2 on the host, no launch, no GPU needed: NULL pointers, negative counts, V or F beyond 2^31 - 1."""
    HN.build()
    lib = L.load()
    names = {"hn_cc_init", "hn_cc_round", "hn_cc_sizes", "hn_mesh_keep", "hn_mesh_compact", "hn_gather_rows",
             "hn_vertex_viewdirs"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES)
    header = open(L.HEADER).read()
    assert all(f"int {n}(" in header for n in names)
    one, big = C.c_void_p(16), 2 ** 31                                      # never dereferenced: refused first
    cam = (C.c_float * 3)(0.0, 0.0, 0.0)
    assert lib.hn_cc_init(one, -1, one, 4, one, None) == -2
    assert lib.hn_cc_init(one, 4, one, -1, one, None) == -2
    assert lib.hn_cc_init(one, big, one, 4, one, None) == -2
    assert lib.hn_cc_init(one, 4, one, big, one, None) == -2
    assert lib.hn_cc_init(None, 4, one, 4, one, None) == -2
    assert lib.hn_cc_init(one, 4, None, 4, one, None) == -2
    assert lib.hn_cc_init(one, 4, one, 4, None, None) == -2
    assert lib.hn_cc_round(one, 0, one, 4, 1, one, None) == -2
    assert lib.hn_cc_round(one, 4, one, 0, 1, one, None) == -2
    assert lib.hn_cc_round(one, big, one, 4, 1, one, None) == -2
    assert lib.hn_cc_round(one, 4, one, big, 1, one, None) == -2
    assert lib.hn_cc_round(one, 4, one, 4, 0, one, None) == -2
    assert lib.hn_cc_round(None, 4, one, 4, 1, one, None) == -2
    assert lib.hn_cc_round(one, 4, None, 4, 1, one, None) == -2
    assert lib.hn_cc_round(one, 4, one, 4, 1, None, None) == -2
    assert lib.hn_cc_sizes(None, one, 4, 4, one, one, None) == -2
    assert lib.hn_cc_sizes(one, one, 4, 4, None, one, None) == -2
    assert lib.hn_cc_sizes(one, one, -4, 4, one, one, None) == -2
    assert lib.hn_cc_sizes(one, one, 4, big, one, one, None) == -2
    assert lib.hn_mesh_keep(one, one, None, 4, 4, one, one, None) == -2
    assert lib.hn_mesh_keep(one, None, one, 4, 4, one, one, None) == -2
    assert lib.hn_mesh_keep(one, one, one, big, 4, one, one, None) == -2
    assert lib.hn_mesh_keep(one, one, one, 4, -1, one, one, None) == -2
    assert lib.hn_mesh_compact(one, one, one, 4, 4, 5, 4, one, one, None) == -2      # more kept than there are
    assert lib.hn_mesh_compact(one, one, one, 4, 4, 4, -1, one, one, None) == -2
    assert lib.hn_mesh_compact(one, None, one, 4, 4, 4, 4, one, one, None) == -2
    assert lib.hn_mesh_compact(one, one, one, 4, 4, 4, 4, one, None, None) == -2
    assert lib.hn_mesh_compact(one, one, one, 4, big, 4, 4, one, one, None) == -2
    assert lib.hn_gather_rows(None, 4, one, 4, 12, one, None) == -2
    assert lib.hn_gather_rows(one, 4, one, 0, 12, one, None) == -2
    assert lib.hn_gather_rows(one, 4, one, 4, 0, one, None) == -2
    assert lib.hn_gather_rows(one, big, one, 4, 12, one, None) == -2
    assert lib.hn_vertex_viewdirs(one, None, 4, 0, 4, None, one, None) == -2         # head-on needs the normals
    assert lib.hn_vertex_viewdirs(None, one, 4, 0, 4, cam, one, None) == -2          # a camera needs the positions
    assert lib.hn_vertex_viewdirs(one, one, 4, 4, 4, None, one, None) == -2          # start past the mesh
    assert lib.hn_vertex_viewdirs(one, one, 4, -1, 4, None, one, None) == -2
    assert lib.hn_vertex_viewdirs(one, one, 4, 0, 0, None, one, None) == -2
    assert lib.hn_vertex_viewdirs(one, one, big, 0, 4, None, one, None) == -2
    assert lib.hn_vertex_viewdirs(one, one, 4, 0, 4, None, None, None) == -2
