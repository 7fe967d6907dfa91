"""Host tests of the texture atlas (csrc/hn_texture.hip, geometry.texture_atlas / rasterize_atlas / bake_texture /
render_textured_mesh / write_obj), no GPU: the argument refusals, the invariants of the NumPy restatement
(tests/texture_restated.py) on the test meshes, the host arithmetic of the atlas size against it, the OBJ round trip from
host arrays, the binding."""
import os
import re

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import geometry as G
from hypernerf_torch_amd import inference

import hashprng as H
import texture_restated as T
import texture_scenes as S

OPS = HN.ops.texture
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_mesh(name):
    return {k: torch.from_numpy(v) for k, v in S.mesh(name).items()}


def layout(name, min_cell=16, max_cell=S.MAX_CELL, texel=None):
    m = S.mesh(name)
    return T.layout(m["vertices"], m["faces"], S.TEXEL[name] if texel is None else texel, min_cell, max_cell)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(min_cell=24), "powers of two"), (dict(max_cell=100), "powers of two"), (dict(min_cell=8), "16 <= min_cell"),
    (dict(max_cell=2048), "max_cell <= 1024"), (dict(min_cell=64, max_cell=32), "min_cell <= max_cell"),
    (dict(min_cell=16.0), "powers of two"), (dict(min_cell=True), "powers of two"),
    (dict(texel=0.0), "texel"), (dict(texel=-1.0), "texel"), (dict(texel=float("nan")), "texel"),
    (dict(texel=float("inf")), "texel"), (dict(texel=1e-50), "texel"), (dict(texel="fine"), "texel"),
    (dict(max_size=16385), "size must be an int in 1 .. 16384"), (dict(max_size=0), "size must be an int"),
    (dict(max_size=512.0), "size must be an int")])
def test_texture_atlas_refuses_bad_arguments_before_it_looks_at_the_device(kw, match):
    args = dict(texel=0.05)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        HN.texture_atlas(host_mesh("tetra"), **args)
    if "texel" not in kw:
        with pytest.raises(ValueError, match=match):
            HN.atlas_texel_for_size(host_mesh("tetra"), kw.pop("max_size", 512), **kw)


def test_a_host_mesh_is_refused_not_computed_on_the_cpu():
    for call in (lambda m: HN.texture_atlas(m, 0.05), lambda m: HN.atlas_texel_for_size(m, 512)):
        with pytest.raises((ValueError, L.HnError), match="GPU"):
            call(host_mesh("tetra"))
    with pytest.raises(ValueError, match="dict"):
        HN.texture_atlas([1, 2], 0.05)
    with pytest.raises(ValueError, match="int32"):
        HN.texture_atlas({"vertices": torch.zeros(3, 3), "faces": torch.zeros(1, 3, dtype=torch.int64)}, 0.05)


def test_the_size_refusal_names_the_size_needed():
    lay = layout("bumpy")
    hist = np.bincount(np.log2(lay["sides"]).astype(int), minlength=11).tolist()
    assert OPS.check_atlas_fits(hist, 16, 512, "texture_atlas") == lay["size"] == (512, 512)
    with pytest.raises(ValueError, match=r"texture_atlas: the atlas needs 512 x 512 texels, max_size is 256"):
        OPS.check_atlas_fits(hist, 16, 256, "texture_atlas")
    with pytest.raises(ValueError, match=r"needs 64 x 32 texels, max_size is 32"):
        OPS.check_atlas_fits([0] * 5 + [4] + [0] * 5, 16, 32, "texture_atlas")      # four faces of side 32: the tetrahedron


def _atlas_from(lay, min_cell=16):
    hist = np.bincount(np.log2(lay["sides"]).astype(int), minlength=11).tolist() if len(lay["sides"]) else [0] * 11
    return {"uv": torch.from_numpy(lay["uv"]), "size": lay["size"], "cell_start": torch.from_numpy(lay["cell_start"]),
            "cell_side": torch.from_numpy(lay["cell_side"]), "cell_face": torch.from_numpy(lay["cell_face"]),
            "texel": 0.05, "min_cell": min_cell, "class_cells": tuple(OPS.class_cells(hist)[1])}


def test_texture_and_atlas_mismatches_are_refused(tmp_path):
    lay = layout("tetra")
    atlas, mesh = _atlas_from(lay), host_mesh("tetra")
    w, h = lay["size"]
    good = torch.zeros((h, w, 3), dtype=torch.uint8)
    OPS.check_atlas(atlas, 4, "t")
    assert OPS.check_texture(good, atlas, "t") is not None
    with pytest.raises(ValueError, match=r"texture is \(64, 32, 3\), the atlas is \(32, 64, 3\)"):
        OPS.check_texture(torch.zeros((w, h, 3), dtype=torch.uint8), atlas, "t")
    with pytest.raises(ValueError, match="uint8 or float32"):
        OPS.check_texture(good.double(), atlas, "t")
    with pytest.raises(ValueError, match="lays out 4 faces, the mesh has 5"):
        OPS.check_atlas(atlas, 5, "t")
    for broken in (dict(atlas, uv=atlas["uv"].double()), dict(atlas, size=(w + 1, h)), dict(atlas, min_cell=24),
                   dict(atlas, class_cells=(0, 1)), {k: v for k, v in atlas.items() if k != "cell_face"}, None, 3):
        with pytest.raises(ValueError, match="the dict texture_atlas returns"):
            OPS.check_atlas(broken, None, "t")
    path = str(tmp_path / "t.obj")
    with pytest.raises(ValueError, match="texture must be uint8"):
        HN.write_obj(path, mesh, atlas, good.double())
    with pytest.raises(ValueError, match="texture must be uint8"):
        HN.write_obj(path, mesh, atlas, good.float())
    with pytest.raises(ValueError, match=r"texture is \(16, 16, 3\)"):
        HN.write_obj(path, mesh, atlas, torch.zeros((16, 16, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="lays out 4 faces, the mesh has 320"):
        HN.write_obj(path, host_mesh("bumpy"), atlas, good)
    with pytest.raises(ValueError, match=r"\.obj"):
        HN.write_obj(str(tmp_path / "t.ply"), mesh, atlas, good)
    assert not os.listdir(tmp_path)
    # the GPU-only functions check their arguments first, then refuse the host tensors
    with pytest.raises(ValueError, match="filter"):
        HN.render_textured_mesh(mesh, atlas, good, torch.zeros(12, 8), torch.zeros(24), (4, 3), filter="cubic")
    with pytest.raises(ValueError, match="shading"):
        HN.render_textured_mesh(mesh, atlas, good, torch.zeros(12, 8), torch.zeros(24), (4, 3), shading="phong")
    with pytest.raises(ValueError, match="texture is"):
        HN.render_textured_mesh(mesh, atlas, good[:16], torch.zeros(12, 8), torch.zeros(24), (4, 3))
    with pytest.raises(ValueError, match="GPU"):
        HN.render_textured_mesh(mesh, atlas, good, torch.zeros(12, 8), torch.zeros(24), (4, 3))
    with pytest.raises(ValueError, match="GPU"):
        HN.rasterize_atlas(mesh, atlas)
    for kw, match in ((dict(dtype=torch.float64), "dtype"), (dict(fill=256), "fill"), (dict(fill=-1), "fill"),
                      (dict(fill=0.5), "fill"), (dict(dtype=torch.float32, fill=float("nan")), "fill")):
        with pytest.raises(ValueError, match=match):
            HN.bake_texture(mesh, atlas, lambda p, n: p, **kw)
    with pytest.raises(ValueError, match="callable"):
        HN.bake_texture(mesh, atlas, None)


# ---- the restatement's own invariants ---------------------------------------------------------------------------------------
CASES = [(name, 16, S.MAX_CELL) for name in S.NAMES] + [("bumpy", 32, 64), ("bumpy", 16, 16), ("tetra", 64, 256)]


@pytest.mark.parametrize("name,min_cell,max_cell", CASES)
def test_restated_layout_invariants(name, min_cell, max_cell):
    lay = layout(name, min_cell, max_cell)
    n_faces = len(S.mesh(name)["faces"])
    (w, h), start, side, pair = lay["size"], lay["cell_start"], lay["cell_side"], lay["cell_face"]
    assert w & (w - 1) == 0 and w >= min_cell and h in (w, w // 2)
    assert ((side >= min_cell) & (side <= max_cell) & (side & (side - 1) == 0)).all()
    assert (np.diff(side) <= 0).all()                                        # descending sides
    assert (start % side[:, None] == 0).all(), "a cell origin is aligned to the cell's side"
    assert (start >= 0).all() and (start[:, 0] + side <= w).all() and (start[:, 1] + side <= h).all()
    taken = np.zeros((h // min_cell, w // min_cell), dtype=np.int32)
    for (ox, oy), s in zip(start.tolist(), side.tolist()):
        taken[oy // min_cell:(oy + s) // min_cell, ox // min_cell:(ox + s) // min_cell] += 1
    assert taken.max(initial=0) <= 1, "two cells overlap"
    # the size is the smallest: the square one step down does not hold the cells, and the half is taken exactly when it fits
    area = int((side.astype(np.int64) ** 2).sum())
    if len(side):
        assert area > (w // 2) ** 2 or w == min_cell
        assert (h == w // 2) == (w > min_cell and bool((start[:, 1] + side <= w // 2).all()))
    else:
        assert (w, h) == (min_cell, min_cell)
    members = pair[pair >= 0]
    assert sorted(members.tolist()) == list(range(n_faces)), "every face sits in exactly one half-cell"
    assert (pair[:, 0] >= 0).all() and (lay["sides"][pair[:, 0]] == side).all()
    both = pair[:, 1] >= 0
    assert (lay["sides"][pair[both, 1]] == side[both]).all()
    for s in np.unique(side):                                                # an odd class leaves only its LAST upper half empty
        assert (~both[side == s])[:-1].sum() == 0
    # the product's host arithmetic gives the same size from the histogram
    hist = np.bincount(np.log2(lay["sides"]).astype(int), minlength=11).tolist() if n_faces else [0] * 11
    assert OPS.atlas_size(hist, min_cell) == (w, h)
    assert OPS.class_cells(hist)[1][-1] == len(side)


def test_the_test_meshes_cover_the_cases_they_are_there_for():
    sides = layout("bumpy")["sides"]
    counts = np.unique(sides, return_counts=True)[1]
    assert len(counts) >= 3 and (counts % 2 == 1).any()
    assert len(np.unique(layout("tetra")["sides"])) == 1 and layout("tetra")["size"] == (64, 32)
    plus, m = layout("bumpy_plus"), S.mesh("bumpy_plus")
    n = len(m["faces"])
    assert plus["sides"][n - 1] == 16 and plus["sides"][n - 2] == S.MAX_CELL          # the point face, the long face
    v = m["vertices"][m["faces"][n - 2]].astype(np.float64)
    assert np.linalg.norm(v[1] - v[0]) > (S.MAX_CELL - 7) * S.TEXEL["bumpy_plus"]
    assert max(layout(name)["size"][0] for name in S.NAMES) <= 512


@pytest.mark.parametrize("name", ["tetra", "bumpy_plus"])
def test_restated_ownership_and_the_gutter(name):
    """Every texel a bilinear fetch reads — at 2000 hashed points per mesh, every corner and every edge midpoint — belongs
    to the face it is fetched for, in the restatement's own rasterisation."""
    m, lay = S.mesh(name), layout(name)
    owner = T.rasterize(m["vertices"], m["faces"], m.get("normals"), lay)["owner"]
    n_faces = len(m["faces"])
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]], dtype=F32)
    face = np.concatenate([np.repeat(np.arange(n_faces), 6), (H.uniform01(3, "tex_face", 2000) * n_faces).astype(np.int64)])
    bary = np.concatenate([np.tile(fixed, (n_faces, 1)), S.hashed_barycentrics(4, 2000)])
    reads = T.fetch_set(lay["uv"], face, bary)
    assert (owner[reads[..., 1], reads[..., 0]] == face[:, None]).all()
    # one ring inside: the neighbours of every texel read WITH A WEIGHT are owned by the face too, or (past the hypotenuse)
    # by nobody.  (A texel read with weight 0 — i1 at a whole a = u - 0.5 — can be the cell's last column in the upper half.)
    t = T.chart_uv(lay["uv"], face, bary) - F32(0.5)
    fx, fy = t[:, 0] - np.floor(t[:, 0]), t[:, 1] - np.floor(t[:, 1])
    weighted = np.stack([np.ones_like(fx, dtype=bool), fx > 0, fy > 0, (fx > 0) & (fy > 0)], axis=1)
    assert not weighted.all()                                                # the corners sit on whole coordinates
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        ring = owner[np.clip(reads[..., 1] + dj, 0, owner.shape[0] - 1), np.clip(reads[..., 0] + di, 0, owner.shape[1] - 1)]
        assert ((ring == face[:, None]) | (ring == -1) | ~weighted).all()


def test_restated_position_is_the_affine_chart():
    """position at the texel under a corner's centre is the vertex; along the chart it is affine in the texel index."""
    m, lay = S.mesh("tetra"), layout("tetra")
    r = T.rasterize(m["vertices"], m["faces"], None, lay)
    for f in range(4):
        for k in range(3):
            x, y = lay["uv"][f, k]
            assert np.array_equal(r["position"][int(y), int(x)], m["vertices"][m["faces"][f, k]])
            assert r["owner"][int(y), int(x)] == f
    second = r["position"][2:-2, 2:] - 2 * r["position"][2:-2, 1:-1] + r["position"][2:-2, :-2]
    same = (r["owner"][2:-2, 2:] == r["owner"][2:-2, :-2]) & (r["owner"][2:-2, 1:-1] >= 0) & \
        (r["owner"][2:-2, 2:] == r["owner"][2:-2, 1:-1])
    assert same.sum() > 500 and np.abs(second[same]).max() < 1e-6


# ---- OBJ --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bumpy", "tetra", "empty"])
def test_obj_round_trip_from_host_tensors(tmp_path, name):
    m, lay = S.mesh(name), layout(name)
    w, h = lay["size"]
    texture = (H.uniform01(9, "obj_tex", h * w * 3) * 256).astype(np.uint8).reshape(h, w, 3)
    path = tmp_path / "frame.obj"
    HN.write_obj(path, host_mesh(name), _atlas_from(lay), torch.from_numpy(texture))
    assert sorted(os.listdir(tmp_path)) == ["frame.mtl", "frame.obj", "frame.png"]
    back = HN.read_obj(path)
    assert back["vertices"].dtype == np.float32 and np.array_equal(back["vertices"].view(np.int32), m["vertices"].view(np.int32))
    assert back["faces"].dtype == np.int32 and np.array_equal(back["faces"], m["faces"])
    if "normals" in m:
        assert np.array_equal(back["normals"].view(np.int32), m["normals"].view(np.int32))
    else:
        assert back["normals"] is None
    assert back["uv"].shape == lay["uv"].shape and np.array_equal(back["uv"], lay["uv"])      # power-of-two sides: exact
    if len(m["faces"]):
        assert 0.0 < back["vt"].min() and back["vt"].max() < 1.0
    assert np.array_equal(back["texture"], texture) and np.array_equal(inference.read_png(str(tmp_path / "frame.png")), texture)
    assert back["size"] == (w, h) and back["mtl"] == "frame.mtl" and back["map_Kd"] == "frame.png"
    assert "map_Kd frame.png" in (tmp_path / "frame.mtl").read_text()
    text = (tmp_path / "frame.obj").read_text()
    assert text.startswith("mtllib frame.mtl\n") and ("usemtl frame\n" in text)
    assert len(re.findall(r"^vt ", text, flags=re.M)) == 3 * len(m["faces"])
    # row 0 of the image is the top: v = 1 - y / H_t
    if len(m["faces"]):
        assert back["vt"][0, 0, 1] == 1.0 - float(lay["uv"][0, 0, 1]) / h


# ---- the binding --------------------------------------------------------------------------------------------------------------
def test_binding_and_public_surface():
    names = {"hn_tex_classify": 11, "hn_tex_layout": 10, "hn_tex_rasterize": 15, "hn_tex_shade": 23}
    HN.build()
    lib = L.load()
    assert lib.hn_version() == 340 and L.HN_VERSION == 340
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hn_kernels.h")).read(), flags=re.S)
    for name, n_args in names.items():
        assert name in L.EXPORTS and hasattr(lib, name) and "hn_texture.hip" in L.SOURCES
        params = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M).group(1)
        assert len(L.ARGTYPES[name]) == params.count(",") + 1 == n_args
        assert getattr(lib, name).argtypes == L.ARGTYPES[name]
    assert not [k for k in L.CONSTANTS if k.startswith("HN_TEX")], "the header's constants stay those of ABI 340"
    # status codes before any launch: a size out of range, then a NULL pointer
    assert lib.hn_tex_classify(None, 3, None, 1, 0.1, 24, 64, None, None, None, None) == -2
    assert lib.hn_tex_classify(None, 3, None, 1, 0.0, 16, 64, None, None, None, None) == -2
    assert lib.hn_tex_classify(None, 3, None, 1, 0.1, 16, 64, None, None, None, None) == -3
    import ctypes
    table = (ctypes.c_int64 * 8)(0, 0, 0, 0, 0, 0, 0, 4)
    assert lib.hn_tex_layout(None, 4, table, 16, 2, None, None, None, None, None) == -3
    assert lib.hn_tex_layout(None, 4, table, 16, 3, None, None, None, None, None) == -2        # 4 faces are 2 cells
    assert lib.hn_tex_layout(None, 5, table, 16, 2, None, None, None, None, None) == -2        # the table ends at 4
    assert lib.hn_tex_layout(None, 4, (ctypes.c_int64 * 8)(0, 4, 4, 4, 4, 4, 4, 4), 16, 2, None, None, None, None, None) == -3
    assert lib.hn_tex_layout(None, 4, (ctypes.c_int64 * 8)(0, 0, 0, 0, 0, 0, 0, 4), 32, 2, None, None, None, None, None) == -2
    cells = (ctypes.c_int64 * 8)(0, 0, 0, 0, 0, 0, 0, 0)
    assert lib.hn_tex_rasterize(None, 0, None, 0, None, None, 0, cells, 16, 16, 24, None, None, None, None) == -2
    assert lib.hn_tex_rasterize(None, 0, None, 0, None, None, 0, cells, 16, 16, 32768, None, None, None, None) == -2
    assert lib.hn_tex_rasterize(None, 0, None, 0, None, None, 0, cells, 16, 16, 16, None, None, None, None) == -3
    bg = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hn_tex_shade(None, 0, None, 0, None, None, None, 3, 16, 16, 1, None, 8, 4, None, None, 1, 0.3, bg, None, None,
                            None, None) == -2
    assert lib.hn_tex_shade(None, 0, None, 0, None, None, None, 1, 16, 16, 2, None, 8, 4, None, None, 1, 0.3, bg, None, None,
                            None, None) == -2
    assert lib.hn_tex_shade(None, 0, None, 0, None, None, None, 1, 16, 16, 1, None, 8, 4, None, None, 1, 0.3, bg, None, None,
                            None, None) == -3
    # the package, its re-exports, the documents
    assert HN.ops.texture is OPS and "texture" in HN.ops.__all__ and "hn_texture.hip" in HN.ops.__doc__
    assert os.path.isdir(os.path.join(ROOT, "hypernerf-torch_amd", "ops", "texture"))
    for name in OPS.__all__:
        assert getattr(F, name) is getattr(OPS, name), name
    for name in ("texture_atlas", "atlas_texel_for_size", "rasterize_atlas", "bake_texture", "bake_field_texture",
                 "render_textured_mesh", "write_obj", "read_obj"):
        assert getattr(HN, name) is getattr(G, name), name
    assert (OPS.TEX_MIN_SIDE, OPS.TEX_MAX_SIDE, OPS.TEX_MAX_ATLAS, OPS.TEX_GUTTER, OPS.TEX_CLASSES) == (16, 1024, 16384, 7, 7)
    src = open(os.path.join(ROOT, "hypernerf-torch_amd", "csrc", "hn_texture.hip")).read()
    for macro, value in (("HN_TEX_MIN_SIDE", 16), ("HN_TEX_MAX_SIDE", 1024), ("HN_TEX_MAX_ATLAS", 16384), ("HN_TEX_GUTTER", 7),
                         ("HN_TEX_CLASSES", 7)):
        assert re.search(r"#define %s (\d+)" % macro, src).group(1) == str(value)
    assert "3.16" in open(os.path.join(ROOT, "DESIGN.md")).read()
