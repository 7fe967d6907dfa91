"""GPU tests of the texture atlas (csrc/hn_texture.hip; geometry.texture_atlas, rasterize_atlas, bake_texture,
bake_field_texture, render_textured_mesh, write_obj) against the face-by-face NumPy restatement (tests/texture_restated.py):
layout and rasterisation bit for bit, the ownership invariant of the bilinear fetch, affine reproduction through the
renderer, sampler parity on a noise texture, the baking bookkeeping, the field, determinism, the OBJ round trip."""
import functools
import os

import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
import mesh_render_scenes as MS
import test_gpu_geometry as TG
import texture_restated as T
import texture_scenes as S
from gpu_common import DEV
from hypernerf_torch_amd import inference

pytestmark = pytest.mark.gpu

F32 = np.float32
MESHES = ("tetra", "bumpy", "bumpy_plus")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a).reshape(-1), bits(b).reshape(-1))


@pytest.fixture
def fp32():
    HN.set_precision("fp32")
    yield
    HN.set_precision("bf16")


@functools.lru_cache(maxsize=None)
def gpu_mesh(name):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in S.mesh(name).items()}


@functools.lru_cache(maxsize=None)
def gpu_atlas(name, min_cell=16, max_cell=S.MAX_CELL):
    return HN.texture_atlas(gpu_mesh(name), S.TEXEL[name], min_cell, max_cell, max_size=512)


@functools.lru_cache(maxsize=None)
def gpu_raster(name):
    return HN.rasterize_atlas(gpu_mesh(name), gpu_atlas(name))


@functools.lru_cache(maxsize=None)
def host_layout(name, min_cell=16, max_cell=S.MAX_CELL):
    m = S.mesh(name)
    return T.layout(m["vertices"], m["faces"], S.TEXEL[name], min_cell, max_cell)


@functools.lru_cache(maxsize=None)
def host_raster(name):
    m = S.mesh(name)
    return T.rasterize(m["vertices"], m["faces"], m.get("normals"), host_layout(name))


@functools.lru_cache(maxsize=None)
def gpu_rays(cam_name):
    cam = torch.from_numpy(MS.camera(cam_name, MS.WH)).to(DEV)
    return cam, HN.camera_rays(cam, MS.WH[0], MS.WH[1], 0.0, 6.0)


# ---- layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,min_cell,max_cell", [(n, 16, S.MAX_CELL) for n in S.NAMES] +
                         [("bumpy", 32, 64), ("bumpy", 16, 16), ("tetra", 64, 256), ("bumpy_plus", 16, 32)])
def test_layout_equals_the_restatement(name, min_cell, max_cell):
    got, want = gpu_atlas(name, min_cell, max_cell), host_layout(name, min_cell, max_cell)
    assert tuple(got["size"]) == tuple(want["size"]), (got["size"], want["size"])
    for key in ("cell_start", "cell_side", "cell_face"):
        assert got[key].dtype == torch.int32 and got[key].device.type == "cuda"
        assert np.array_equal(host(got[key]), want[key]), key
    assert same_bits(got["uv"], want["uv"])
    assert got["texel"] == float(F32(S.TEXEL[name])) and got["min_cell"] == min_cell


def test_the_meshes_hold_the_cases_on_the_device_too():
    sides = host(gpu_atlas("bumpy")["cell_side"])
    pair = host(gpu_atlas("bumpy")["cell_face"])
    faces_per_side = {int(s): int((pair[sides == s] >= 0).sum()) for s in np.unique(sides)}
    assert len(faces_per_side) >= 3 and any(n % 2 for n in faces_per_side.values()), faces_per_side
    assert (pair[:, 1] < 0).sum() == sum(n % 2 for n in faces_per_side.values())
    assert tuple(gpu_atlas("tetra")["size"]) == (64, 32)                       # the half-height case
    assert tuple(gpu_atlas("empty")["size"]) == (16, 16) and gpu_atlas("empty")["uv"].shape == (0, 3, 2)


def test_refusals_on_the_device():
    m = gpu_mesh("bumpy")
    v = m["vertices"].shape[0]
    bad = dict(m, faces=m["faces"].clone())
    bad["faces"][17, 1] = v
    with pytest.raises(ValueError, match=rf"vertex id outside \[0, {v}\)"):
        HN.texture_atlas(bad, S.TEXEL["bumpy"])
    bad["faces"][17, 1] = -1
    with pytest.raises(ValueError, match="vertex id outside"):
        HN.texture_atlas(bad, S.TEXEL["bumpy"])
    with pytest.raises(ValueError, match="vertex id outside"):
        HN.atlas_texel_for_size(bad, 512)
    with pytest.raises(ValueError, match=r"the atlas needs 512 x 512 texels, max_size is 256"):
        HN.texture_atlas(m, S.TEXEL["bumpy"], 16, S.MAX_CELL, max_size=256)
    # a mesh that is not the atlas's: ids out of range own nothing and read nothing
    fewer = dict(m, vertices=m["vertices"][:100].contiguous(), normals=m["normals"][:100].contiguous())
    r = HN.rasterize_atlas(fewer, gpu_atlas("bumpy"))
    owner, faces = host(r["owner"]), S.mesh("bumpy")["faces"]
    inside = (faces < 100).all(axis=1)
    want = host_raster("bumpy")["owner"]
    assert np.array_equal(owner, np.where((want >= 0) & inside[np.maximum(want, 0)], want, -1))
    assert not host(r["position"])[owner < 0].any()


def test_texel_for_size_walks_the_ladder():
    m, data = gpu_mesh("bumpy"), S.mesh("bumpy")
    longest = float((data["vertices"].max(0).astype(np.float64) - data["vertices"].min(0)).max())
    for size in (512, 256):
        texel = HN.atlas_texel_for_size(m, size, 16, S.MAX_CELL)
        ladder = [float(F32(2.0 ** (0.5 * k) * longest / size)) for k in range(64)]
        assert texel in ladder
        k = ladder.index(texel)
        assert max(T.layout(data["vertices"], data["faces"], texel, 16, S.MAX_CELL)["size"]) <= size
        assert k > 0 and max(T.layout(data["vertices"], data["faces"], ladder[k - 1], 16, S.MAX_CELL)["size"]) > size
        assert max(HN.texture_atlas(m, texel, 16, S.MAX_CELL, max_size=size)["size"]) <= size
    with pytest.raises(ValueError, match="even with every face"):
        HN.atlas_texel_for_size(m, 128, 16, S.MAX_CELL)                       # 160 cells of 16 need 256 x 256
    with pytest.raises(ValueError, match="no faces"):
        HN.atlas_texel_for_size(gpu_mesh("empty"), 128)


# ---- rasterisation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_rasterisation_equals_the_restatement_bit_for_bit(name):
    got, want = gpu_raster(name), host_raster(name)
    w, h = gpu_atlas(name)["size"]
    assert got["owner"].shape == (h, w) and got["position"].shape == (h, w, 3) and got["normal"].shape == (h, w, 3)
    assert np.array_equal(host(got["owner"]), want["owner"])
    for key in ("position", "normal"):
        a, b = host(got[key]), want[key]
        print(f"rasterize {name} {key}: max |difference| {np.abs(a.astype(np.float64) - b).max(initial=0.0):.3g}")
        assert same_bits(a, b), key
    assert not host(got["position"])[want["owner"] < 0].any() and not host(got["normal"])[want["owner"] < 0].any()


def test_rasterisation_without_vertex_normals_uses_the_face_normal():
    m, data = gpu_mesh("bumpy_plus"), S.mesh("bumpy_plus")
    got = HN.rasterize_atlas({"vertices": m["vertices"], "faces": m["faces"]}, gpu_atlas("bumpy_plus"))
    want = T.rasterize(data["vertices"], data["faces"], None, host_layout("bumpy_plus"))
    assert np.array_equal(host(got["owner"]), want["owner"])
    assert same_bits(got["position"], want["position"]) and same_bits(got["normal"], want["normal"])
    n_faces = len(data["faces"])
    for degenerate in (n_faces - 3, n_faces - 1):                             # the collinear face, the point face
        assert (want["owner"] == degenerate).any() and not want["normal"][want["owner"] == degenerate].any()


# ---- the ownership invariant ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_every_texel_a_bilinear_fetch_reads_belongs_to_the_face(name):
    """10^4 hashed points per mesh plus every corner and edge midpoint of every face: the four texels hn_tex_shade's
    bilinear fetch reads (the restatement's fetch_set: the same fp32 expression, from the DEVICE's uv) all have
    owner == face on the device's owner image.  No exceptions."""
    n_faces = len(S.mesh(name)["faces"])
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]], dtype=F32)
    face = np.concatenate([np.repeat(np.arange(n_faces), 6), (H.uniform01(3, "tex_face", 10000) * n_faces).astype(np.int64)])
    bary = np.concatenate([np.tile(fixed, (n_faces, 1)), S.hashed_barycentrics(4, 10000)])
    reads = T.fetch_set(host(gpu_atlas(name)["uv"]), face, bary)
    owner = host(gpu_raster(name)["owner"])
    assert reads.min() >= 0 and reads[..., 0].max() < owner.shape[1] and reads[..., 1].max() < owner.shape[0]
    wrong = owner[reads[..., 1], reads[..., 0]] != face[:, None]
    assert wrong.sum() == 0, f"{int(wrong.sum())} texels read outside their face's chart"


# ---- affine reproduction ----------------------------------------------------------------------------------------------------
def affine_for(name):
    """(A (3, 3), c (3,)) float64 with A x + c in [0.1, 0.9] over the mesh's vertices, each channel reaching both ends."""
    v = S.mesh(name)["vertices"].astype(np.float64)
    a = np.array([[0.9, -0.4, 0.3], [-0.2, 0.8, 0.5], [0.4, 0.6, -0.7]])
    raw = v @ a.T
    scale = 0.8 / (raw.max(0) - raw.min(0))
    return a * scale[:, None], 0.1 - raw.min(0) * scale


@functools.lru_cache(maxsize=None)
def affine_texture(name):
    a, c = affine_for(name)
    at, ct = torch.from_numpy(a.astype(F32)).to(DEV), torch.from_numpy(c.astype(F32)).to(DEV)
    return HN.bake_texture(gpu_mesh(name), gpu_atlas(name),
                           lambda p, n: ((p[:, None, :] * at[None]).sum(-1) + ct).clamp(0.0, 1.0), dtype=torch.float32)


@pytest.mark.parametrize("cam_name", MS.CAMERAS)
@pytest.mark.parametrize("name", MESHES)
def test_an_affine_colour_comes_back_through_the_renderer(name, cam_name):
    """shading='none': the rendered colour at a hit pixel is A x + c at x = sum b_k v_k within 2e-4 (bilinear: (u, v) carries
    ~1e-4 texel of fp32 rounding at magnitudes <= 512, the colour moves by at most 0.8 / 9 per texel) and within one
    texel's colour step 0.8 / L_min = 0.8 / 9 (nearest).  Observed maxima: DESIGN.md 3.16."""
    data, m = S.mesh(name), gpu_mesh(name)
    a, c = affine_for(name)
    a32, c32 = a.astype(F32).astype(np.float64), c.astype(F32).astype(np.float64)
    cam, rays = gpu_rays(cam_name)
    for filt, bound in (("bilinear", 2e-4), ("nearest", 0.8 / 9)):
        img = HN.render_textured_mesh(m, gpu_atlas(name), affine_texture(name), rays, cam, MS.WH, shading="none", filter=filt)
        face, bary = host(img["face"]).reshape(-1), host(img["bary"]).reshape(-1, 3).astype(np.float64)
        hit = face >= 0
        assert hit.sum() > 200, (name, cam_name, int(hit.sum()))
        corners = data["vertices"].astype(np.float64)[data["faces"][face[hit]]]           # (n, 3, 3)
        x = (bary[hit][:, :, None] * corners).sum(axis=1)
        want = x @ a32.T + c32
        err = np.abs(host(img["rgb"]).reshape(-1, 3)[hit].astype(np.float64) - want).max()
        print(f"affine {name} {cam_name} {filt}: max error {err:.3g} over {int(hit.sum())} pixels (bound {bound:.3g})")
        assert err < bound, (name, cam_name, filt, err)
        assert np.array_equal(host(img["rgb"]).reshape(-1, 3)[~hit], np.ones((int((~hit).sum()), 3), dtype=F32))


# ---- sampler parity ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_texture(name, kind):
    w, h = host_layout(name)["size"]
    u = H.uniform01(11, "tex_noise_" + name, h * w * 3).reshape(h, w, 3)
    return (u * 256).astype(np.uint8) if kind == "uint8" else u.astype(F32)


@pytest.mark.parametrize("filt", ["bilinear", "nearest"])
@pytest.mark.parametrize("shading,ambient", [("headlight", 0.3), ("none", 0.3)])
@pytest.mark.parametrize("name,kind,cam_name", [("bumpy", "uint8", "plain"), ("bumpy", "uint8", "distorted"),
                                                ("bumpy_plus", "uint8", "inside"), ("tetra", "uint8", "plain"),
                                                ("bumpy", "fp32", "plain")])
def test_the_sampler_against_the_restatement_on_noise(name, kind, cam_name, shading, ambient, filt):
    data, m = S.mesh(name), gpu_mesh(name)
    texture = noise_texture(name, kind)
    cam, rays = gpu_rays(cam_name)
    background = (0.25, 0.5, 1.0)
    img = HN.render_textured_mesh(m, gpu_atlas(name), torch.from_numpy(texture).to(DEV), rays, cam, MS.WH, shading=shading,
                                  ambient=ambient, background=background, filter=filt)
    face, bary = host(img["face"]).reshape(-1), host(img["bary"]).reshape(-1, 3)
    assert (face >= 0).sum() > 200
    want = T.shade(data["vertices"], data["faces"], data.get("normals"), host(gpu_atlas(name)["uv"]), texture, host(rays), face,
                   bary, shading, ambient, background, filt)
    rgb = host(img["rgb"]).reshape(-1, 3)
    print(f"sampler {name} {kind} {cam_name} {shading} {filt}: max |rgb difference| {np.abs(rgb - want['rgb']).max():.3g}")
    assert np.array_equal(host(img["rgb8"]).reshape(-1, 3), want["rgb8"])
    assert same_bits(rgb, want["rgb"])
    assert same_bits(host(img["normal"]).reshape(-1, 3), want["normal"])
    assert img["rgb"].shape == (MS.WH[1], MS.WH[0], 3) and img["rgb8"].dtype == torch.uint8


@pytest.mark.parametrize("kind", ["uint8", "fp32"])
@pytest.mark.parametrize("name,cam_name", [("bumpy", "plain"), ("tetra", "distorted"), ("empty", "plain")])
def test_a_constant_texture_is_render_mesh_with_that_base_colour(name, cam_name, kind):
    """Headlight, clamp, quantiser, normals and background: bit for bit hn_mesh_shade's, through both public functions."""
    m, (w, h) = gpu_mesh(name), gpu_atlas(name)["size"]
    byte = np.array([201, 87, 30], dtype=np.uint8)
    colour = byte.astype(F32) / F32(255.0) if kind == "uint8" else np.array([0.8, 0.35, 0.6], dtype=F32)
    texture = np.broadcast_to(byte if kind == "uint8" else colour, (h, w, 3)).copy()
    cam, rays = gpu_rays(cam_name)
    for shading, ambient, background in (("headlight", 0.3, (1.0, 1.0, 1.0)), ("headlight", 0.0, (0.1, 0.2, 0.3)),
                                         ("none", 0.3, (0.0, 0.5, 1.0))):
        plain = HN.render_mesh(m, rays, cam, MS.WH, shading=shading, ambient=ambient, background=background,
                               base_color=tuple(float(x) for x in colour))
        for filt in ("bilinear", "nearest"):
            got = HN.render_textured_mesh(m, gpu_atlas(name), torch.from_numpy(texture).to(DEV), rays, cam, MS.WH,
                                          shading=shading, ambient=ambient, background=background, filter=filt)
            assert set(got) == set(plain)
            for key in plain:
                assert got[key].shape == plain[key].shape and got[key].dtype == plain[key].dtype
                assert same_bits(got[key], plain[key]), (key, shading, filt)


# ---- baking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tetra", "bumpy_plus", "empty"])
def test_bake_texture_bookkeeping(name):
    m, atlas, rast = gpu_mesh(name), gpu_atlas(name), gpu_raster(name)
    owned = rast["owner"].view(-1) >= 0
    n = int(owned.sum())
    seen = []

    def color_fn(points, normals):
        seen.append((points, normals))
        return torch.from_numpy(H.uniform01(21, "bake_" + name, n * 3).reshape(n, 3)).to(DEV)
    tex8 = HN.bake_texture(m, atlas, color_fn, fill=7)
    tex32 = HN.bake_texture(m, atlas, color_fn, dtype=torch.float32, fill=-2.5)
    assert len(seen) == 2, "color_fn is called once per bake"
    for points, normals in seen:                                              # exactly the owned texels, row-major
        assert same_bits(points, rast["position"].view(-1, 3)[owned]) and same_bits(normals, rast["normal"].view(-1, 3)[owned])
    w, h = atlas["size"]
    colors = torch.from_numpy(H.uniform01(21, "bake_" + name, n * 3).reshape(n, 3)).to(DEV)
    assert tex8.shape == (h, w, 3) and tex8.dtype == torch.uint8 and tex32.dtype == torch.float32
    assert torch.equal(tex8.view(-1, 3)[owned], (colors * 255).to(torch.uint8))         # vertex_colors' truncation
    assert torch.equal(tex32.view(-1, 3)[owned], colors)
    assert (tex8.view(-1, 3)[~owned] == 7).all() and (tex32.view(-1, 3)[~owned] == -2.5).all()
    with pytest.raises(ValueError, match=rf"\({n}, 3\) float32"):
        HN.bake_texture(m, atlas, lambda p, q: p[:, :2])


def test_bake_field_texture_is_vertex_colors_at_the_owned_texels(fp32):
    kw, warp_kind, _ = TG.QUERY_CASES["bendy_fused"]
    model, _ = TG.small_model(kw, warp_kind, 163)
    m, atlas, rast = gpu_mesh("tetra"), gpu_atlas("tetra"), gpu_raster("tetra")
    owned = rast["owner"].view(-1) >= 0
    points, normals = rast["position"].view(-1, 3)[owned], rast["normal"].view(-1, 3)[owned]
    assert 1000 < points.shape[0] < 2048
    frame, cam = 23, (0.3, -1.7, 0.6)
    for view in ("normal", cam):
        direct = HN.vertex_colors(model, points, normals, frame, view=view, dtype=torch.float32)
        baked = HN.bake_field_texture(model, m, atlas, frame, view=view, dtype=torch.float32)
        assert getattr(model, "_level_state", None) is None
        assert same_bits(baked.view(-1, 3)[owned], direct)
        assert not baked.view(-1, 3)[~owned].any()
        assert torch.equal(HN.bake_field_texture(model, m, atlas, frame, view=view, chunk=1000, dtype=torch.float32), baked)
        baked8 = HN.bake_field_texture(model, m, atlas, frame, view=view)
        assert baked8.dtype == torch.uint8 and torch.equal(baked8.view(-1, 3)[owned],
                                                           HN.vertex_colors(model, points, normals, frame, view=view))
        assert torch.equal(HN.bake_field_texture(model, m, atlas, frame, view=view, chunk=1000), baked8)
    assert float(direct.min()) >= 0.0 and float(direct.max()) <= 1.0 and float(direct.std()) > 0.0
    with pytest.raises(ValueError, match="chunk"):
        HN.bake_field_texture(model, m, atlas, frame, chunk=0)


def test_two_runs_give_the_same_bits():
    m = gpu_mesh("bumpy_plus")
    first = gpu_atlas("bumpy_plus")
    again = HN.texture_atlas(m, S.TEXEL["bumpy_plus"], 16, S.MAX_CELL, max_size=512)
    for key in ("uv", "cell_start", "cell_side", "cell_face"):
        assert same_bits(first[key], again[key]), key
    assert first["size"] == again["size"] and first["class_cells"] == again["class_cells"]
    r1, r2 = gpu_raster("bumpy_plus"), HN.rasterize_atlas(m, again)
    for key in ("owner", "position", "normal"):
        assert same_bits(r1[key], r2[key]), key
    fn = lambda p, n: (0.5 + 0.5 * torch.sin(7.0 * p + n)).contiguous()      # noqa: E731
    assert torch.equal(HN.bake_texture(m, first, fn), HN.bake_texture(m, again, fn))


# ---- OBJ --------------------------------------------------------------------------------------------------------------------
def test_obj_round_trip_from_the_device(tmp_path):
    m, data, atlas = gpu_mesh("bumpy"), S.mesh("bumpy"), gpu_atlas("bumpy")
    texture = HN.bake_texture(m, atlas, lambda p, n: (0.5 + 0.5 * n).clamp(0.0, 1.0).contiguous())
    path = str(tmp_path / "bumpy.obj")
    HN.write_obj(path, m, atlas, texture)
    back = HN.read_obj(path)
    assert same_bits(back["vertices"], data["vertices"]) and same_bits(back["normals"], data["normals"])
    assert np.array_equal(back["faces"], data["faces"])
    uv = host(atlas["uv"])
    w, h = atlas["size"]
    assert np.abs(back["uv"].astype(np.float64) - uv).max() <= np.spacing(F32(max(w, h)))      # 1 ulp; exact here
    assert same_bits(back["uv"], uv)
    assert np.array_equal(back["texture"], host(texture))
    assert np.array_equal(inference.read_png(str(tmp_path / "bumpy.png")), host(texture))
    assert "map_Kd bumpy.png" in open(os.path.join(tmp_path, "bumpy.mtl")).read() and back["map_Kd"] == "bumpy.png"
    with pytest.raises(ValueError, match="uint8"):
        HN.write_obj(path, m, atlas, texture.float())
