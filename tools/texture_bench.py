"""Times the texture atlas (geometry.texture_atlas / rasterize_atlas / bake_texture / render_textured_mesh,
csrc/hn_texture.hip) stage by stage, one JSON line:

  python tools/texture_bench.py                      # analytic spheres at 128^3 and 256^3, a 4096^2 atlas, 378 x 504 pixels
  python tools/texture_bench.py --res 32 --size 512 --wh 64 48
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/texture_bench.py --shade-only      # the two shaders' kernel times

Per resolution the mesh is extract_isosurface of an analytic sphere lattice and the texel length is
atlas_texel_for_size(mesh, --size) — with --size doubled until F / 2 cells of 16 x 16 texels fit, since a face never gets
less than half a 16-texel cell.  Every stage is bracketed by device events, `--repeats` runs after `--warmup`; the
medians and the (min, max) spread are reported in ms:
  classify   hn_tex_classify, the class histogram and its host read (ops.texture.face_classes)
  layout     the sort of the keys and hn_tex_layout (ops.texture.atlas_layout)
  rasterize  hn_tex_rasterize: 28 bytes written per texel
  scatter    the owned texels' index (torch.nonzero), a gather of their points and normals, the uint8 conversion and the
             indexed store of bake_texture, with a colour function that costs nothing (the normal as a colour)
  tex_shade  hn_tex_shade on the traced image (bilinear, uint8 texture)
  mesh_shade hn_mesh_shade on the same image, for scale: both are one pass over the pixels
`texel_search_ms` is atlas_texel_for_size (host clock around it, it ends in host reads).  With --field the field-query
share of bake_field_texture is stated on its own: `field_bake_ms` for the whole bake of a default NerfModel (bench config
2's architecture, seeded weights) and `field_query_ms` for vertex_colors alone on the same owned texels."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def sphere_grid(n, device):
    import torch
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=device)
    x, y, z = torch.meshgrid(ax - 0.031, ax + 0.017, ax - 0.023, indexing="ij")
    return (0.7 - torch.sqrt(x * x + y * y + z * z)).float().contiguous()


def stage_times(stages, warmup, repeats):
    """{name: {'median', 'min', 'max'} ms} of a list of (name, thunk) run in order `warmup + repeats` times."""
    import torch
    times = {name: [] for name, _ in stages}
    for it in range(warmup + repeats):
        marks = []
        for name, fn in stages:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks.append((name, e0, e1))
        torch.cuda.synchronize()
        if it >= warmup:
            for name, e0, e1 in marks:
                times[name].append(e0.elapsed_time(e1))
    return {name: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--wh", type=int, nargs=2, default=[378, 504], metavar=("W", "H"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--shade-only", action="store_true", help="the first mesh's two shaders only (for a profiler run)")
    ap.add_argument("--field", action="store_true", help="also time bake_field_texture and its field query")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import hypernerf_torch_amd as HN
    from hypernerf_torch_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("texture_bench.py measures on the GPU; none is visible")
    w, h = a.wh
    bounds = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
    cam = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.05, -3.0, 1.6 * min(w, h), 1, 0, w / 2, h / 2, 0, 0, 0, 0, 0, 0, 0],
                       dtype=torch.float32, device=DEV)
    rays = F.generate_rays_nerfies(h, w, cam, 2.0, 4.5, image_id=7)
    rows = []
    for res in a.res[:1] if a.shade_only else a.res:
        mesh = HN.extract_isosurface(sphere_grid(res, DEV), 0.0, bounds)
        vertices, faces, normals = mesh["vertices"], mesh["faces"], mesh["normals"]
        size = a.size          # F faces need at least F / 2 cells of 16 x 16: a mesh too large for --size gets the next power
        while size < 16384 and 128 * faces.shape[0] > size * size:
            size *= 2
        t0 = time.perf_counter()
        texel = HN.atlas_texel_for_size(mesh, size)
        search_ms = (time.perf_counter() - t0) * 1e3
        atlas = HN.texture_atlas(mesh, texel, max_size=size)
        st = {"rast": HN.rasterize_atlas(mesh, atlas)}
        texture = HN.bake_texture(mesh, atlas, lambda p, n: (0.5 + 0.5 * n).clamp(0.0, 1.0))
        traced = F.mesh_trace(vertices, faces, rays, cam, (w, h))

        def classify():
            st["cls"] = F.face_classes(vertices, faces, texel, 16, 256, "texture_bench")

        def layout():
            F.atlas_layout(st["cls"][1], st["cls"][2], 16)

        def rasterize():
            st["rast"] = F.atlas_rasterize(vertices, faces, normals, atlas)

        def scatter():
            r = st["rast"]
            index = torch.nonzero(r["owner"].view(-1) >= 0).view(-1)
            out = torch.full((atlas["size"][1], atlas["size"][0], 3), 0, dtype=torch.uint8, device=DEV)
            r["position"].view(-1, 3)[index]
            out.view(-1, 3)[index] = (r["normal"].view(-1, 3)[index] * 255).to(torch.uint8)

        def tex_shade():
            F.texture_shade(vertices, faces, normals, atlas, texture, rays, traced["face"], traced["bary"])

        def mesh_shade():
            F.mesh_shade(vertices, faces, normals, None, rays, traced["face"], traced["bary"])

        shaders = [("tex_shade", tex_shade), ("mesh_shade", mesh_shade)]
        ms = stage_times(shaders if a.shade_only else
                         [("classify", classify), ("layout", layout), ("rasterize", rasterize), ("scatter", scatter)] + shaders,
                         a.warmup, a.repeats)
        owner = st["rast"]["owner"]
        row = {"resolution": res, "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "texel": texel,
               "atlas_wh": list(atlas["size"]), "cells": int(atlas["cell_side"].shape[0]),
               "cell_sides": {int(s): int(n) for s, n in zip(*torch.unique(atlas["cell_side"], return_counts=True))},
               "owned_texels": int((owner >= 0).sum()), "owned_share": float((owner >= 0).double().mean()),
               "covered_pixels": int((traced["face"] >= 0).sum()), "texel_search_ms": search_ms, "ms": ms}
        if a.field and not a.shade_only:
            from gpu_common import EMB, load_hash
            from hypernerf_torch_amd.hypernerf.models import NerfModel
            m = NerfModel(EMB, n_samples_coarse=64, n_samples_fine=64, noise_std=None, view_fourier_dim=6,
                          hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True)
            load_hash(m, 3)
            m = m.to(DEV).eval()
            keep = owner.view(-1) >= 0
            points, nrm = st["rast"]["position"].view(-1, 3)[keep], st["rast"]["normal"].view(-1, 3)[keep]
            field = stage_times([("field_bake", lambda: HN.bake_field_texture(m, mesh, atlas, 12)),
                                 ("field_query", lambda: HN.vertex_colors(m, points, nrm, 12, dtype=torch.float32))], 1, 3)
            row["field_bake_ms"], row["field_query_ms"] = field["field_bake"], field["field_query"]
        rows.append(row)
    print(json.dumps({"image_wh": [w, h], "atlas_size": a.size, "repeats": a.repeats, "warmup": a.warmup, "meshes": rows,
                      "build": F.L.build_id()}))


if __name__ == "__main__":
    main()
