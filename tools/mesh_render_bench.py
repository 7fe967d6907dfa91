"""Times the mesh renderer (geometry.render_mesh, csrc/hn_mesh_render.hip) stage by stage, one JSON line:

  python tools/mesh_render_bench.py                      # the analytic torus at 128^3 and 256^3, 378 x 504 pixels
  python tools/mesh_render_bench.py --res 64 --wh 64 48

Per resolution the mesh is extract_isosurface of the analytic torus lattice; the camera looks at it from (0.1, -0.05, -3)
with the focal length at which it fills most of the image.  Every stage is bracketed by device events, `--repeats` runs
after `--warmup`, and the medians are reported in ms:
  project   hn_mesh_project: 12 V read, 12 V written
  bin       hn_mesh_bin_count, the scan, the host read of the pair count, hn_mesh_bin_fill (8 bytes written per pair)
  sort      the stable torch.sort of the pairs by tile, the tile bounds, the gather of the face ids
  trace     hn_mesh_trace: per tile its faces (48 bytes each) through LDS, every pixel against every face of its tile
  shade     hn_mesh_shade
`pairs` is the number of (tile, face) pairs, `faces_per_tile` its mean and maximum over the tiles, `off_surface_pixels` the
covered pixels whose hit point lies more than two lattice spacings from the analytic torus.  At the first resolution
`trace_brute_ms` is hn_mesh_trace with binning=False (every face at every pixel), `brute_differs_pixels` the pixels
whose face differs from the binned picture and `brute_off_surface_pixels` its own count of hits off the surface (the
fp32 edge test on near-degenerate faces).  `render_image_ms` is
inference.render_image of a default NerfModel (bench config 2's architecture, seeded weights, 64 + 64 samples) at the same
image size in the same run, for scale: what one frame of the field costs beside one frame of its mesh."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def torus_grid(n, device):
    import torch
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=device)
    x, y, z = torch.meshgrid(ax - 0.031, ax + 0.017, ax - 0.023, indexing="ij")
    return (0.23 - torch.sqrt((torch.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).float().contiguous()


def off_surface(rays, out, tol):
    """Covered pixels whose hit point o + depth * d lies further than `tol` from the analytic torus: hits the fp32 edge
    test reports for a near-degenerate face along the extension of its line (limits)."""
    import torch
    p = rays[:, 0:3].double() + out["depth"].double()[:, None] * rays[:, 3:6].double()
    x, y, z = p[:, 0] - 0.031, p[:, 1] + 0.017, p[:, 2] - 0.023
    dist = (0.23 - torch.sqrt((torch.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).abs()
    return int(((out["face"] >= 0) & (dist > tol)).sum())


def stage_times(stages, warmup, repeats):
    """{name: median ms} of a list of (name, thunk) run in order `warmup + repeats` times, device events around each."""
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
    return {name: sorted(v)[len(v) // 2] for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--wh", type=int, nargs=2, default=[378, 504], metavar=("W", "H"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--no-field", action="store_true", help="skip the render_image reference")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import hypernerf_torch_amd as HN
    from hypernerf_torch_amd import functional as F
    from hypernerf_torch_amd import inference
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_bench.py measures on the GPU; none is visible")
    w, h = a.wh
    bounds = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
    cam = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.05, -3.0, 1.6 * min(w, h), 1, 0, w / 2, h / 2, 0, 0, 0, 0, 0, 0, 0],
                       dtype=torch.float32, device=DEV)
    rays = F.generate_rays_nerfies(h, w, cam, 2.0, 4.5, image_id=7)
    n_tiles = ((w + F.MESH_TILE - 1) // F.MESH_TILE) * ((h + F.MESH_TILE - 1) // F.MESH_TILE)
    rows = []
    for k, res in enumerate(a.res):
        mesh = HN.extract_isosurface(torus_grid(res, DEV), 0.0, bounds)
        vertices, faces = mesh["vertices"], mesh["faces"]
        st = {}

        def project():
            st["pix"], st["vflags"] = F.mesh_project(vertices, cam)

        def bins():
            st["pairs"] = F.mesh_tile_pairs(vertices, faces, cam, (w, h), st["pix"], st["vflags"])

        def sort():
            st["begin"], st["end"], st["pair_face"] = F.group_tile_pairs(st["pairs"][0], st["pairs"][1], n_tiles)

        out = {"face": torch.empty(h * w, dtype=torch.int32, device=DEV), "depth": torch.empty(h * w, device=DEV),
               "bary": torch.empty((h * w, 3), device=DEV)}

        def trace(begin=None, end=None, pair_face=None):
            begin, end, pair_face = (st["begin"], st["end"], st["pair_face"]) if begin is None else (begin, end, pair_face)
            F.L.launch("hn_mesh_trace", F.L.ptr(vertices), vertices.shape[0], F.L.ptr(faces), faces.shape[0], F.L.ptr(rays),
                       rays.shape[1], h, w, F.L.ptr(begin), F.L.ptr(end), F.L.ptr(pair_face), pair_face.shape[0],
                       F.L.ptr(out["face"]), F.L.ptr(out["depth"]), F.L.ptr(out["bary"]), F.L.stream_handle())

        def shade():
            st["img"] = F.mesh_shade(vertices, faces, mesh["normals"], None, rays, out["face"], out["bary"])

        ms = stage_times([("project", project), ("bin", bins), ("sort", sort), ("trace", trace), ("shade", shade)],
                         a.warmup, a.repeats)
        per_tile = (st["end"] - st["begin"]).double()
        row = {"resolution": res, "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]),
               "pairs": int(st["pair_face"].shape[0]), "tiles": n_tiles,
               "faces_per_tile": {"mean": float(per_tile.mean()), "max": int(per_tile.max())},
               "covered_pixels": int((out["face"] >= 0).sum()),
               "ms": ms, "total_ms": sum(ms.values())}
        whole = HN.render_mesh(mesh, rays, cam, (w, h))
        assert torch.equal(whole["face"].view(-1), out["face"]) and torch.equal(whole["rgb8"], st["img"]["rgb8"].view(h, w, 3))
        row["off_surface_pixels"] = off_surface(rays, out, 2.0 * 2.0 / (res - 1))
        if k == 0:
            begin, end, every = F.mesh_bins(vertices, faces, cam, (w, h), binning=False)
            binned_face = out["face"].clone()
            row["trace_brute_ms"] = stage_times([("trace", lambda: trace(begin, end, every))], 1, 3)["trace"]
            row["brute_differs_pixels"] = int((binned_face != out["face"]).sum())
            row["brute_off_surface_pixels"] = off_surface(rays, out, 2.0 * 2.0 / (res - 1))
        rows.append(row)
    result = {"image_wh": [w, h], "repeats": a.repeats, "warmup": a.warmup, "meshes": rows, "build": F.L.build_id()}
    if not a.no_field:
        from gpu_common import EMB, load_hash
        from hypernerf_torch_amd.hypernerf.models import NerfModel
        HN.set_precision(a.precision)
        m = NerfModel(EMB, n_samples_coarse=64, n_samples_fine=64, noise_std=None, view_fourier_dim=6,
                      hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True)
        load_hash(m, 3)
        m = m.to(DEV).eval()
        m.use_stratified_sampling = False
        result["render_image_ms"] = stage_times([("field", lambda: inference.render_image(m, rays))], 2, 5)["field"]
        result["precision"] = a.precision
    print(json.dumps(result))


if __name__ == "__main__":
    main()
