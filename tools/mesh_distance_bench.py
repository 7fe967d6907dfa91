"""Times the mesh-distance path (csrc/hn_mesh_distance.hip, geometry.sample_surface / build_distance_grid /
point_mesh_distance / mesh_distance), one JSON line:

  python tools/mesh_distance_bench.py                      # the torus at 128^3 and 256^3, 10^6 samples
  python tools/mesh_distance_bench.py --res 64 --samples 100000 --runs 5

Per resolution the target is the isosurface of an analytic torus (the field of tools/mesh_render_bench.py: 178 952 faces
at 128^3, 720 560 at 256^3) and the queries are `--samples` area-weighted samples of `simplify_mesh(target, 2 lattice
spacings)` — the question the feature exists for: what did the simplification cost.  Stages, each the median of `--runs`
calls after `--warmup`, bracketed by device events on the current stream (a stage that reads the host includes the read):
  sample_ms        sample_surface of the simplified mesh: hn_md_face_weights, the integer cdf (torch), one host read, hn_md_sample
  grid_ms          build_distance_grid of the target at the default resolution: extent, pack, count, scan, host read, fill,
                   stable sort, searchsorted
  query_sorted_ms / query_unsorted_ms    point_mesh_distance against that grid with and without sorting the queries by cell
                   (the sort is inside the sorted figure); `same_bits` says the two gave equal bits
  sweep            grid_ms and query_sorted_ms at GRID_DENSITY x `--densities`: the numbers behind the default resolution
  mesh_distance_ms the whole two-sided call at `--samples` per side, host wall clock ending in a synchronise
Then at `--brute-res` (44^3: about 21 k faces) x `--brute-samples` queries the same query at grid_resolution=1 — every face
for every point, through the same kernel — beside the default grid: `speedup`, and `same_bits` again."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def torus_grid(n, device):
    import torch
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=device)
    x, y, z = torch.meshgrid(ax - 0.031, ax + 0.017, ax - 0.023, indexing="ij")
    return (0.23 - torch.sqrt((torch.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).float().contiguous()


def event_ms(fn, warmup, runs):
    """(median ms of `runs` calls after `warmup`, the last result): device events around each call."""
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), out


def same_bits(a, b):
    import torch
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ('distance', 'face', 'closest'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--densities", type=float, nargs="*", default=[0.25, 0.5, 1.0, 2.0, 4.0], help="multiples of GRID_DENSITY")
    ap.add_argument("--brute-res", type=int, default=44)
    ap.add_argument("--brute-samples", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    sys.path[:0] = [ROOT]
    import torch
    from hypernerf_torch_amd import _lib as L
    from hypernerf_torch_amd import geometry as G
    from hypernerf_torch_amd.ops import mesh as M
    if not torch.cuda.is_available():
        raise SystemExit("mesh_distance_bench.py measures on the GPU; none is visible")
    bounds = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)

    def meshes(res):
        target = G.extract_isosurface(torus_grid(res, DEV), 0.0, bounds)
        small = G.simplify_mesh(target, 2 * 2.0 / (res - 1), origin=(-1.0, -1.0, -1.0))
        return target, small

    rows = []
    for res in a.res:
        target, small = meshes(res)
        n_faces = int(target['faces'].shape[0])
        sample_ms, samples = event_ms(lambda: G.sample_surface(small, a.samples, seed=1), a.warmup, a.runs)
        pts = samples['points']
        grid_ms, grid = event_ms(lambda: G.build_distance_grid(target), a.warmup, a.runs)
        sorted_ms, out_s = event_ms(lambda: G.point_mesh_distance(pts, grid, sort_queries=True), a.warmup, a.runs)
        unsorted_ms, out_u = event_ms(lambda: G.point_mesh_distance(pts, grid, sort_queries=False), a.warmup, a.runs)
        row = {"resolution": res, "faces": n_faces, "vertices": int(target['vertices'].shape[0]),
               "query_mesh_faces": int(small['faces'].shape[0]), "samples": a.samples, "sample_ms": sample_ms,
               "grid_resolution": list(grid['resolution']), "pairs": int(grid['pair_face'].shape[0]), "grid_ms": grid_ms,
               "query_sorted_ms": sorted_ms, "query_unsorted_ms": unsorted_ms, "same_bits": same_bits(out_s, out_u),
               "distance_mean": float(out_s['distance'].double().mean()), "distance_max": float(out_s['distance'].max()),
               "queries_per_s_sorted": a.samples / sorted_ms * 1e3, "sweep": []}
        lo, hi = M.vertex_extent(target['vertices'])
        base = M.GRID_DENSITY
        for k in a.densities:
            M.GRID_DENSITY = base * k
            try:
                r = M.default_grid_resolution(n_faces, lo, hi)
            finally:
                M.GRID_DENSITY = base
            g_ms, g = event_ms(lambda: G.build_distance_grid(target, r), a.warmup, a.runs)
            q_ms, out_k = event_ms(lambda: G.point_mesh_distance(pts, g, sort_queries=True), a.warmup, a.runs)
            row["sweep"].append({"density": base * k, "grid_resolution": list(g['resolution']), "pairs": int(g['pair_face'].shape[0]),
                                 "grid_ms": g_ms, "query_sorted_ms": q_ms, "same_bits": same_bits(out_s, out_k)})
            del g, out_k
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = G.mesh_distance(target, small, n_samples=a.samples, seed=0, thresholds=[2.0 / (res - 1)])
        torch.cuda.synchronize()
        row["mesh_distance_ms"] = (time.perf_counter() - t0) * 1e3
        row["mesh_distance"] = {k: stats[k] for k in ('chamfer', 'hausdorff', 'a_to_b', 'b_to_a', 'thresholds')}
        rows.append(row)
        del target, small, grid, out_s, out_u, pts, samples
    target, small = meshes(a.brute_res)
    pts = G.sample_surface(small, a.brute_samples, seed=1)['points']
    grid, brute = G.build_distance_grid(target), G.build_distance_grid(target, 1)
    grid_q_ms, out_g = event_ms(lambda: G.point_mesh_distance(pts, grid), a.warmup, a.runs)
    brute_ms, out_b = event_ms(lambda: G.point_mesh_distance(pts, brute), 1, max(1, a.runs // 3))
    baseline = {"resolution": a.brute_res, "faces": int(target['faces'].shape[0]), "samples": a.brute_samples,
                "grid_resolution": list(grid['resolution']), "grid_query_ms": grid_q_ms, "brute_force_ms": brute_ms,
                "speedup": brute_ms / grid_q_ms, "same_bits": same_bits(out_g, out_b),
                "point_triangle_tests_per_s": a.brute_samples * int(target['faces'].shape[0]) / brute_ms * 1e3}
    print(json.dumps({"tool": "mesh_distance_bench", "warmup": a.warmup, "runs": a.runs, "build": L.build_id(),
                      "device": torch.cuda.get_device_name(0), "grid_density": M.GRID_DENSITY,
                      "workload": "analytic torus isosurface; queries = samples of simplify_mesh(target, 2 spacings)",
                      "results": rows, "brute_force_baseline": baseline}))


if __name__ == "__main__":
    main()
