"""Times the geometry path on a model of bench config 2's architecture (bendy sheet, warp, GLO conditions; untrained,
seeded weights), one JSON line:

  python tools/mesh_bench.py                       # 128^3 and 256^3, bf16
  python tools/mesh_bench.py --res 64 --precision fp32

Per resolution: `density_grid` (a chunk loop of hn_grid_points -> the fused level program -> hn_density_activate) and
`extract_isosurface` at the median density (an untrained field is noise: far more surface than a trained scene has, so
the vertex / face terms are on the heavy side), each as host wall clock around `--repeats` calls that end in a device
synchronise, after one warm-up call; then one more call with every launch bracketed by device events, which gives the
time per pass.  `bytes` is what each isosurface pass must move (N lattice points, V vertices, F faces):
  hn_iso_mark       4 N read (grid) + 1 N written (marks)
  hn_iso_vertices   1 N read + 28 N written (edge slots) + 24 V written (positions, normals)
  hn_iso_faces      count: 4 N read;  emit: 4 N read + 12 F gathered from the slots + 12 F written
and `floor_ms` is those bytes over the HBM rate given with --hbm-tbs (default 8.0, the MI355X's HBM3E peak; a float4 copy
reaches about 6.3).

Then, on that mesh, the post-processing stages, timed the same way (V' / F' = what keep_largest=1 leaves, R = rounds):
  mesh_components   hn_cc_init 12 F read + 4 V written; per round hook 12 F read + 12 F of parents gathered, jump 4 V
                    read + 4 V gathered: 12 F + 4 V + R (24 F + 8 V); `rounds` counts the last one, which changes nothing
  component_sizes   12 F read + 4 F of labels gathered + 4 V zeroed
  filter_mesh(keep_largest=1), whole call (labelling and sizes included) and, as `filter_rest`, what it adds to them:
                    keep 4 V + 12 F read, 4 V + 4 F written; two scans 8 V + 8 F; compact 4 V + 16 F read, 4 V' + 12 F'
                    written, 12 F' gathered; vertices and normals 2 x (12 V' gathered + 12 V' written)
  vertex_colors(view='normal')   12 V normals + 12 V positions read, 3 V of uint8 written (the directions and the float
                    colours live one chunk at a time); its time is the level program's, so `points_per_s` is the figure to
                    hold against density_grid's.

Then `simplify_mesh` on the unfiltered mesh with cells of --simplify (default 2 and 4) lattice spacings from the lower
bounds, beside `extract_isosurface_ms` of the same grid.  `total_ms` is the whole call (four host reads); the stages are
timed on their own the same way: `extent_ms` (vertex_extent: hn_simplify_extent, a reduction of its partials and
the host read), `keys_ms` (the hn_simplify_keys launch, device events), `sort_ms` (the rest of
cluster_vertices: torch's stable sort of V int64 keys, run lengths, the inverse), `reduce_ms` (hn_simplify_reduce, one
work-item per cluster), `faces_ms` (cluster_faces: three launches, `faces_kernels_ms`, and two stable sorts over F names
plus a scan, `faces_sorts_ms`) and `rest_ms` (compaction, gathers, relabelling, two host reads)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats * 1e3, out


def per_launch(fn):
    """{launch name: summed ms} of one call, from device events around every launch."""
    from hypernerf_torch_amd import _lib as L
    L.KERNEL_TIMES = {}
    try:
        fn()
        times = L.collect_kernel_times()
    finally:
        L.KERNEL_TIMES = None
    return {k: {"launches": len(v), "ms": sum(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--simplify", type=float, nargs="*", default=[2.0, 4.0], help="cell sizes in lattice spacings")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import hypernerf_torch_amd as HN
    from gpu_common import EMB, load_hash
    from hypernerf_torch_amd import _lib as L
    from hypernerf_torch_amd import functional as FN
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench.py measures on the GPU; none is visible")
    HN.set_precision(a.precision)
    m = NerfModel(EMB, n_samples_coarse=64, n_samples_fine=64, noise_std=1.0, view_fourier_dim=6,
                  hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True)
    load_hash(m, 3)
    m = m.to(DEV)
    bounds = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
    rows = []
    for res in a.res:
        n = res ** 3
        grid_ms, grid = timed(lambda: HN.density_grid(m, bounds, res, 7, chunk=a.chunk), a.repeats)
        iso = float(grid.median())
        iso_ms, mesh = timed(lambda: HN.extract_isosurface(grid, iso, bounds), a.repeats)
        v, f = int(mesh["vertices"].shape[0]), int(mesh["faces"].shape[0])
        passes = per_launch(lambda: HN.extract_isosurface(grid, iso, bounds))
        query = per_launch(lambda: HN.density_grid(m, bounds, res, 7, chunk=a.chunk))
        need = {"hn_iso_mark": 5 * n, "hn_iso_vertices": 29 * n + 24 * v, "hn_iso_faces": 8 * n + 24 * f}
        for name, b in need.items():
            if name in passes:
                passes[name]["bytes"] = b
                passes[name]["floor_ms"] = b / (a.hbm_tbs * 1e12) * 1e3
        row = {"resolution": res, "points": n, "density_grid_ms": grid_ms, "points_per_s": n / grid_ms * 1e3,
               "extract_isosurface_ms": iso_ms, "vertices": v, "faces": f, "iso": iso,
               "isosurface_passes": passes, "density_grid_launches": query}
        del grid
        floor = lambda b: b / (a.hbm_tbs * 1e12) * 1e3
        label_ms, (labels, rounds) = timed(lambda: FN.mesh_components(mesh["faces"], v, return_rounds=True), a.repeats)
        sizes_ms, sizes = timed(lambda: HN.component_sizes(labels, mesh["faces"]), a.repeats)
        filter_ms, kept = timed(lambda: HN.filter_mesh(mesh, keep_largest=1), a.repeats)
        v1, f1 = int(kept["vertices"].shape[0]), int(kept["faces"].shape[0])
        stages = per_launch(lambda: HN.filter_mesh(mesh, keep_largest=1))
        label_b = 12 * f + 4 * v + rounds * (24 * f + 8 * v)
        sizes_b = 16 * f + 4 * v
        rest_b = (8 * v + 16 * f) + 8 * (v + f) + (4 * v + 16 * f + 4 * v1 + 24 * f1) + 48 * v1
        row["mesh_components"] = {"ms": label_ms, "rounds": rounds, "cap": v + 1, "bytes": label_b, "floor_ms": floor(label_b),
                                  "components": int((sizes > 0).sum())}
        row["component_sizes"] = {"ms": sizes_ms, "bytes": sizes_b, "floor_ms": floor(sizes_b)}
        row["filter_mesh_keep_largest_1"] = {"ms": filter_ms, "vertices": v1, "faces": f1, "launches": stages,
                                             "filter_rest": {"ms": filter_ms - label_ms - sizes_ms, "bytes": rest_b,
                                                             "floor_ms": floor(rest_b)},
                                             "fraction_of_density_grid": filter_ms / grid_ms}
        del kept, labels, sizes
        color_ms, colors = timed(lambda: HN.vertex_colors(m, mesh["vertices"], mesh["normals"], 7, chunk=a.chunk), a.repeats)
        color_b = 27 * v
        row["vertex_colors_normal"] = {"ms": color_ms, "points_per_s": v / color_ms * 1e3, "bytes": color_b,
                                       "floor_ms": floor(color_b),
                                       "launches": per_launch(lambda: HN.vertex_colors(m, mesh["vertices"], mesh["normals"], 7,
                                                                                       chunk=a.chunk))}
        del colors
        row["simplify_mesh"] = []
        origin = (bounds[0], bounds[2], bounds[4])
        for k in a.simplify:
            cell = k * (bounds[1] - bounds[0]) / (res - 1)
            total_ms, small = timed(lambda: HN.simplify_mesh(mesh, cell, origin), a.repeats)
            extent_ms, _ = timed(lambda: FN.vertex_extent(mesh["vertices"]), a.repeats)
            cluster_ms, clusters = timed(lambda: FN.cluster_vertices(mesh["vertices"], cell, origin), a.repeats)
            n_clusters = int(clusters["cluster_keys"].shape[0])
            reduce_ms, _ = timed(lambda: FN.reduce_clusters(mesh["vertices"], mesh["normals"], None, clusters, cell, origin),
                                 a.repeats)
            faces_ms, _ = timed(lambda: FN.cluster_faces(mesh["faces"], clusters["vertex_cluster"], n_clusters), a.repeats)
            launches = per_launch(lambda: HN.simplify_mesh(mesh, cell, origin))
            keys_ms = launches["hn_simplify_keys"]["ms"]
            face_kernels = sum(launches.get(n, {"ms": 0.0})["ms"] for n in
                               ("hn_simplify_face_keys", "hn_simplify_face_net", "hn_simplify_face_emit"))
            row["simplify_mesh"].append({
                "k": k, "cell": cell, "total_ms": total_ms, "extent_ms": extent_ms, "keys_ms": keys_ms, "sort_ms": cluster_ms - keys_ms,
                "reduce_ms": reduce_ms, "faces_ms": faces_ms, "faces_kernels_ms": face_kernels,
                "faces_sorts_ms": faces_ms - face_kernels,
                "rest_ms": total_ms - extent_ms - cluster_ms - reduce_ms - faces_ms, "clusters": n_clusters,
                "members_mean": v / max(n_clusters, 1), "vertices": int(small["vertices"].shape[0]),
                "faces": int(small["faces"].shape[0]), "fraction_of_extract_isosurface": total_ms / iso_ms,
                "launches": launches})
            del small, clusters
        rows.append(row)
        del mesh
    print(json.dumps({"tool": "mesh_bench", "precision": a.precision, "chunk": a.chunk, "repeats": a.repeats,
                      "hbm_tbs": a.hbm_tbs, "build": L.build_id(),
                      "workload": "NerfModel use_warp bendy_sheet nerf_embed+alpha_cond (config 2), fine level", "results": rows}))


if __name__ == "__main__":
    main()
