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
reaches about 6.3)."""
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
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import hypernerf_torch_amd as HN
    from gpu_common import EMB, load_hash
    from hypernerf_torch_amd import _lib as L
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
        rows.append({"resolution": res, "points": n, "density_grid_ms": grid_ms, "points_per_s": n / grid_ms * 1e3,
                     "extract_isosurface_ms": iso_ms, "vertices": v, "faces": f, "iso": iso,
                     "isosurface_passes": passes, "density_grid_launches": query})
        del grid, mesh
    print(json.dumps({"tool": "mesh_bench", "precision": a.precision, "chunk": a.chunk, "repeats": a.repeats,
                      "hbm_tbs": a.hbm_tbs, "build": L.build_id(),
                      "workload": "NerfModel use_warp bendy_sheet nerf_embed+alpha_cond (config 2), fine level", "results": rows}))


if __name__ == "__main__":
    main()
