"""Times the registration path (csrc/hn_registration.hip, geometry.register_mesh), one JSON line:

  python tools/registration_bench.py                       # the 128^3 torus, 10^5 and 10^6 samples
  python tools/registration_bench.py --res 64 --samples 20000 --runs 5

The target is the isosurface of the analytic torus of tools/mesh_distance_bench.py (178 952 faces at 128^3); the source is
`--samples` area-weighted samples of it, turned by 3 degrees about (1, 2, 3) and shifted by (0.01, -0.02, 0.015): what an
iteration of register_mesh sees.  Stages, each the median of `--runs` calls after `--warmup`, bracketed by device events
on the current stream:
  transform_ms       hn_reg_transform of the samples
  query_ms           ops.mesh.grid_query of the transformed samples (cell keys, sort, hn_md_query)
  threshold_ms       ops.registration.trim_threshold at trim 0.9 (torch.sort and a gather)
  moments_point_ms / moments_plane_ms    hn_reg_moments: the moments launch and the finishing launch, default block count
  torch_point_ms / torch_plane_ms        the baseline: the same sums as torch float64 operations on the device (masks in
                     place of branches, one matmul for J^T J); `*_rel_diff` is its largest relative difference from the kernel
  blocks             the moments pair at other block counts: the numbers behind the default
  register_ms        a whole register_mesh (method 'plane', trim 0.9) from the samples, host wall clock ending in a
                     synchronise, with its iterations and final rms.  A torus is symmetric about its axis: the spin about it
                     is free, so the figure of merit is the rms, not the recovered angle."""
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


def torch_moments(p, query, tri, tau, mode):
    """The sums of hn_reg_moments as torch float64 operations (the baseline, not the code under test)."""
    import torch
    d, face = query['distance'], query['face']
    inlier = torch.isfinite(d) & (d <= tau) & (face >= 0) & (face < tri.shape[0])
    p64, d64 = p.double(), torch.where(inlier, d, torch.zeros_like(d)).double()
    q64 = torch.where(inlier[:, None], query['closest'], torch.zeros_like(p)).double()
    if mode == 'point':
        w = inlier.double()
        pw = p64 * w[:, None]
        return torch.cat([w.sum().reshape(1), (d64 * d64).sum().reshape(1), pw.sum(0), q64.sum(0), (q64.T @ pw).reshape(9),
                          (pw * p64).sum().reshape(1), (q64 * q64).sum().reshape(1)])
    t = tri[torch.where(inlier, face, torch.zeros_like(face)).long()].double()
    m = torch.linalg.cross(t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3])
    length = m.norm(dim=1)
    inlier = inlier & (length > 0) & torch.isfinite(length)
    w = inlier.double()
    nrm = torch.where(inlier[:, None], m / length[:, None], torch.zeros_like(m))
    r = ((p64 - q64) * nrm).sum(1) * w
    jac = torch.cat([torch.linalg.cross(p64, nrm), nrm, (p64 * nrm).sum(1, keepdim=True)], 1)
    jtj = jac.T @ jac
    iu = torch.triu_indices(7, 7, device=p.device)
    return torch.cat([w.sum().reshape(1), (d64 * d64 * w).sum().reshape(1), (r * r).sum().reshape(1), jtj[iu[0], iu[1]], jac.T @ r])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--samples", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--blocks", type=int, nargs="*", default=[64, 128, 256, 512, 1024])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    sys.path[:0] = [ROOT]
    import numpy as np
    import torch
    from hypernerf_torch_amd import _lib as L
    from hypernerf_torch_amd import geometry as G
    from hypernerf_torch_amd.ops import mesh as M
    from hypernerf_torch_amd.ops import registration as R
    if not torch.cuda.is_available():
        raise SystemExit("registration_bench.py measures on the GPU; none is visible")
    target = G.extract_isosurface(torus_grid(a.res, DEV), 0.0, (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0))
    grid = G.build_distance_grid(target)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    rot, shift = R.rodrigues(axis * np.radians(3.0)), np.array([0.01, -0.02, 0.015])
    rows = []
    for n in a.samples:
        samples = R.transform_points(G.sample_surface(target, n, seed=1)['points'], 1.0, rot, shift)
        transform_ms, moved = event_ms(lambda: R.transform_points(samples, 1.0, np.eye(3), np.zeros(3)), a.warmup, a.runs)
        query_ms, query = event_ms(lambda: M.grid_query(moved, grid), a.warmup, a.runs)
        threshold_ms, tau = event_ms(lambda: R.trim_threshold(query['distance'], 0.9), a.warmup, a.runs)
        row = {"samples": n, "default_blocks": R.default_moment_blocks(n), "transform_ms": transform_ms, "query_ms": query_ms,
               "threshold_ms": threshold_ms, "blocks": []}
        for mode in ('point', 'plane'):
            ms, sums = event_ms(lambda: R.registration_moments(moved, query, grid['tri'], tau, mode), a.warmup, a.runs)
            base_ms, base = event_ms(lambda: torch_moments(moved, query, grid['tri'], tau, mode), a.warmup, a.runs)
            again = R.registration_moments(moved, query, grid['tri'], tau, mode)
            width = R.REG_POINT_SUMS if mode == 'point' else R.REG_SUMS
            scale = base.abs().clamp(min=1e-300)
            row.update({f"moments_{mode}_ms": ms, f"torch_{mode}_ms": base_ms, f"{mode}_speedup": base_ms / ms,
                        f"{mode}_rel_diff": float(((sums[:width] - base).abs() / scale).max()),
                        f"{mode}_same_bits": bool(torch.equal(sums.view(torch.int64), again.view(torch.int64))),
                        f"{mode}_inliers": int(sums[0])})
        for nb in a.blocks:
            entry = {"n_blocks": nb}
            for mode in ('point', 'plane'):
                entry[f"moments_{mode}_ms"] = event_ms(lambda: R.registration_moments(moved, query, grid['tri'], tau, mode, nb),
                                                       a.warmup, a.runs)[0]
            row["blocks"].append(entry)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = G.register_mesh(samples, grid, method='plane', trim=0.9)
        torch.cuda.synchronize()
        row.update({"register_ms": (time.perf_counter() - t0) * 1e3, "iterations": fit['iterations'], "converged": fit['converged'],
                    "rms_first": fit['history'][0]['rms'], "rms_last": fit['rms'], "inliers": fit['inliers']})
        row["register_ms_per_iteration"] = row["register_ms"] / fit['iterations']
        rows.append(row)
        del samples, moved, query
    print(json.dumps({"tool": "registration_bench", "warmup": a.warmup, "runs": a.runs, "build": L.build_id(),
                      "device": torch.cuda.get_device_name(0), "resolution": a.res, "faces": int(target['faces'].shape[0]),
                      "grid_resolution": list(grid['resolution']),
                      "workload": "analytic torus isosurface; source = its samples turned by 3 degrees and shifted", "results": rows}))


if __name__ == "__main__":
    main()
