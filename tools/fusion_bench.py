"""Times depth fusion (csrc/hn_fusion.hip) on a synthetic scene, one JSON line:

  python tools/fusion_bench.py                     # lattices 128^3 and 256^3, 60 orbit views of 378 x 504
  python tools/fusion_bench.py --res 64 --views 24 --image 96 128

The scene: a sphere of radius 0.5 at the origin inside bounds +-0.8, `--views` orbit cameras at radius 3 and 20 degrees of
elevation whose image holds the bounds; every depth image is the exact distance along the GPU's own rays
(geometry.camera_rays) to the sphere, +inf on a miss — so every voxel-view projects, reads its pixel and updates.

Per lattice, each as host wall clock around `--repeats` calls that end in a device synchronise, after one warm-up call,
and once more with every launch bracketed by device events (`launches`):
  integrate_ms         ops.mesh.tsdf_integrate of all views in one launch (hn_tsdf_integrate; a wave owns a 4 x 4 x 4 brick
                       of lattice points), with `voxel_views_per_s` = N * views / time.  `bytes` is what the launch must
                       move — 8 N read and 8 N written for the two volumes, plus the depth stack once, 4 * views * H * W —
                       and `floor_ms` those bytes over the HBM rate given with --hbm-tbs (default 8.0, the MI355X's peak).
                       The launch is bound by its arithmetic (a projection, three divisions and a root per voxel-view),
                       not by those bytes: `floor_ms` says how far.
  tsdf_isosurface_ms   geometry.tsdf_isosurface (the lattice -tsdf / +1, extract_isosurface, the face filter, two scans,
                       the compaction and two gathers; three host reads), beside `extract_isosurface_ms` of the same
                       lattice alone.
  face_keep_ms         ops.mesh.tsdf_face_keep on the unfiltered mesh: 12 F read, 36 F of vertices and 32 F of weights
                       gathered, 4 F + 4 V written."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BOUNDS = (-0.8, 0.8, -0.8, 0.8, -0.8, 0.8)
RADIUS = 0.5


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


def sphere_depths(cams, wh):
    """(N, H, W) fp32 on the GPU: the distance along each camera's own rays to the sphere, +inf on a miss."""
    import torch
    import hypernerf_torch_amd as HN
    w, h = wh
    out = torch.empty((len(cams), h, w), dtype=torch.float32, device=DEV)
    for n, rec in enumerate(cams):
        rays = HN.camera_rays(torch.from_numpy(rec).to(DEV), w, h, 0.0, 6.0).double()
        o, d = rays[:, 0:3], rays[:, 3:6]
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - RADIUS * RADIUS)
        t = -b - torch.sqrt(disc.clamp_min(0.0))
        out[n] = torch.where((disc >= 0) & (t > 0), t, torch.full_like(t, float("inf"))).float().view(h, w)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--views", type=int, default=60)
    ap.add_argument("--image", type=int, nargs=2, default=[378, 504], metavar=("W", "H"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import hypernerf_torch_amd as HN
    from hypernerf_torch_amd import _lib as L
    from hypernerf_torch_amd import functional as FN
    if not torch.cuda.is_available():
        raise SystemExit("fusion_bench.py measures on the GPU; none is visible")
    wh = tuple(a.image)
    half = 0.8 * np.sqrt(3.0)
    focal = 0.45 * min(wh) * np.sqrt(9.0 - half * half) / half
    cams = HN.orbit_cameras((0.0, 0.0, 0.0), 3.0, a.views, 20.0, focal=focal, image_wh=wh)
    depths = sphere_depths(cams, wh)
    cams_dev = torch.from_numpy(cams).to(DEV)
    floor = lambda b: b / (a.hbm_tbs * 1e12) * 1e3
    rows = []
    for res in a.res:
        n = res ** 3
        shape = (res, res, res)
        trunc = 4.0 * 1.6 / (res - 1)
        tsdf, weight = (torch.zeros(shape, dtype=torch.float32, device=DEV) for _ in range(2))
        integrate = lambda: FN.tsdf_integrate(tsdf, weight, BOUNDS, cams_dev, depths, trunc)
        integrate_ms, _ = timed(integrate, a.repeats)
        launches = per_launch(integrate)
        need = 16 * n + 4 * depths.numel()
        volume = HN.fuse_depth(depths, cams_dev, BOUNDS, res)
        del tsdf, weight
        lattice = torch.where(volume['weight'] > 0, -volume['tsdf'], torch.ones_like(volume['tsdf']))
        iso_ms, raw = timed(lambda: HN.extract_isosurface(lattice, 0.0, BOUNDS), a.repeats)
        del lattice
        tsdf_iso_ms, mesh = timed(lambda: HN.tsdf_isosurface(volume, BOUNDS), a.repeats)
        keep = lambda: FN.tsdf_face_keep(raw['vertices'], raw['faces'], volume['weight'], BOUNDS)
        keep_ms, _ = timed(keep, a.repeats)
        v, f = int(raw['vertices'].shape[0]), int(raw['faces'].shape[0])
        keep_b = 84 * f + 4 * v
        radial = (mesh['vertices'].double().norm(dim=1) - RADIUS).abs().max().item() / (1.6 / (res - 1))
        rows.append({"resolution": res, "points": n, "views": a.views, "trunc": trunc, "mapping": "brick 4x4x4 per wave",
                     "integrate_ms": integrate_ms, "voxel_views_per_s": n * a.views / integrate_ms * 1e3,
                     "integrate": {"launches": launches, "bytes": need, "floor_ms": floor(need)},
                     "observed_fraction": float((volume['weight'] > 0).float().mean()),
                     "extract_isosurface_ms": iso_ms, "tsdf_isosurface_ms": tsdf_iso_ms,
                     "tsdf_isosurface_launches": per_launch(lambda: HN.tsdf_isosurface(volume, BOUNDS)),
                     "face_keep_ms": keep_ms, "face_keep": {"launches": per_launch(keep), "bytes": keep_b, "floor_ms": floor(keep_b)},
                     "vertices": v, "faces": f, "kept_vertices": int(mesh['vertices'].shape[0]),
                     "kept_faces": int(mesh['faces'].shape[0]), "max_radial_error_spacings": radial})
        del volume, raw, mesh
    print(json.dumps({"tool": "fusion_bench", "image_wh": list(wh), "repeats": a.repeats, "hbm_tbs": a.hbm_tbs,
                      "build": L.build_id(), "workload": "sphere r 0.5 in bounds +-0.8, orbit cameras at radius 3",
                      "results": rows}))


if __name__ == "__main__":
    main()
