"""Times empty-space skipping (csrc/hn_occupancy.hip), one JSON line:

  python tools/occupancy_bench.py                          # kernels at 64^3 and 128^3, 378 x 504 rays; the image overhead
  python tools/occupancy_bench.py --train-steps 800        # + quality and speed on a briefly trained field
  python tools/occupancy_bench.py --parent-inference FILE  # + another commit's inference.py, timed in alternation

`kernels`: per lattice the host wall clock around `--repeats` calls that end in a device synchronise, after a warm-up
call, of occupancy_mark, one occupancy_dilate, occupancy_count and clip_rays for the rays of one 378 x 504 orbit camera at
radius 3; the density is a ball of radius 0.5 in bounds +-0.8 (as tools/fusion_bench.py's scene), so most rays walk the whole
grid.  `bytes` is what each launch must move and `floor_ms` those bytes over the HBM rate given with --hbm-tbs.

`overhead`: inference.render_image of that image with tools/eval_bench.py's model (64 + 64 samples, bf16, untrained),
without an occupancy and with an all-occupied grid whose box holds every ray's [near, far] — nothing is clipped (b = 1,
a = 0), the pixels are the same bits, and the difference is the cost of the feature's plumbing: one clip launch, the view
directions as a separate source, the weights' sum and two multiply-adds per ray.  The variants alternate; the median of
`--image-reps` runs each is reported.

`trained` (--train-steps N > 0): the synthetic Blender scene of tests/blender_scene.py at 128 x 128, N steps of 4096 rays,
then the val split rendered plain, clipped at both ends and clipped in front only (clip_far=False), each at the model's
sample counts and at half of them, and plain / clipped without the sample at infinity — with the PSNR and SSIM against
ground truth (inference.evaluate_images) and images/s (render_image alone).  The scene's images are not views of one
object, so the PSNR is low; what matters is how it moves between the cases."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
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


def alternate(variants, reps):
    """{name: [ms, ...]} of `reps` rounds over the variants in turn, each call ended by a device synchronise."""
    import torch
    times = {name: [] for name in variants}
    for name, fn in variants.items():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def kernels(a):
    import numpy as np
    import torch
    import hypernerf_torch_amd as HN
    from hypernerf_torch_amd import functional as FN
    w, h = a.image
    half = 0.8 * np.sqrt(3.0)
    focal = 0.45 * min(w, h) * np.sqrt(9.0 - half * half) / half
    cam = HN.orbit_cameras((0.0, 0.0, 0.0), 3.0, 1, 20.0, focal=focal, image_wh=(w, h))[0]
    rays = HN.camera_rays(torch.from_numpy(cam).to(DEV), w, h, 0.5, 6.0)
    n = rays.shape[0]
    floor = lambda b: b / (a.hbm_tbs * 1e12) * 1e3
    rows = []
    for res in a.res:
        axis = torch.linspace(BOUNDS[0], BOUNDS[1], res, device=DEV)
        r2 = axis[:, None, None] ** 2 + axis[None, :, None] ** 2 + axis[None, None, :] ** 2
        grid = torch.where(r2 <= RADIUS ** 2, 10.0, 0.0).contiguous()
        cells = (res - 1,) * 3
        mark_ms, bits = timed(lambda: FN.occupancy_mark(grid, 5.0), a.repeats)
        dilate_ms, grown = timed(lambda: FN.occupancy_dilate(bits, cells, 1), a.repeats)
        count_ms, count = timed(lambda: FN.occupancy_count(grown), a.repeats)
        occ = {'bits': grown, 'cells': cells, 'bounds': BOUNDS}
        clip_ms, clip = timed(lambda: HN.clip_rays(rays, occ, 0.5, 6.0), a.repeats)
        everything = {'bits': torch.full_like(grown, -1), 'cells': cells, 'bounds': BOUNDS}
        if cells[2] % 64:
            everything['bits'][:, :, -1] = (1 << (cells[2] % 64)) - 1
        clip_all_ms, _ = timed(lambda: HN.clip_rays(rays, everything, 0.5, 6.0), a.repeats)
        words = bits.numel()
        rows.append({"resolution": res, "cells": list(cells), "words": words, "rays": n,
                     "occupied_fraction": int(count) / float(np.prod(cells)), "hit_fraction": float(clip['hit'].float().mean()),
                     "mark_ms": mark_ms, "mark": {"bytes": 4 * res ** 3 + 8 * words, "floor_ms": floor(4 * res ** 3 + 8 * words)},
                     "dilate_ms": dilate_ms, "dilate": {"bytes": 16 * words, "floor_ms": floor(16 * words)},
                     "count_ms": count_ms, "clip_ms": clip_ms, "clip_all_occupied_ms": clip_all_ms,
                     "clip": {"bytes": n * (2 * 4 * rays.shape[1] + 8 + 1 + 8), "floor_ms": floor(n * (8 * rays.shape[1] + 17))},
                     "lattice_queries_over_image_samples": res ** 3 / float(n * (64 + 128))})
    return rows


def eval_model():
    import torch
    import hypernerf_torch_amd as HN
    from hypernerf_torch_amd.hypernerf import models
    HN.set_precision("bf16")
    emb = {k: list(range(100)) for k in ("warp", "appearance", "time")}
    emb["camera"] = [0]
    torch.manual_seed(0)
    m = models.NerfModel(emb, n_samples_coarse=64, n_samples_fine=64, hyper_slice_method="bendy_sheet",
                         use_nerf_embed=True, use_alpha_cond=True).to(DEV)
    m.eval()
    m.use_stratified_sampling = False
    return m


def overhead(a):
    import torch
    from hypernerf_torch_amd import inference
    w, h = a.image
    n = w * h
    m = eval_model()
    g = torch.Generator().manual_seed(1)
    o = torch.rand(n, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.zeros(n, 1), torch.ones(n, 1), torch.full((n, 1), 7.0)], dim=1).to(DEV)
    cells = (127, 127, 127)
    occ = {'bits': torch.full((127, 127, 2), -1, dtype=torch.int64, device=DEV), 'cells': cells, 'bounds': (-3.0, 3.0) * 3}
    occ['bits'][:, :, 1] = (1 << 63) - 1
    variants = {"plain": lambda: inference.render_image(m, rays, chunk=a.chunk),
                "identity_grid": lambda: inference.render_image(m, rays, chunk=a.chunk, occupancy=occ)}
    if a.parent_inference:
        spec = importlib.util.spec_from_file_location("hypernerf_torch_amd.inference_of_parent", a.parent_inference)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        variants["parent_commit"] = lambda: parent.render_image(m, rays, chunk=a.chunk)
    same = all(torch.equal(variants["plain"]()[k], variants["identity_grid"]()[k]) for k in ('rgb', 'depth', 'acc'))
    times = alternate(variants, a.image_reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med.get("parent_commit", med["plain"])
    return {"what": f"render_image, one {w}x{h} image, 64+64 samples, bf16, chunk {a.chunk}", "bit_identical": bool(same),
            "median_ms": med, "min_ms": {k: min(v) for k, v in times.items()}, "all_ms": times,
            "overhead_of_identity_grid": med["identity_grid"] / base - 1.0,
            "plain_over_parent": (med["plain"] / med["parent_commit"] - 1.0) if "parent_commit" in med else None}


def trained(a):
    import torch
    import hypernerf_torch_amd as HN
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from blender_scene import make_scene, write_scene
    from hypernerf_torch_amd import inference
    from hypernerf_torch_amd.datasets import BlenderDataset
    from hypernerf_torch_amd.hypernerf import models
    from hypernerf_torch_amd.training import TrainStep
    size, batch, nc, nf = 128, 4096, 64, 64
    HN.set_precision("bf16")
    emb = {k: list(range(100)) for k in ("warp", "appearance", "time")}
    emb["camera"] = [0]
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        root = write_scene(os.path.join(tmp, "scene"), make_scene(seed=23, size=size))
        train = BlenderDataset(root, split="train", img_wh=(size, size))
        val = BlenderDataset(root, split="val", img_wh=(size, size))
        samples = [val[i] for i in range(len(val))]
    m = models.NerfModel(emb, near=train.near, far=train.far, n_samples_coarse=nc, n_samples_fine=nf,
                         hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True).to(DEV)
    m.use_white_background = True
    ts = TrainStep(m, lr=5e-4)
    g = torch.Generator(device=DEV).manual_seed(3)
    t0 = time.perf_counter()
    for _ in range(a.train_steps):
        idx = torch.randint(0, train.all_rays.shape[0], (batch,), generator=g, device=DEV)
        log = ts.step(train.all_rays[idx], train.all_rgbs[idx])
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    m.eval()
    m.use_stratified_sampling = False
    bounds = (-2.5, 2.5) * 3
    occ = HN.occupancy_grid(m, bounds, a.train_res, 1, a.sigma_min, dilate=1)
    build_ms, _ = timed(lambda: HN.occupancy_grid(m, bounds, a.train_res, 1, a.sigma_min, dilate=1), 2)
    hit = [float(HN.clip_rays(s['rays'], occ, m.near, m.far)['hit'].float().mean()) for s in samples]
    span = [float((lambda t: (t[:, 1] - t[:, 0]).mean())(HN.clip_rays(s['rays'], occ, m.near, m.far)['t'])) for s in samples]
    cases = []
    half = (nc // 2, nf // 2)
    # the model was trained with use_sample_at_infinity: its last sample, at `far`, carries what is left of the ray.  The
    # *_front cases clip the near end only and keep that sample at `far`; the *_no_inf pair renders without it.
    for name, counts, grid, clip_far, at_infinity in (
            ("plain", (nc, nf), None, True, True), ("clipped", (nc, nf), occ, True, True),
            ("clipped_half", half, occ, True, True), ("plain_half", half, None, True, True),
            ("clipped_front", (nc, nf), occ, False, True), ("clipped_front_half", half, occ, False, True),
            ("plain_no_inf", (nc, nf), None, True, False), ("clipped_no_inf", (nc, nf), occ, True, False)):
        m.num_coarse_samples, m.num_fine_samples = counts
        m.use_sample_at_infinity = at_infinity
        kw = {} if grid is None else dict(occupancy=grid, clip_far=clip_far)
        res = inference.evaluate_images(m, samples, chunk=a.chunk, **kw)
        render = lambda: [inference.render_image(m, s['rays'], chunk=a.chunk, keys=('rgb', 'depth'), **kw) for s in samples]
        ms, _ = timed(render, a.image_reps)
        cases.append({"case": name, "samples": list(counts), "clip_far": clip_far, "sample_at_infinity": at_infinity,
                      "mean_psnr": res['mean_psnr'], "psnrs": res['psnrs'], "mean_ssim": res['mean_ssim'],
                      "images_per_s": len(samples) / ms * 1e3})
    m.num_coarse_samples, m.num_fine_samples = nc, nf
    m.use_sample_at_infinity = True
    return {"scene": f"tests/blender_scene.py seed 23 at {size}x{size}, 5 train / 8 val images", "train_steps": a.train_steps,
            "batch": batch, "train_s": train_s, "last_loss": float(log["train/loss"]), "bounds": list(bounds),
            "resolution": a.train_res, "sigma_min": a.sigma_min, "dilate": 1, "occupied_fraction": HN.occupancy_fraction(occ),
            "grid_build_ms": build_ms, "hit_fraction": sum(hit) / len(hit), "mean_clipped_span": sum(span) / len(span),
            "near_far": [m.near, m.far], "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--image", type=int, nargs=2, default=[378, 504], metavar=("W", "H"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--image-reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--train-res", type=int, default=128)
    ap.add_argument("--sigma-min", type=float, default=0.5)
    ap.add_argument("--parent-inference", default=None)
    ap.add_argument("--skip-overhead", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hypernerf_torch_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("occupancy_bench.py measures on the GPU; none is visible")
    out = {"tool": "occupancy_bench", "image_wh": list(a.image), "repeats": a.repeats, "hbm_tbs": a.hbm_tbs,
           "build": L.build_id(), "kernels": kernels(a)}
    if not a.skip_overhead:
        out["overhead"] = overhead(a)
    if a.train_steps > 0:
        out["trained"] = trained(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
