"""Times training-time occupancy (hn_occ_clip_batch, TrainStep(occupancy=)), one JSON line per run:

  python tools/train_occupancy_bench.py --sections kernels step refresh
  python tools/train_occupancy_bench.py --sections step --parent-root DIR     # + another checkout (built), in alternation
  python tools/train_occupancy_bench.py --sections trained --train-steps 800

`kernels`: hn_occ_clip_batch beside hn_occ_clip_rays on the same rays (origins at radius 0.2 .. 4 aimed at the box, all of
frame 7), at 1024 and 4096 rays, 64^3 and 128^3 lattices, clip_far 0 and 1, a random grid with about 15 % of the cells
occupied and an all-occupied one.  A sample is the host wall clock around `--burst` back-to-back calls ended by a device
synchronise, divided by the burst; the variants alternate for `--reps` rounds; median, min and max are reported.

`step`: config 2 of bench.py (1024 rays, 64 + 64 samples, bf16) through TrainStep as a replayed graph: plain, and with an
all-occupied TrainOccupancy whose box holds every ray (nothing is clipped: the price of the feature's plumbing).  The
variants alternate in windows of `--window` steps.  With --parent-root the same plain step of another checkout runs in
child processes that alternate with child processes of this tree.

`refresh`: one occupancy_grid of a frame (the field queried at every lattice point, mark, one dilation) at 64^3 and 128^3.

`trained` (--train-steps N): the synthetic Blender scene of tests/blender_scene.py at 128 x 128, N steps of 4096 rays each
for: plain 64 + 64, plain 32 + 32, occupancy 32 + 32 with clip_far=False (64^3 cells, warm-up N / 4 steps, a refresh every
16 steps) — ms per step over the last half of the run, and PSNR / SSIM of the val split rendered plain with each model's
own sample counts.  That scene's images are not views of one object: it can show that clipping does no harm, not what
it gains on a real capture."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BOUNDS = (-1.5, 1.5) * 3
NEAR, FAR = 0.5, 6.0


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def alternate(variants, reps, burst):
    import torch
    times = {name: [] for name in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(burst):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / burst * 1e3)
    return {name: spread(ms) for name, ms in times.items()}


def kernels(a):
    import numpy as np
    import torch
    import hypernerf_torch_amd as HN
    rows = []
    for res in a.res:
        cells = (res - 1,) * 3
        words = (cells[2] + 63) // 64
        rng = np.random.default_rng(res)
        grids = {"random_15pct": rng.random(cells) < 0.15, "all_occupied": np.ones(cells, dtype=bool)}
        for n in a.rays:
            u = rng.normal(size=(n, 3))
            o = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.2, 4.0, size=(n, 1))
            d = rng.uniform(-2.0, 2.0, size=(n, 3)) - o
            d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.6, size=(n, 1))
            rays = np.zeros((n, 9), dtype=np.float32)
            rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7], rays[:, 8] = o, d, NEAR, FAR, 7
            rays = torch.from_numpy(rays).to(DEV)
            for grid_name, grid in grids.items():
                padded = np.zeros(cells[:2] + (64 * words,), dtype=np.uint64)
                padded[:, :, :cells[2]] = grid
                bits = (padded.reshape(cells[0], cells[1], words, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
                occ = {'bits': torch.from_numpy(bits.view(np.int64)).to(DEV), 'cells': cells, 'bounds': BOUNDS}
                stack = HN.OccupancyStack(cells, BOUNDS, [7], device=DEV)
                stack.set(7, occ)
                out = HN.clip_batch(rays, stack, NEAR, FAR)
                variants = {}
                for clip_far in (0, 1):
                    variants[f"clip_batch_far{clip_far}"] = (
                        lambda cf=clip_far: HN.clip_batch(rays, stack, NEAR, FAR, clip_far=bool(cf), out=out))
                    variants[f"clip_rays_far{clip_far}"] = lambda cf=clip_far: HN.clip_rays(rays, occ, NEAR, FAR, clip_far=bool(cf))
                same = all(torch.equal(HN.clip_batch(rays, stack, NEAR, FAR, clip_far=bool(cf))['rays'],
                                       HN.clip_rays(rays, occ, NEAR, FAR, clip_far=bool(cf))['rays']) for cf in (0, 1))
                rows.append({"resolution": res, "rays": n, "grid": grid_name, "occupied_fraction": float(grid.mean()),
                             "hit_fraction": float(out['hit'].float().mean()), "bit_identical": bool(same),
                             "ms": alternate(variants, a.reps, a.burst)})
    return rows


def config2(torch):
    import hypernerf_torch_amd as HN
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    HN.set_precision("bf16")
    emb = {"warp": list(range(100)), "camera": [0], "appearance": list(range(100)), "time": list(range(100))}
    b = 1024
    g = torch.Generator(device="cpu").manual_seed(1234)
    o = torch.rand(b, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(b, 3, generator=g), dim=-1)
    ids = torch.randint(0, 100, (b, 1), generator=g).float()
    target = torch.rand(b, 3, generator=g).to(DEV)
    torch.manual_seed(0)
    model = NerfModel(emb, near=0.0, far=1.0, n_samples_coarse=64, n_samples_fine=64, noise_std=1.0, view_fourier_dim=6,
                      hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True).to(DEV)
    rays = torch.cat([o, d, torch.zeros(b, 1), torch.ones(b, 1), ids], dim=1).to(DEV)
    return model, rays, target


def step(a):
    """{variant: spread} of config-2 steps in windows; `a.variants` picks plain and / or identity."""
    import torch
    from hypernerf_torch_amd.training import TrainStep
    steps = {}
    for name in a.variants:
        model, rays, target = config2(torch)
        kw = {}
        if name == "identity":
            from hypernerf_torch_amd.training import TrainOccupancy
            ids = sorted({int(v) for v in rays[:, 8].tolist()})
            kw["occupancy"] = TrainOccupancy(model, (-4.0, 4.0) * 3, 128, ids, 0.5, warmup_steps=10 ** 9)
        ts = TrainStep(model, lr=5e-4, **kw)
        for _ in range(a.warmup):
            log = ts.step(rays, target)
        steps[name] = (ts, rays, target)
        if name == "identity":
            assert float(log["train/occupancy_hit"]) == 1.0 and float(log["train/occupancy_span"]) == 1.0
    torch.cuda.synchronize()
    times = {name: [] for name in steps}
    for _ in range(a.windows):
        for name, (ts, rays, target) in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.window):
                ts.step(rays, target)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.window * 1e3)
    return {name: dict(spread(ms), windows_ms=ms) for name, ms in times.items()}


def step_with_parent(a):
    """Child processes in alternation: this tree (plain and identity, alternating inside), the parent tree (plain)."""
    me = os.path.abspath(__file__)
    runs = {"this": [], "parent": []}
    for _ in range(a.parent_rounds):
        for which, root, variants in (("this", ROOT, ["plain", "identity"]), ("parent", a.parent_root, ["plain"])):
            cmd = [sys.executable, me, "--sections", "step", "--package-root", root, "--windows", str(a.windows), "--window",
                   str(a.window), "--warmup", str(a.warmup), "--variants"] + variants
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(f"child ({which}) failed:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            runs[which].append(json.loads(res.stdout.strip().splitlines()[-1])["step"])
    out = {}
    for which, variants in (("this", ["plain", "identity"]), ("parent", ["plain"])):
        for v in variants:
            ms = [w for r in runs[which] for w in r[v]["windows_ms"]]
            out[f"{which}_{v}"] = dict(spread(ms), per_process_median_ms=[r[v]["median_ms"] for r in runs[which]])
    return out


def refresh(a):
    import torch
    import hypernerf_torch_amd as HN
    model, rays, _ = config2(torch)
    rows = []
    for res in a.res:
        fn = lambda: HN.occupancy_grid(model, (-4.0, 4.0) * 3, res, 7, 0.5, dilate=1)
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(spread(ms), resolution=res, lattice_points=res ** 3,
                         what="occupancy_grid of one frame: field query at every lattice point, mark, one dilation (bf16, config 2)"))
    return rows


def trained(a):
    import torch
    import hypernerf_torch_amd as HN
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from blender_scene import make_scene, write_scene
    from hypernerf_torch_amd import inference
    from hypernerf_torch_amd.datasets import BlenderDataset
    from hypernerf_torch_amd.hypernerf import models
    from hypernerf_torch_amd.training import TrainOccupancy, TrainStep
    size, batch = 128, 4096
    HN.set_precision("bf16")
    emb = {k: list(range(100)) for k in ("warp", "appearance", "time")}
    emb["camera"] = [0]
    with tempfile.TemporaryDirectory() as tmp:
        root = write_scene(os.path.join(tmp, "scene"), make_scene(seed=23, size=size))
        train = BlenderDataset(root, split="train", img_wh=(size, size))
        val = BlenderDataset(root, split="val", img_wh=(size, size))
        samples = [val[i] for i in range(len(val))]
    bounds = (-2.5, 2.5) * 3
    cases = []
    for name, counts, with_occ in (("plain_64_64", (64, 64), False), ("plain_32_32", (32, 32), False),
                                   ("occupancy_32_32_front", (32, 32), True)):
        torch.manual_seed(0)
        m = models.NerfModel(emb, near=train.near, far=train.far, n_samples_coarse=counts[0], n_samples_fine=counts[1],
                             hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True).to(DEV)
        m.use_white_background = True
        occ = None
        if with_occ:
            # rows without an id column: the clip gives them id 0, prepare_ray_dict renders them as frame 1
            occ = TrainOccupancy(m, bounds, a.train_res, [0], a.sigma_min, dilate=1, clip_far=False,
                                 warmup_steps=a.train_steps // 4, refresh_every=16,
                                 builder=lambda _: HN.occupancy_grid(m, bounds, a.train_res, 1, a.sigma_min, dilate=1))
        ts = TrainStep(m, lr=5e-4, occupancy=occ)
        g = torch.Generator(device=DEV).manual_seed(3)
        half_t = None
        for i in range(a.train_steps):
            if i == a.train_steps // 2:
                torch.cuda.synchronize()
                half_t = time.perf_counter()
            idx = torch.randint(0, train.all_rays.shape[0], (batch,), generator=g, device=DEV)
            log = ts.step(train.all_rays[idx], train.all_rgbs[idx])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - half_t) / (a.train_steps - a.train_steps // 2) * 1e3
        m.eval()
        m.use_stratified_sampling = False
        res = inference.evaluate_images(m, samples, chunk=32768)
        case = {"case": name, "samples": list(counts), "ms_per_step_last_half": ms, "last_loss": float(log["train/loss"]),
                "mean_psnr": res['mean_psnr'], "mean_ssim": res['mean_ssim'], "psnrs": res['psnrs']}
        if occ is not None:
            case.update(refreshes=occ.refreshes, occupied_fraction=HN.occupancy_fraction(occ.stack.occupancy(0)),
                        last_hit=float(log["train/occupancy_hit"]), last_span=float(log["train/occupancy_span"]))
        cases.append(case)
        m.train()
    return {"scene": f"tests/blender_scene.py seed 23 at {size}x{size}", "train_steps": a.train_steps, "batch": batch,
            "bounds": list(bounds), "resolution": a.train_res, "sigma_min": a.sigma_min, "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", nargs="+", default=["kernels", "step", "refresh"],
                    choices=["kernels", "step", "refresh", "trained"])
    ap.add_argument("--res", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--variants", nargs="+", default=["plain", "identity"], choices=["plain", "identity"])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package is imported")
    ap.add_argument("--parent-root", default=None, help="step: another built checkout, timed in alternating child processes")
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=800)
    ap.add_argument("--train-res", type=int, default=64)
    ap.add_argument("--sigma-min", type=float, default=0.5)
    a = ap.parse_args()
    out = {"tool": "train_occupancy_bench"}
    if "step" in a.sections and a.parent_root:
        out["step_with_parent"] = step_with_parent(a)        # children only: before this process opens the GPU
        a.sections = [s for s in a.sections if s != "step"]
    sys.path.insert(0, a.package_root)
    import torch
    from hypernerf_torch_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("train_occupancy_bench.py measures on the GPU; none is visible")
    out["build"] = L.build_id()
    for section in a.sections:
        out[section] = {"kernels": kernels, "step": step, "refresh": refresh, "trained": trained}[section](a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
