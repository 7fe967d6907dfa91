"""Data-path measurements of the datasets (hypernerf_torch_amd.datasets), one JSON line per part:

  python tools/data_bench.py --part load     # dataset load: decode, HIP LANCZOS resize vs Pillow's, whole constructor
  python tools/data_bench.py --part steps    # steps/s at config 2 (1024 rays x (64+64), bf16, graphs): fed the
                                             # reference's way (CPU DataLoader -> .cuda() -> step(rays, rgbs), 0 and
                                             # 3 workers) vs TrainStep(batcher=RayBatcher(...))
  python tools/data_bench.py --part kernel   # hn_ray_batch launches only, for a run of its own under
                                             # rocprofv3 --kernel-trace --stats (kernel time from the trace)

`--dataset blender` (default: llff) measures the same parts on a Blender scene of RGBA images (20 images of 512 x 512
resized to 436 x 436: as many rays as the LLFF scene within 0.3 %); its `kernel` part launches the RGB gather on the
LLFF scene as well, so that one trace holds hn_ray_batch_kernel<3, false> and <4, false> side by side at 8 ray columns
each.

`--dataset nerfies` measures `steps` (batcher-fed only: there is no reference loader to feed a DataLoader from) and
`kernel` on a Nerfies-format capture of 20 images of 504 x 378 at image_scale 1, every camera with lens distortion but
the first (as many rays as the LLFF scene); its `kernel` part launches the LLFF gather as well, 9 ray columns each, so
that one trace holds hn_ray_batch_kernel<3, false> and hn_ray_batch_kernel<3, true> (the Nerfies camera) side by side.

Scenes are synthetic and seeded (tests/llff_scene.py, tests/blender_scene.py, tests/nerfies_scene.py), written to a temporary directory.  Times are host wall clock
around work that ends in a device synchronise, after warm-up.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hypernerf_torch_amd as HN  # noqa: E402
from hypernerf_torch_amd import functional as F  # noqa: E402
from hypernerf_torch_amd.datasets import BlenderDataset, LLFFDataset, NerfiesDataset, RayBatcher, image_io  # noqa: E402
import blender_scene  # noqa: E402
import nerfies_scene  # noqa: E402
from llff_scene import make_scene, write_scene  # noqa: E402

DEV = "cuda:0"
BLENDER_SRC, BLENDER_WH = 512, (436, 436)


def _blender_train(a, tmp, seed):
    scene = blender_scene.make_scene(seed=seed, size=BLENDER_SRC, frames=(("train", a.images),))
    return blender_scene.write_scene(os.path.join(tmp, f"blender{seed}"), scene)


def _nerfies_train(a, tmp, seed):
    scene = nerfies_scene.make_scene(seed, wh=(504, 378), n_train=a.images, n_val=0, image_scale=1)
    root = nerfies_scene.write_scene(os.path.join(tmp, f"nerfies{seed}"), scene)
    return NerfiesDataset(root, split="train", image_scale=1)


def _sync_time(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def part_load_blender(a, tmp):
    root = _blender_train(a, tmp, 11)
    paths = sorted(os.path.join(root, "train", f) for f in os.listdir(os.path.join(root, "train")))
    decoded = [image_io.load_rgba8(p) for p in paths[:2]]
    wh = BLENDER_WH
    out = {"part": "load", "dataset": "blender", "images": a.images, "source_hw": [BLENDER_SRC, BLENDER_SRC],
           "img_wh": list(wh), "pillow": image_io.have_pillow()}
    t0 = time.perf_counter()
    for p in paths:
        image_io.load_rgba8(p)
    out["decode_ms_per_image"] = (time.perf_counter() - t0) / len(paths) * 1e3
    x = torch.from_numpy(decoded[0]).to(DEV)
    F.resize_lanczos_rgba8(x, wh)                              # tables + first launches
    out["hip_resize_ms_per_image"] = _sync_time(lambda: F.resize_lanczos_rgba8(x, wh), reps=20) * 1e3
    if image_io.have_pillow():
        from PIL import Image
        im = Image.fromarray(decoded[0], "RGBA")
        t0 = time.perf_counter()
        for _ in range(5):
            r = im.resize(wh, Image.Resampling.LANCZOS)
        out["pillow_resize_ms_per_image"] = (time.perf_counter() - t0) / 5 * 1e3
        out["hip_equals_pillow"] = bool(np.array_equal(np.asarray(r), F.resize_lanczos_rgba8(x, wh).cpu().numpy()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = BlenderDataset(root, split="train", img_wh=wh)
    torch.cuda.synchronize()
    out["dataset_train_s"] = time.perf_counter() - t0
    out["dataset_device_bytes"] = ds.rgba8.numel() + ds.c2w.numel() * 4
    out["all_rays_rgbs_bytes_if_built"] = ds.n_rays * (ds.ray_cols + 3) * 4
    return out


def part_load(a, tmp):
    if a.dataset == "blender":
        return part_load_blender(a, tmp)
    if a.dataset == "nerfies":
        raise SystemExit("--dataset nerfies has no `load` part: its images are read as they are, without a resize")
    src_h, src_w = a.src_hw
    pix, pb = make_scene(a.images, src_h, src_w, seed=11, focal=1.1 * src_w)
    root = write_scene(os.path.join(tmp, "load"), pix, pb)
    wh = (504, 378)
    paths = sorted(os.path.join(root, "images", f) for f in os.listdir(os.path.join(root, "images")))
    decoded = [image_io.load_rgb8(p) for p in paths[:2]]
    out = {"part": "load", "images": a.images, "source_hw": [src_h, src_w], "img_wh": list(wh),
           "pillow": image_io.have_pillow()}
    t0 = time.perf_counter()
    for p in paths:
        image_io.load_rgb8(p)
    out["decode_ms_per_image"] = (time.perf_counter() - t0) / len(paths) * 1e3
    x = torch.from_numpy(decoded[0]).to(DEV)
    F.resize_lanczos_u8(x, wh)                                 # tables + first launch
    out["hip_resize_ms_per_image"] = _sync_time(lambda: F.resize_lanczos_u8(x, wh), reps=20) * 1e3
    out["upload_and_hip_resize_ms_per_image"] = _sync_time(
        lambda: F.resize_lanczos_u8(torch.from_numpy(decoded[1]).to(DEV), wh), reps=10) * 1e3
    if image_io.have_pillow():
        from PIL import Image
        im = Image.fromarray(decoded[0])
        t0 = time.perf_counter()
        for _ in range(5):
            r = im.resize(wh, Image.Resampling.LANCZOS)
        out["pillow_resize_ms_per_image"] = (time.perf_counter() - t0) / 5 * 1e3
        out["hip_equals_pillow"] = bool(np.array_equal(np.asarray(r), F.resize_lanczos_u8(x, wh).cpu().numpy()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = LLFFDataset(root, split="train", img_wh=wh)
    torch.cuda.synchronize()
    out["dataset_train_s"] = time.perf_counter() - t0
    out["dataset_device_bytes"] = ds.rgb8.numel() + ds.c2w.numel() * 4
    out["all_rays_rgbs_bytes_if_built"] = ds.n_rays * (ds.ray_cols + 3) * 4
    return out


class _DictRays(torch.utils.data.Dataset):
    """What the reference's train split hands a DataLoader: one dict per ray from host tensors."""

    def __init__(self, rays, rgbs):
        self.rays, self.rgbs = rays, rgbs

    def __len__(self):
        return self.rays.shape[0]

    def __getitem__(self, i):
        return {'rays': self.rays[i], 'rgbs': self.rgbs[i]}


def _config2_step(batcher=None, near=0.0, far=1.0):
    from gpu_common import EMB
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    from hypernerf_torch_amd.training import TrainStep
    HN.set_precision("bf16")
    torch.manual_seed(0)
    m = NerfModel(EMB, near=near, far=far, n_samples_coarse=64, n_samples_fine=64, noise_std=1.0, view_fourier_dim=6,
                  hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True).to(DEV)
    return TrainStep(m, lr=5e-4, batcher=batcher)


def part_steps(a, tmp):
    if a.dataset == "nerfies":
        ds = _nerfies_train(a, tmp, 12)
        ts = _config2_step(RayBatcher(ds, 1024, generator=torch.Generator().manual_seed(0)), near=ds.near, far=ds.far)
        for _ in range(a.warmup):
            ts.step()
        dt = _sync_time(ts.step, reps=a.steps)
        ts.batcher.check()
        return {"part": "steps", "dataset": "nerfies", "rays": ds.n_rays, "batch": 1024, "steps": a.steps,
                "warmup": a.warmup, "batcher_ms_per_step": dt * 1e3, "batcher_steps_per_s": 1.0 / dt,
                "workload": "NerfModel use_warp bendy_sheet nerf_embed+alpha_cond, 1024 rays x (64+64), bf16, graphs"}
    if a.dataset == "blender":
        ds = BlenderDataset(_blender_train(a, tmp, 12), split="train", img_wh=BLENDER_WH)
        head = {"part": "steps", "dataset": "blender"}
    else:
        pix, pb = make_scene(a.images, 378, 504, seed=12, focal=400.0)
        root = write_scene(os.path.join(tmp, "steps"), pix, pb)
        ds = LLFFDataset(root, split="train", img_wh=(504, 378), include_idx=True)
        head = {"part": "steps"}
    b, steps, warm = 1024, a.steps, a.warmup
    out = {**head, "rays": ds.n_rays, "batch": b, "steps": steps, "warmup": warm,
           "workload": "NerfModel use_warp bendy_sheet nerf_embed+alpha_cond, 1024 rays x (64+64), bf16, graphs"}

    # batcher-fed: the gather is the first launch of the captured step
    ts = _config2_step(RayBatcher(ds, b, generator=torch.Generator().manual_seed(0)))
    for _ in range(warm):
        ts.step()
    dt = _sync_time(ts.step, reps=steps)
    out["batcher_ms_per_step"] = dt * 1e3
    out["batcher_steps_per_s"] = 1.0 / dt

    # fed the reference's way: DataLoader(shuffle=True) over host dicts -> .cuda() -> step(rays, rgbs)
    host = _DictRays(ds.all_rays.cpu(), ds.all_rgbs.cpu())
    ds._all_rays = ds._all_rgbs = None
    for workers in a.workers:
        ts = _config2_step()
        loader = torch.utils.data.DataLoader(host, batch_size=b, shuffle=True, num_workers=workers,
                                             generator=torch.Generator().manual_seed(0))
        it = iter(loader)

        def one():
            batch = next(it)
            ts.step(batch['rays'].cuda(), batch['rgbs'].cuda())
        for _ in range(warm):
            one()
        dt = _sync_time(one, reps=steps)
        out[f"dataloader_w{workers}_ms_per_step"] = dt * 1e3
        out[f"dataloader_w{workers}_steps_per_s"] = 1.0 / dt
        t0 = time.perf_counter()
        for _ in range(steps):
            next(it)
        out[f"dataloader_w{workers}_host_ms_per_batch"] = (time.perf_counter() - t0) / steps * 1e3
        del it, loader
    return out


def part_kernel_blender(a, tmp):
    """Both gathers in one process, 8 ray columns each, alternating in blocks of 50 launches."""
    pix, pb = make_scene(a.images, 378, 504, seed=13, focal=400.0)
    llff = LLFFDataset(write_scene(os.path.join(tmp, "kernel"), pix, pb), split="train", img_wh=(504, 378))
    blender = BlenderDataset(_blender_train(a, tmp, 13), split="train", img_wh=BLENDER_WH)
    bts = [RayBatcher(ds, 1024, generator=torch.Generator().manual_seed(0)) for ds in (llff, blender)]
    for bt in bts:
        bt.begin_epoch()
    n = min(a.steps * 10, min(bt.steps_per_epoch for bt in bts) - 1)
    for k in range(0, n, 50):
        for bt in bts:
            for _ in range(min(50, n - k)):
                bt.launch(1024)
    torch.cuda.synchronize()
    for bt in bts:
        bt.check()
    return {"part": "kernel", "dataset": "blender", "launches_each": n, "batch": 1024,
            "rays": {"llff": llff.n_rays, "blender": blender.n_rays}, "bytes_written_per_launch": 1024 * (8 + 3) * 4,
            "kernels": {"llff": "hn_ray_batch_kernel<3, false>", "blender": "hn_ray_batch_kernel<4, false>"}}


def part_kernel_nerfies(a, tmp):
    """The LLFF and the Nerfies gather in one process, 9 ray columns each, alternating in blocks of 50 launches."""
    pix, pb = make_scene(a.images, 378, 504, seed=13, focal=400.0)
    llff = LLFFDataset(write_scene(os.path.join(tmp, "kernel"), pix, pb), split="train", img_wh=(504, 378),
                       include_idx=True)
    nerfies = _nerfies_train(a, tmp, 13)
    bts = [RayBatcher(ds, 1024, generator=torch.Generator().manual_seed(0)) for ds in (llff, nerfies)]
    for bt in bts:
        bt.begin_epoch()
    n = min(a.steps * 10, min(bt.steps_per_epoch for bt in bts) - 1)
    for k in range(0, n, 50):
        for bt in bts:
            for _ in range(min(50, n - k)):
                bt.launch(1024)
    torch.cuda.synchronize()
    for bt in bts:
        bt.check()
    return {"part": "kernel", "dataset": "nerfies", "launches_each": n, "batch": 1024,
            "rays": {"llff": llff.n_rays, "nerfies": nerfies.n_rays}, "bytes_written_per_launch": 1024 * (9 + 3) * 4,
            "kernels": {"llff": "hn_ray_batch_kernel<3, false>", "nerfies": "hn_ray_batch_kernel<3, true>"}}


def part_kernel(a, tmp):
    if a.dataset == "blender":
        return part_kernel_blender(a, tmp)
    if a.dataset == "nerfies":
        return part_kernel_nerfies(a, tmp)
    pix, pb = make_scene(a.images, 378, 504, seed=13, focal=400.0)
    root = write_scene(os.path.join(tmp, "kernel"), pix, pb)
    ds = LLFFDataset(root, split="train", img_wh=(504, 378), include_idx=True)
    bt = RayBatcher(ds, 1024, generator=torch.Generator().manual_seed(0))
    bt.begin_epoch()
    n = min(a.steps * 10, bt.steps_per_epoch - 1)
    for _ in range(n):
        bt.launch(1024)
    torch.cuda.synchronize()
    bt.check()
    return {"part": "kernel", "launches": n, "batch": 1024, "bytes_written_per_launch": 1024 * (9 + 3) * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("load", "steps", "kernel"), required=True)
    ap.add_argument("--dataset", choices=("llff", "blender", "nerfies"), default="llff")
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--src-hw", type=int, nargs=2, default=(1512, 2016), dest="src_hw")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workers", type=int, nargs="+", default=(0, 3))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_bench measures on the GPU; none is visible")
    with tempfile.TemporaryDirectory() as tmp:
        out = {"load": part_load, "steps": part_steps, "kernel": part_kernel}[a.part](a, tmp)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
