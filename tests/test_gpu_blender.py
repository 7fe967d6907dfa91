"""GPU tests (MI355X) of the device-resident Blender dataset: the HIP RGBA LANCZOS resize against Pillow's bytes,
BlenderDataset against the reference's tensors at every size recorded in g23 (all_rgbs bit for bit: the blend onto
white is three separately rounded operations), RayBatcher against a shuffled DataLoader over all_rays / all_rgbs,
TrainStep(batcher=...) against TrainStep.step fed the same batches, the bounds check of the RGBA gather, no host sync
and no extra launch in a batched step, and evaluate_images over the val split with and without the valid mask."""
import os

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
from blender_scene import make_scene, write_scene
from gpu_common import DEV, EMB, load_hash
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses
from hypernerf_torch_amd.datasets import BlenderDataset, LLFFDataset, RayBatcher, image_io
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.training import TrainStep

pytestmark = pytest.mark.gpu
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
SIZES = (64, 32, 24, 80)
ROW_STEP = 7


@pytest.fixture(scope="module")
def g23(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g23_blender.npz")))


@pytest.fixture(scope="module")
def scene(g23, tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("g23")), {s: (g23[f"scene_{s}_pixels"], g23[f"scene_{s}_poses"])
                                                             for s in ("train", "val", "test")})


def _rays_close(got, ref, what):
    """g15's bound, as test_gpu_datasets.py: 2e-6 of the rows' scale (the reference's CPU matmul may fuse
    multiply-adds)."""
    got = got.detach().cpu().double()
    ref = torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= 2e-6 * max(1.0, ref.abs().max().item()), (what, err)


def test_hip_rgba_resize_equals_pillow(g23):
    cases = sorted(k[len("resize_"):-len("_in")] for k in g23 if k.startswith("resize_") and k.endswith("_in"))
    assert len(cases) == 7
    for c in cases:
        src, ref = g23[f"resize_{c}_in"], g23[f"resize_{c}_out"]
        x = torch.from_numpy(src).to(DEV)
        got = F.resize_lanczos_rgba8(x, (ref.shape[1], ref.shape[0]))
        assert got.dtype == torch.uint8 and got.data_ptr() != x.data_ptr()
        assert np.array_equal(got.cpu().numpy(), ref), c
    # the two conversions alone, against their NumPy statements
    src = g23["resize_down_in"]
    pm = F.premultiply_u8(torch.from_numpy(src).to(DEV))
    assert np.array_equal(pm.cpu().numpy(), image_io.premultiply_u8_reference(src))
    back = F.premultiply_u8(pm, inverse=True)
    assert np.array_equal(back.cpu().numpy(), image_io.unpremultiply_u8_reference(pm.cpu().numpy()))


def test_blend_white_is_three_rounded_operations():
    """Every (colour, alpha) byte pair: hn_blend_white_u8 equals the reference's expression on ToTensor values bit for
    bit, and the mask is alpha > 0."""
    c, a = torch.meshgrid(torch.arange(256), torch.arange(256), indexing="ij")
    rgba = torch.stack([c, 255 - c, (c * 7 + 3) % 256, a], -1).reshape(-1, 4).to(torch.uint8)
    x = rgba.float().div(255)
    ref = x[:, :3] * x[:, 3:] + (1 - x[:, 3:])
    got, mask = F.blend_white_u8(rgba.to(DEV), with_mask=True)
    assert got.shape == (65536, 3) and mask.dtype == torch.bool and mask.shape == (65536,)
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(mask.cpu(), rgba[:, 3] > 0)
    assert torch.equal(F.blend_white_u8(rgba.to(DEV)), got)
    fused = (x[:, :3].double() * x[:, 3:].double() + (1 - x[:, 3:]).double()).float()
    assert (fused != ref).any()            # the distinction is real on these inputs


def test_blender_train_matches_reference(g23, scene):
    for s in SIZES:
        tag = f"train_{s}"
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        ds = BlenderDataset(scene, split="train", img_wh=(s, s))
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated() - before
        assert len(ds) == int(g23[f"{tag}/len"]) == ds.n_rays == 5 * s * s and ds.ray_cols == 8
        assert ds.focal == float(g23[f"{tag}/focal"]) and np.array_equal(np.stack(ds.poses), g23[f"{tag}/poses"])
        assert ds.white_back is True and (ds.near, ds.far) == (2.0, 6.0) and len(ds.image_paths) == 5
        # nothing per ray until asked: the device holds the uint8 stack (4 B/ray), the poses and the resize tables
        # (a few KB, each rounded up to the allocator's 512 B) — all_rgbs alone would be 12 B/ray more
        assert ds.rgba8.dtype == torch.uint8 and tuple(ds.rgba8.shape) == (5, s, s, 4)
        assert ds._all_rays is None and ds._all_rgbs is None
        assert held <= 4 * ds.n_rays + 16384, (tag, held)
        rgbs = ds.all_rgbs
        assert rgbs.dtype == torch.float32 and torch.equal(rgbs.cpu(), torch.from_numpy(g23[f"{tag}/rgbs"])), tag
        rays = ds.all_rays
        assert rays.shape == (len(ds), 8)
        sel = torch.from_numpy(g23[f"{tag}/rays_sel"].astype(np.int64))
        _rays_close(rays[sel.to(DEV)], g23[f"{tag}/rays_rows"], tag)
        smp = ds[5]
        assert torch.equal(smp["rays"], rays[5]) and torch.equal(smp["rgbs"], rgbs[5])
        other = BlenderDataset(scene, split="train", img_wh=(s, s), use_pillow=False)
        assert torch.equal(other.rgba8, ds.rgba8) and torch.equal(other.c2w, ds.c2w)
        assert torch.equal(other.all_rgbs, rgbs) and torch.equal(other.all_rays, rays)
        del ds, other, rgbs, rays, smp          # so that the next size's `held` counts its own dataset only


def test_blender_val_and_test_samples_match_reference(g23, scene):
    tags = sorted({k.split("/")[0] for k in g23 if k.endswith("/valid_mask")})
    assert len(tags) == 7
    for tag in tags:
        split, s, k = tag.split("_")
        s, k = int(s), int(k)
        ds = BlenderDataset(scene, split=split, img_wh=(s, s))
        assert len(ds) == int(g23[f"{split}_{s}/len"]) == (8 if split == "val" else 3)
        smp = ds[k]
        assert smp["hw"] == (s, s) and all(smp[key].is_cuda for key in ("rays", "rgbs", "c2w", "valid_mask"))
        assert torch.equal(smp["c2w"].cpu(), torch.from_numpy(g23[f"{tag}/c2w"])), tag
        assert torch.equal(smp["rgbs"].cpu(), torch.from_numpy(g23[f"{tag}/rgbs"])), tag
        assert smp["valid_mask"].dtype == torch.bool and smp["valid_mask"].shape == (s * s,)
        assert torch.equal(smp["valid_mask"].cpu(), torch.from_numpy(g23[f"{tag}/valid_mask"])), tag
        assert smp["rays"].shape == (s * s, 8)
        _rays_close(smp["rays"][::ROW_STEP], g23[f"{tag}/rays"], tag)
        with pytest.raises(IndexError):
            ds[len(ds)]


def test_ray_batcher_equals_dataloader(tmp_path):
    """Two full epochs on a 6-image 160 x 160 scene (resized from 200 x 200): RayBatcher(generator=g) yields exactly
    the batches of DataLoader(batch_size=B, shuffle=True, generator=g) over all_rays / all_rgbs, short last batch
    included."""
    root = write_scene(str(tmp_path / "big"), make_scene(seed=7, size=200, frames=(("train", 6),)))
    ds = BlenderDataset(root, split="train", img_wh=(160, 160))
    n, b = len(ds), 4096
    assert n == 6 * 160 * 160 and n % b != 0
    batcher = RayBatcher(ds, b, generator=torch.Generator().manual_seed(3))
    assert batcher.steps_per_epoch == -(-n // b)
    loader = torch.utils.data.DataLoader(range(n), batch_size=b, shuffle=True,
                                         generator=torch.Generator().manual_seed(3))
    all_rays, all_rgbs = ds.all_rays, ds.all_rgbs
    a8 = ds.rgba8.reshape(-1, 4)[:, 3]
    assert min(float((a8 == 0).float().mean()), float((a8 == 255).float().mean())) > 0.1
    for _ in range(2):
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        steps = 0
        for (rays, rgbs), idx in zip(batcher, loader):
            idx = idx.to(DEV)
            assert rays.shape == (idx.numel(), 8) and rgbs.shape == (idx.numel(), 3)
            assert torch.equal(rays, all_rays[idx]) and torch.equal(rgbs, all_rgbs[idx])
            seen.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
            steps += 1
        assert steps == batcher.steps_per_epoch and rays.shape[0] == n % b
        assert bool((seen == 1).all())
        assert torch.equal(torch.sort(batcher.perm).values, torch.arange(n, device=DEV))
    batcher.check()


NS = 32          # samples per level: a multiple of 32 keeps the whole gradient of a step bit-reproducible


def _small_model(seed, precision, ns=NS):
    HN.set_precision(precision)
    m = models.NerfModel(EMB, n_samples_coarse=ns, n_samples_fine=ns, noise_std=None, **KW)
    load_hash(m, seed)
    return m.to(DEV)


def _rng_for(rows, gen):
    return {"t_rand": torch.rand((rows, NS), generator=gen).to(DEV), "u": torch.rand((rows, NS), generator=gen).to(DEV)}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainstep_with_batcher_matches_step(scene, precision):
    """TrainStep(batcher=...) over three epochs of the g23 scene at 24 x 24, B = 1024 (2880 rays: every epoch ends on a
    short batch of 832) leaves the parameters bit-identical to a TrainStep on a copy of the model driven by
    step(rays, rgbs) with the batches RayBatcher yields eagerly and the same injected draws; the batch the graph
    gathers equals the eager batch bit for bit at every step."""
    ds = BlenderDataset(scene, split="train", img_wh=(24, 24))
    b = 1024
    m1, m2 = _small_model(3, precision), _small_model(3, precision)
    ts1 = TrainStep(m1, lr=1e-3, batcher=RayBatcher(ds, b, generator=torch.Generator().manual_seed(9)))
    ts2 = TrainStep(m2, lr=1e-3)
    eager = RayBatcher(ds, b, generator=torch.Generator().manual_seed(9))
    assert ts1.batcher.short_rows == len(ds) % b == 832
    g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    n_steps = 0
    for epoch in range(3):
        for rays, rgbs in eager:
            rows = rays.shape[0]
            l1 = ts1.step(rng=_rng_for(rows, g1))
            assert torch.equal(ts1.batcher.rays[:rows], rays) and torch.equal(ts1.batcher.rgbs[:rows], rgbs)
            l2 = ts2.step(rays.clone(), rgbs.clone(), rng=_rng_for(rows, g2))
            assert torch.equal(l1["train/loss"], l2["train/loss"]), (epoch, n_steps)
            assert torch.equal(ts1.arena.data, ts2.arena.data), (epoch, n_steps)
            n_steps += 1
        ts1.epoch_end()
        ts2.epoch_end()
    assert n_steps == 9 and len(ts1._batched) == 2          # one program per batch size, no recapture per epoch
    ts1.batcher.check()


def test_rgba_gather_past_the_permutation_is_flagged(scene):
    """A gather past the end of the epoch's permutation writes NaN rows and sets the error word instead of reading out
    of bounds or wrapping; begin_epoch() reports it.  (The kernel's bounds check is what is under test: nothing
    faults.)"""
    ds = BlenderDataset(scene, split="train", img_wh=(32, 32))
    bt = RayBatcher(ds, 1024, generator=torch.Generator().manual_seed(4))
    bt.begin_epoch()
    bt.launch(1024)
    assert int(bt.state[0]) == 1024 and int(bt.state[2]) == 0 and not torch.isnan(bt.rays).any()
    bt.state[0] = len(ds) - 10                       # 10 rays left; gather 1024
    bt.launch(1024)
    assert int(bt.state[0]) == len(ds) - 10 + 1024 and int(bt.state[1]) == 0 and int(bt.state[2]) == 1
    idx = bt.perm[len(ds) - 10:]
    assert torch.equal(bt.rays[:10], ds.all_rays[idx]) and torch.equal(bt.rgbs[:10], ds.all_rgbs[idx])
    assert torch.isnan(bt.rays[10:1024]).all() and torch.isnan(bt.rgbs[10:1024]).all()
    with pytest.raises(HN._lib.HnError, match="out of step"):
        bt.begin_epoch()
    # an index outside the dataset inside the permutation is refused the same way
    bt.state.zero_()
    bt.perm[3] = len(ds)
    bt.perm[5] = -1
    bt.launch(1024)
    bad = torch.isnan(bt.rays).any(1)
    assert bad.nonzero().flatten().tolist() == [3, 5] and int(bt.state[2]) == 1
    assert torch.isnan(bt.rgbs[[3, 5]]).all() and not torch.isnan(bt.rgbs[bad.logical_not()]).any()


def _captured_launches(monkeypatch, ts):
    """Names of the C-ABI launches in the program that the first step() call captures: that call runs the step a few
    times to warm up and once more under capture, each run starting with the gather — the launches from the last
    gather on are the captured ones (the replay that follows launches nothing from Python)."""
    names = []
    real = HN._lib.launch

    def counting(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(HN._lib, "launch", counting)
    try:
        ts.step()
    finally:
        monkeypatch.setattr(HN._lib, "launch", real)
    gathers = [i for i, n in enumerate(names) if n.startswith("hn_ray_batch")]
    assert len(gathers) >= 2, names
    return names[gathers[-1]:]


def test_batched_step_has_no_host_sync_and_no_extra_launch(scene, tmp_path, monkeypatch):
    """The batched step over a Blender dataset replays without a host sync, and its program holds the launches of the
    same step over an LLFF dataset of the same batch size and ray width — the blend lives in the gather launch."""
    from llff_scene import make_scene as llff_make, write_scene as llff_write
    blender = BlenderDataset(scene, split="train", img_wh=(32, 32))
    llff = LLFFDataset(llff_write(str(tmp_path / "llff"), *llff_make(6, 30, 40)), split="train", img_wh=(40, 30))
    assert blender.ray_cols == llff.ray_cols == 8
    launches = {}
    for name, ds in (("blender", blender), ("llff", llff)):
        m = _small_model(4, "bf16")
        ts = TrainStep(m, lr=1e-3, batcher=RayBatcher(ds, 512, generator=torch.Generator().manual_seed(2)))
        launches[name] = _captured_launches(monkeypatch, ts)
        for _ in range(2):
            ts.step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                ts.step()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        ts.batcher.check()
    assert launches["blender"][0] == "hn_ray_batch_rgba" and launches["llff"][0] == "hn_ray_batch"
    assert "hn_blend_white_u8" not in launches["blender"] and len(launches["blender"]) > 10
    assert launches["blender"][1:] == launches["llff"][1:]


def test_evaluate_images_over_val_split(scene):
    from hypernerf_torch_amd.inference import evaluate_images, render_image
    m = _small_model(5, "fp32").eval()
    m.use_stratified_sampling = False
    ds = BlenderDataset(scene, split="val", img_wh=(24, 24))
    plain = evaluate_images(m, ds)
    masked = evaluate_images(m, ds, use_valid_mask=True)
    assert len(plain["psnrs"]) == len(masked["psnrs"]) == 8 and plain["images"][0].shape == (24, 24, 3)
    n_partial = 0
    for i in range(8):
        s = ds[i]
        img = render_image(m, s["rays"], keys=("rgb", "depth"))["rgb"].view(24, 24, 3)
        gt = s["rgbs"].view(24, 24, 3)
        mask = s["valid_mask"].view(24, 24)
        assert plain["psnrs"][i] == float(losses.psnr(gt, img)), i
        assert masked["psnrs"][i] == float(losses.psnr(gt, img, valid_mask=mask)), i
        n_partial += int(0 < int(mask.sum()) < mask.numel() and masked["psnrs"][i] != plain["psnrs"][i])
    assert n_partial == 8                  # the mask excludes pixels in every image, and the figure moves
    assert plain["mean_psnr"] == sum(plain["psnrs"]) / 8
