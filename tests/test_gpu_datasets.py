"""GPU tests (MI355X) of the device-resident LLFF dataset and the in-graph ray batcher: the HIP LANCZOS resize against
Pillow's bytes, LLFFDataset against the reference's tensors in every configuration recorded in g22, RayBatcher against
a shuffled DataLoader over all_rays / all_rgbs for two epochs, TrainStep(batcher=...) against TrainStep.step fed the
same batches, no host sync in a batched step, and evaluate_images over the val split."""
import os

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
from gpu_common import DEV, EMB, load_hash
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.datasets import LLFFDataset, RayBatcher, distributed_sampler_order
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.training import TrainStep
from llff_scene import make_scene, write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)


@pytest.fixture(scope="module")
def g22(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g22_llff.npz")))


@pytest.fixture(scope="module")
def scene(g22, tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("g22")), g22["scene_pixels"], g22["scene_poses_bounds"])


def _tags(g22, prefix):
    tags = set()
    for k in g22:
        parts = k.split("/")[0].rsplit("_", 3)
        if "/" in k and k.startswith(prefix) and len(parts) == 4 and parts[1] in "sn" and parts[2] in "ix":
            tags.add(k.split("/")[0])
    return sorted(tags)


def _cfg(tag):
    split, s, i, wh = tag.rsplit("_", 3)
    w, h = (int(v) for v in wh.split("x"))
    return split, s == "s", i == "i", (w, h)


def _rays_close(got, ref, what):
    """g15's bound: 2e-6 of the rows' scale (the reference's CPU matmul may fuse multiply-adds)."""
    got = got.detach().cpu().double()
    ref = torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= 2e-6 * max(1.0, ref.abs().max().item()), (what, err)


def _unit(u8):
    return torch.from_numpy(np.asarray(u8)).float() / 255


def test_hip_resize_equals_pillow(g22):
    cases = sorted(k[len("resize_"):-len("_in")] for k in g22 if k.startswith("resize_") and k.endswith("_in"))
    for c in cases:
        src, ref = g22[f"resize_{c}_in"], g22[f"resize_{c}_out"]
        got = F.resize_lanczos_u8(torch.from_numpy(src).to(DEV), (ref.shape[1], ref.shape[0]))
        assert np.array_equal(got.cpu().numpy(), ref), c


def test_llff_dataset_matches_reference(g22, scene):
    tags = _tags(g22, "train_")
    assert len(tags) == 12
    for tag in tags:
        _, spheric, idx, (w, h) = _cfg(tag)
        ds = LLFFDataset(scene, split="train", img_wh=(w, h), spheric_poses=spheric, include_idx=idx)
        assert len(ds) == int(g22[f"{tag}/len"])
        assert ds.rgb8.dtype == torch.uint8 and ds._all_rays is None          # nothing per ray until asked
        rgbs = ds.all_rgbs
        assert torch.equal(rgbs.cpu(), _unit(g22[f"train_{w}x{h}/rgb8"])), tag
        rays = ds.all_rays
        assert rays.shape == (len(ds), 9 if idx else 8)
        sel = torch.from_numpy(g22[f"{tag}/rays_sel"].astype(np.int64))
        _rays_close(rays[sel.to(DEV), :8], g22[f"{tag}/rays_rows"], tag)
        if idx:
            assert torch.equal(rays[:, 8].cpu(), torch.from_numpy(g22[f"{tag}/ids"].astype(np.float32))), tag
        s = ds[5]
        assert torch.equal(s["rays"], rays[5]) and torch.equal(s["rgbs"], rgbs[5])


def test_llff_val_and_test_samples_match_reference(g22, scene):
    tags = _tags(g22, "val_") + _tags(g22, "test")
    for tag in tags:
        split, spheric, idx, (w, h) = _cfg(tag)
        ds = LLFFDataset(scene, split=split, img_wh=(w, h), spheric_poses=spheric, include_idx=idx)
        if split == "val":
            s = ds[0]
            assert s["hw"] == (h, w) and s["c2w"].is_cuda
            assert torch.equal(s["c2w"].cpu(), torch.from_numpy(g22[f"{tag}/c2w"]))
            _rays_close(s["rays"], g22[f"{tag}/rays"], tag)
            assert torch.equal(s["rgbs"].cpu(), _unit(g22[f"{tag}/rgb8"])), tag
        else:
            ks = sorted(int(k.rsplit("_", 1)[1]) for k in g22 if k.startswith(f"{tag}/rays_"))
            assert ks
            for k in ks:
                s = ds[k]
                assert "rgbs" not in s and s["hw"] == (h, w)
                assert torch.equal(s["c2w"].cpu(), torch.from_numpy(g22[f"{tag}/c2w_{k}"]))
                _rays_close(s["rays"][::7], g22[f"{tag}/rays_{k}"], f"{tag} pose {k}")


def test_llff_private_png_decoder_path(g22, scene):
    """use_pillow=False: the package's PNG reader feeds the same bytes to the device."""
    a = LLFFDataset(scene, split="train", img_wh=(56, 42), use_pillow=False)
    assert torch.equal(a.all_rgbs.cpu(), _unit(g22["train_56x42/rgb8"]))


def test_ray_batcher_equals_dataloader(tmp_path):
    """Two full epochs on a 20-image 378 x 504 scene: RayBatcher(generator=g) yields exactly the batches of
    DataLoader(batch_size=B, shuffle=True, generator=g) over all_rays / all_rgbs, short last batch included."""
    pix, pb = make_scene(20, 378, 504, seed=7, focal=400.0)
    root = write_scene(str(tmp_path / "big"), pix, pb)
    ds = LLFFDataset(root, split="train", img_wh=(504, 378), include_idx=True)
    n, b = len(ds), 4096
    assert n % b != 0
    batcher = RayBatcher(ds, b, generator=torch.Generator().manual_seed(3))
    assert batcher.steps_per_epoch == -(-n // b)
    loader = torch.utils.data.DataLoader(range(n), batch_size=b, shuffle=True,
                                         generator=torch.Generator().manual_seed(3))
    all_rays, all_rgbs = ds.all_rays, ds.all_rgbs
    for _ in range(2):
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        steps = 0
        for (rays, rgbs), idx in zip(batcher, loader):
            idx = idx.to(DEV)
            assert rays.shape == (idx.numel(), 9) and rgbs.shape == (idx.numel(), 3)
            assert torch.equal(rays, all_rays[idx]) and torch.equal(rgbs, all_rgbs[idx])
            seen.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
            steps += 1
        assert steps == batcher.steps_per_epoch and rays.shape[0] == n % b
        assert bool((seen == 1).all())
        assert torch.equal(torch.sort(batcher.perm).values, torch.arange(n, device=DEV))


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
    """TrainStep(batcher=...) over two epochs of the g22 scene at 40 x 30, B = 1024 (every epoch ends on a short
    batch) leaves the parameters bit-identical to a TrainStep on a copy of the model driven by step(rays, rgbs) with
    the batches RayBatcher yields eagerly and the same injected draws; the batch the graph gathers equals the eager
    batch bit for bit at every step."""
    ds = LLFFDataset(scene, split="train", img_wh=(40, 30), include_idx=True)
    b = 1024
    m1, m2 = _small_model(3, precision), _small_model(3, precision)
    ts1 = TrainStep(m1, lr=1e-3, batcher=RayBatcher(ds, b, generator=torch.Generator().manual_seed(9)))
    ts2 = TrainStep(m2, lr=1e-3)
    eager = RayBatcher(ds, b, generator=torch.Generator().manual_seed(9))
    assert ts1.batcher.short_rows == len(ds) % b != 0
    g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    n_steps = 0
    for epoch in range(2):
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
    assert n_steps == 12 and len(ts1._batched) == 2          # one program per batch size, no recapture per epoch
    ts1.batcher.check()


def test_ray_batch_past_the_permutation_is_flagged(scene):
    """A gather past the end of the epoch's permutation writes NaN rows and sets the error word instead of reading
    out of bounds or wrapping; begin_epoch() reports it."""
    ds = LLFFDataset(scene, split="train", img_wh=(40, 30))
    bt = RayBatcher(ds, 1024, generator=torch.Generator().manual_seed(4))
    bt.begin_epoch()
    bt.state[0] = len(ds) - 10                       # 10 rays left; gather 1024
    bt.launch(1024)
    assert int(bt.state[0]) == len(ds) - 10 + 1024 and int(bt.state[1]) == 0
    assert not torch.isnan(bt.rays[:10]).any() and torch.isnan(bt.rays[10:1024]).all()
    assert torch.isnan(bt.rgbs[10:1024]).all()
    with pytest.raises(HN._lib.HnError, match="out of step"):
        bt.begin_epoch()


def _dp_batched_worker(port, root, q):
    import sys
    for pth in (ROOT, os.path.join(ROOT, "tests")):
        if pth not in sys.path:
            sys.path.insert(0, pth)
    import datetime
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=0, world_size=1, timeout=datetime.timedelta(seconds=120))
    try:
        ds = LLFFDataset(root, split="train", img_wh=(40, 30), include_idx=True)
        b = 1024
        ts1 = TrainStep(_small_model(3, "bf16"), lr=1e-3, force_dp=True,
                        batcher=RayBatcher(ds, b, seed=5))
        ts2 = TrainStep(_small_model(3, "bf16"), lr=1e-3, force_dp=True)
        g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
        ok = []
        for epoch in range(2):
            ts1.batcher.set_epoch(epoch)
            order = distributed_sampler_order(len(ds), 0, 1, seed=5, epoch=epoch).to(DEV)
            for k in range(ts1.batcher.steps_per_epoch):
                idx = order[k * b:(k + 1) * b]
                rays, rgbs = ds.all_rays[idx], ds.all_rgbs[idx]
                ts1.step(rng=_rng_for(idx.numel(), g1))
                ts2.step(rays, rgbs, rng=_rng_for(idx.numel(), g2))
                ok.append(torch.equal(ts1.batcher.rays[:idx.numel()], rays) and torch.equal(ts1.arena.data, ts2.arena.data))
            ts1.epoch_end()
            ts2.epoch_end()
        q.put({"ok": ok, "dp_graph": ts1.dp_graph})
    except Exception as e:          # noqa: BLE001
        q.put({"error": repr(e)})
    finally:
        dist.destroy_process_group()


def test_trainstep_with_batcher_data_parallel(scene):
    """torch.distributed (one gloo rank, force_dp): TrainStep(batcher=...) with set_epoch(e) at each epoch's start
    follows DistributedSampler's order for that epoch and matches TrainStep.step fed those batches bit for bit."""
    import multiprocessing as mp
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_batched_worker, args=(port, scene, q))
    p.start()
    res = q.get(timeout=300)
    p.join(60)
    assert "error" not in res, res
    assert len(res["ok"]) == 12 and all(res["ok"]), res


def test_batched_step_has_no_host_sync(scene):
    ds = LLFFDataset(scene, split="train", img_wh=(40, 30), include_idx=True)
    m = _small_model(4, "bf16")
    ts = TrainStep(m, lr=1e-3, batcher=RayBatcher(ds, 512, generator=torch.Generator().manual_seed(2)))
    for _ in range(3):                 # capture + first replays
        ts.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            ts.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_evaluate_images_over_val_split(g22, scene):
    from hypernerf_torch_amd.inference import evaluate_images, render_image
    m = _small_model(5, "fp32").eval()
    m.use_stratified_sampling = False
    ds = LLFFDataset(scene, split="val", img_wh=(40, 30), include_idx=True)
    res = evaluate_images(m, ds)
    assert len(res["psnrs"]) == 1 and res["images"][0].shape == (30, 40, 3)
    s = ds[0]
    img = render_image(m, s["rays"], keys=("rgb",))["rgb"]
    direct = float(-10 * torch.log10(((img - s["rgbs"]) ** 2).mean()))
    assert abs(res["psnrs"][0] - direct) <= 1e-4, (res["psnrs"][0], direct)
