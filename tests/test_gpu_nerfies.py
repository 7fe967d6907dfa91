"""GPU tests (MI355X) of the device-resident Nerfies-format dataset: the rays of hn_generate_rays_nerfies against the
float64 statement of the camera model recorded in g24 (two scenes, one odd in both dimensions; cameras without, with
realistic and with strong distortion), all_rgbs bit for bit, RayBatcher's gather against all_rays / all_rgbs bit for
bit (both kernels inline one device function) and against a shuffled DataLoader's order, the bounds check of the
gather, TrainStep(batcher=...) against TrainStep.step fed the same batches, no host sync and no extra launch in a
batched step, evaluate_images over the val split, the test split, and the C-ABI's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import nerfies_scene as NS
from gpu_common import DEV, EMB, load_hash
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.datasets import LLFFDataset, NerfiesDataset, RayBatcher
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.training import TrainStep

pytestmark = pytest.mark.gpu
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
ROW_STEP = 7
NS_SAMPLES = 32          # samples per level: a multiple of 32 keeps the whole gradient of a step bit-reproducible


@pytest.fixture(scope="module")
def g24(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g24_nerfies.npz")))


@pytest.fixture(scope="module")
def roots(g24, tmp_path_factory):
    """{'a': the 24 x 16 capture (5 train images: 1920 rays), 'b': the 67 x 41 one}, written from g24."""
    out = {}
    for name in ("a", "b"):
        scene = NS.scene_from_arrays({k.split("/", 1)[1]: v for k, v in g24.items() if k.startswith(name + "/")})
        out[name] = NS.write_scene(str(tmp_path_factory.mktemp("g24" + name)), scene)
    return out


@pytest.fixture(scope="module")
def train_a(roots):
    """Scene a's train split with all_rays / all_rgbs built: shared, and left unchanged, by the tests below."""
    ds = NerfiesDataset(roots["a"], split="train", image_scale=2)
    ds.all_rays, ds.all_rgbs
    return ds


def _rays_close(got, ref, what):
    """The project's ray bound (test_gpu_datasets.py, test_gpu_blender.py): 2e-6 of the rows' scale.  The same
    arithmetic in float32 NumPy is within 1.1e-7 of float64.  Columns 6 to 8 (near, far, id) are compared exactly."""
    got = got.detach().cpu()
    ref64 = torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err = (got.double() - ref64).abs().max().item()
    print(f"{what}: max |rays - f64| = {err:.3e} (bound {2e-6 * max(1.0, ref64.abs().max().item()):.3e})")
    assert err <= 2e-6 * max(1.0, ref64.abs().max().item()), (what, err)
    assert torch.equal(got[:, 6:], ref64[:, 6:].float()), what


def test_rays_match_the_float64_statement(g24, roots):
    for name, (w, h) in (("a", (24, 16)), ("b", (67, 41))):
        ds = NerfiesDataset(roots[name], split="train", image_scale=2)
        assert ds.img_wh == (w, h) and ds.ray_cols == 9 and ds._all_rays is None
        assert ds.rgb8.dtype == torch.uint8 and ds.rgb8.is_cuda and tuple(ds.rgb8.shape) == (len(ds.ids), h, w, 3)
        rays = ds.all_rays
        assert rays.dtype == torch.float32 and rays.shape == (len(ds), 9) == (len(ds.ids) * h * w, 9)
        _rays_close(rays[::ROW_STEP], g24[f"{name}/train_rows"], f"{name} train")
        assert torch.equal(rays[::h * w, 8].cpu(), torch.tensor(ds.metadata_ids, dtype=torch.float32))
        norm = rays[:, 3:6].double().norm(dim=1)
        assert float((norm - 1).abs().max()) <= 2e-7
        smp = ds[5]
        assert torch.equal(smp["rays"], rays[5]) and torch.equal(smp["rgbs"], ds.all_rgbs[5])
        val = NerfiesDataset(roots[name], split="val", image_scale=2)
        got = torch.cat([val[k]["rays"] for k in range(len(val))], 0)
        _rays_close(got[::ROW_STEP], g24[f"{name}/val_rows"], f"{name} val")
        # 8 columns and another metadata key: the same first eight columns, another id
        plain = NerfiesDataset(roots[name], split="train", image_scale=2, include_idx=False)
        assert plain.ray_cols == 8 and torch.equal(plain.all_rays, rays[:, :8])
        app = NerfiesDataset(roots[name], split="train", image_scale=2, metadata_key="appearance_id", use_pillow=False)
        assert torch.equal(app.all_rays[:, :8], rays[:, :8]) and torch.equal(app.rgb8, ds.rgb8)
        assert app.all_rays[::h * w, 8].tolist() == [float(v) for v in app.metadata_ids] != ds.metadata_ids


def test_all_rgbs_is_u8_over_255(g24, train_a):
    ids = [str(i) for i in g24["a/ids"]]
    pix = np.concatenate([g24["a/pixels"][ids.index(i)].reshape(-1, 3) for i in train_a.ids])
    ref = torch.from_numpy(pix).float().div(255)
    assert train_a.all_rgbs.dtype == torch.float32 and torch.equal(train_a.all_rgbs.cpu(), ref)


def test_gather_and_whole_image_launch_share_one_device_function(train_a):
    """RayBatcher(ds, 100) over the 1920-ray scene: 20 steps, the last short, every batch bit for bit the rows of
    all_rays / all_rgbs at the permutation."""
    bt = RayBatcher(train_a, 100, generator=torch.Generator().manual_seed(6))
    assert bt.steps_per_epoch == 20 and bt.short_rows == 20
    steps = 0
    seen = torch.zeros(len(train_a), dtype=torch.int32, device=DEV)
    for k, (rays, rgbs) in enumerate(bt):
        idx = bt.perm[100 * k:100 * k + 100]
        assert rays.shape == (idx.numel(), 9) and rgbs.shape == (idx.numel(), 3)
        assert torch.equal(rays, train_a.all_rays[idx]) and torch.equal(rgbs, train_a.all_rgbs[idx]), k
        seen.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
        steps += 1
    assert steps == 20 and rays.shape[0] == 20 and bool((seen == 1).all())
    bt.check()


def test_ray_batcher_equals_dataloader(train_a):
    """Two epochs: the batches of DataLoader(batch_size=B, shuffle=True, generator=g) over all_rays / all_rgbs."""
    n, b = len(train_a), 256
    bt = RayBatcher(train_a, b, generator=torch.Generator().manual_seed(3))
    loader = torch.utils.data.DataLoader(range(n), batch_size=b, shuffle=True,
                                         generator=torch.Generator().manual_seed(3))
    for _ in range(2):
        steps = 0
        for (rays, rgbs), idx in zip(bt, loader):
            idx = idx.to(DEV)
            assert torch.equal(rays, train_a.all_rays[idx]) and torch.equal(rgbs, train_a.all_rgbs[idx])
            steps += 1
        assert steps == bt.steps_per_epoch == 8 and rays.shape[0] == n % b == 128
        assert torch.equal(torch.sort(bt.perm).values, torch.arange(n, device=DEV))
    bt.check()


def test_gather_past_the_permutation_is_flagged(train_a):
    """A cursor pushed past the end of the epoch's permutation writes NaN rows and sets the error word instead of
    reading out of bounds; check() reports it.  (The kernel's bounds check is what is under test: nothing faults.)"""
    n = len(train_a)
    bt = RayBatcher(train_a, 256, generator=torch.Generator().manual_seed(4))
    bt.begin_epoch()
    bt.launch(256)
    assert int(bt.state[0]) == 256 and int(bt.state[2]) == 0 and not torch.isnan(bt.rays).any()
    bt.state[0] = n - 10                             # 10 rays left; gather 256
    bt.launch(256)
    assert int(bt.state[0]) == n - 10 + 256 and int(bt.state[1]) == 0 and int(bt.state[2]) == 1
    idx = bt.perm[n - 10:]
    assert torch.equal(bt.rays[:10], train_a.all_rays[idx]) and torch.equal(bt.rgbs[:10], train_a.all_rgbs[idx])
    assert torch.isnan(bt.rays[10:256]).all() and torch.isnan(bt.rgbs[10:256]).all()
    with pytest.raises(HN._lib.HnError, match="out of step"):
        bt.check()
    # an index outside the dataset inside the permutation is refused the same way
    bt.state.zero_()
    bt.perm[3] = n
    bt.perm[5] = -1
    bt.launch(256)
    bad = torch.isnan(bt.rays).any(1)
    assert bad.nonzero().flatten().tolist() == [3, 5] and int(bt.state[2]) == 1
    assert torch.isnan(bt.rgbs[[3, 5]]).all() and not torch.isnan(bt.rgbs[bad.logical_not()]).any()


def _model_for(ds, seed, precision):
    """near / far from the scene, GLO tables sized from the capture's metadata."""
    HN.set_precision(precision)
    emb = {"warp": list(range(ds.num_embeddings["warp"])), "camera": list(range(ds.num_embeddings["camera"])),
           "appearance": list(range(ds.num_embeddings["appearance"])), "time": list(range(ds.num_embeddings["warp"]))}
    m = models.NerfModel(emb, near=ds.near, far=ds.far, n_samples_coarse=NS_SAMPLES, n_samples_fine=NS_SAMPLES,
                         noise_std=None, **KW)
    load_hash(m, seed)
    return m.to(DEV)


def _rng_for(rows, gen):
    return {"t_rand": torch.rand((rows, NS_SAMPLES), generator=gen).to(DEV),
            "u": torch.rand((rows, NS_SAMPLES), generator=gen).to(DEV)}


def test_trainstep_with_batcher_matches_step(train_a):
    """Three steps of TrainStep(batcher=RayBatcher(ds, 96)) leave the parameters bit-identical to a TrainStep on a
    copy of the model driven by step(rays, rgbs) with the batches RayBatcher yields eagerly and the same injected
    draws (the comparison, and its tolerance of none, of the LLFF and Blender tests)."""
    m1, m2 = _model_for(train_a, 3, "fp32"), _model_for(train_a, 3, "fp32")
    ts1 = TrainStep(m1, lr=1e-3, batcher=RayBatcher(train_a, 96, generator=torch.Generator().manual_seed(9)))
    ts2 = TrainStep(m2, lr=1e-3)
    eager = RayBatcher(train_a, 96, generator=torch.Generator().manual_seed(9))
    g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    before = ts1.arena.data.clone()
    for k, (rays, rgbs) in zip(range(3), eager):
        l1 = ts1.step(rng=_rng_for(96, g1))
        assert torch.equal(ts1.batcher.rays, rays) and torch.equal(ts1.batcher.rgbs, rgbs)
        l2 = ts2.step(rays.clone(), rgbs.clone(), rng=_rng_for(96, g2))
        assert torch.isfinite(l1["train/loss"]).all() and torch.equal(l1["train/loss"], l2["train/loss"]), k
        assert torch.equal(ts1.arena.data, ts2.arena.data), k
    assert not torch.equal(ts1.arena.data, before) and len(ts1._batched) == 1
    ts1.batcher.check()


def _captured_launches(monkeypatch, ts):
    """Names of the C-ABI launches in the program that the first step() call captures (test_gpu_blender.py): the
    launches from the last gather on."""
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


def test_batched_step_has_no_host_sync_and_no_extra_launch(train_a, tmp_path, monkeypatch):
    """The batched step over a Nerfies capture replays without a host sync, and its program holds the launches of the
    same step over an LLFF dataset of the same batch size and ray width — the camera model lives in the gather."""
    from llff_scene import make_scene as llff_make, write_scene as llff_write
    llff = LLFFDataset(llff_write(str(tmp_path / "llff"), *llff_make(6, 30, 40)), split="train", img_wh=(40, 30),
                       include_idx=True)
    assert train_a.ray_cols == llff.ray_cols == 9
    launches = {}
    for name, ds in (("nerfies", train_a), ("llff", llff)):
        if name == "nerfies":
            m = _model_for(ds, 4, "bf16")
        else:
            HN.set_precision("bf16")
            m = models.NerfModel(EMB, n_samples_coarse=NS_SAMPLES, n_samples_fine=NS_SAMPLES, noise_std=None, **KW)
            load_hash(m, 4)
            m = m.to(DEV)
        ts = TrainStep(m, lr=1e-3, batcher=RayBatcher(ds, 96, generator=torch.Generator().manual_seed(2)))
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
    assert launches["nerfies"][0] == "hn_ray_batch_nerfies" and launches["llff"][0] == "hn_ray_batch"
    assert "hn_generate_rays_nerfies" not in launches["nerfies"] and len(launches["nerfies"]) > 10
    assert launches["nerfies"][1:] == launches["llff"][1:]


def test_evaluate_images_over_val_split_and_test_split(g24, roots, train_a):
    from hypernerf_torch_amd.inference import evaluate_images
    m = _model_for(train_a, 5, "fp32").eval()
    m.use_stratified_sampling = False
    val = NerfiesDataset(roots["a"], split="val", image_scale=2)
    res = evaluate_images(m, val)
    assert len(res["psnrs"]) == 2 and all(np.isfinite(p) for p in res["psnrs"])
    assert all(img.shape == (16, 24, 3) for img in res["images"])
    ids = [str(i) for i in g24["a/ids"]]
    for k, i in enumerate(val.ids):
        s = val[k]
        assert s["hw"] == (16, 24) and s["rays"].shape == (384, 9) and s["rgbs"].shape == (384, 3)
        assert torch.equal(s["rgbs"].cpu(), torch.from_numpy(g24["a/pixels"][ids.index(i)].reshape(-1, 3)).float() / 255)
    test = NerfiesDataset(roots["a"], split="test", image_scale=2, camera_path=NS.CAMERA_PATH, test_id=4)
    samples = [test[k] for k in range(len(test))]
    assert len(samples) == 3 and all("rgbs" not in s and s["rays"].shape == (384, 9) for s in samples)
    assert all(bool((s["rays"][:, 8] == 4).all()) for s in samples)
    ref = g24["a/test_rows"].copy()
    ref[:, 8] = 4                                       # g24's test rows carry test_id 0
    _rays_close(torch.cat([s["rays"] for s in samples], 0)[::ROW_STEP], ref, "a test")
    with pytest.raises(IndexError):
        test[3]


def test_c_abi_argument_errors(train_a):
    """row_floats of 7, a null camera table and n_rays that is no multiple of H*W return -2 / -3 / -2 without
    launching: the buffers keep their contents and the cursor stays."""
    lib = HN._lib.load()
    L = HN._lib
    ds = train_a
    w, h = ds.img_wh
    perm = torch.arange(len(ds), dtype=torch.int64, device=DEV)
    state = torch.zeros(3, dtype=torch.int64, device=DEV)
    rays = torch.full((64, 9), 7.0, device=DEV)
    rgbs = torch.full((64, 3), 7.0, device=DEV)
    image = torch.full((h * w, 9), 7.0, device=DEV)

    def batch(cams=ds.cams, n_rays=len(ds), row_floats=9):
        return lib.hn_ray_batch_nerfies(L.ptr(perm), C.c_longlong(perm.numel()), L.ptr(state), C.c_int(64),
                                        C.c_longlong(n_rays), C.c_int(h), C.c_int(w), L.ptr(cams), L.ptr(ds.image_ids),
                                        C.c_float(ds.near), C.c_float(ds.far), C.c_int(row_floats), L.ptr(ds.rgb8),
                                        L.ptr(rays), L.ptr(rgbs), L.stream_handle())

    def whole(cam=ds.cams[0], row_floats=9):
        return lib.hn_generate_rays_nerfies(C.c_int(h), C.c_int(w), L.ptr(cam), C.c_float(ds.near), C.c_float(ds.far),
                                            C.c_float(0.0), C.c_int(row_floats), L.ptr(image), L.stream_handle())
    assert batch(row_floats=7) == -2 and batch(cams=None) == -3 and batch(n_rays=len(ds) - 1) == -2
    assert whole(row_floats=7) == -2 and whole(cam=None) == -3
    torch.cuda.synchronize()
    assert bool((rays == 7).all()) and bool((rgbs == 7).all()) and bool((image == 7).all())
    assert state.tolist() == [0, 0, 0]
    assert batch() == 0
    torch.cuda.synchronize()
    assert state.tolist() == [64, 0, 0] and torch.equal(rays, ds.all_rays[:64]) and torch.equal(rgbs, ds.all_rgbs[:64])
    with pytest.raises(HN._lib.HnError, match="bad shapes"):
        F.ray_batch_nerfies(perm, state, 64, h, w, ds.cams[:, :12].contiguous(), ds.rgb8, rays, rgbs, ds.near, ds.far,
                            image_ids=ds.image_ids)
