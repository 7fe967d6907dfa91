"""Host side of the LLFF dataset (hypernerf_torch_amd.datasets) against the reference's LLFFDataset
(tests/golden/g22_llff.npz, tests/golden/make_dataset_golden.py): pose math, focal, bounds, val index and the render
paths of the test splits; the LANCZOS coefficient tables and fixed-point passes against Pillow's bytes; the private PNG
decoder on Pillow-written files; the per-epoch order against DataLoader's RandomSampler and DistributedSampler; and the
inputs the dataset refuses.  No GPU."""
import os
import zlib

import numpy as np
import pytest
import torch

from hypernerf_torch_amd.datasets import LLFFDataset, dataset_dict, distributed_sampler_order, random_sampler_order
from hypernerf_torch_amd.datasets import image_io
from hypernerf_torch_amd.datasets.llff import read_poses_bounds
from llff_scene import write_scene


@pytest.fixture(scope="module")
def g22(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g22_llff.npz")))


@pytest.fixture
def scene(g22, tmp_path):
    return write_scene(str(tmp_path / "scene"), g22["scene_pixels"], g22["scene_poses_bounds"])


def _tags(g22, prefix):
    """Configuration tags <split>_<s|n>_<i|x>_<W>x<H> recorded in g22 whose split starts with `prefix`."""
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


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max(initial=0.0) <= tol * max(1.0, np.abs(b).max(initial=0.0)), np.abs(a - b).max()


def test_dataset_dict():
    assert dataset_dict == {'llff': LLFFDataset}


def test_pose_math_matches_reference(g22, scene):
    tags = _tags(g22, "train_")
    assert len(tags) == 12
    for tag in tags:
        _, spheric, _, wh = _cfg(tag)
        meta = read_poses_bounds(scene, wh, spheric)
        _close(meta["focal"], g22[f"{tag}/focal"])
        _close(meta["poses"], g22[f"{tag}/poses"])
        _close(meta["pose_avg"], g22[f"{tag}/pose_avg"])
        _close(meta["bounds"], g22[f"{tag}/bounds"])
        assert (len(g22["scene_pixels"]) - 1) * wh[0] * wh[1] == int(g22[f"{tag}/len"])


def test_val_and_test_splits_match_reference(g22, scene):
    """Constructed without a device: val keeps the closest-to-centre pose, test splits carry the spiral / spheric /
    training render path; the same attributes as the reference."""
    tags = _tags(g22, "val_") + _tags(g22, "test")
    assert len(tags) == 9
    for tag in tags:
        split, spheric, idx, wh = _cfg(tag)
        ds = LLFFDataset(scene, split=split, img_wh=wh, spheric_poses=spheric, include_idx=idx)
        _close(ds.focal, g22[f"{tag}/focal"])
        _close(ds.poses, g22[f"{tag}/poses"])
        _close(ds.pose_avg, g22[f"{tag}/pose_avg"])
        _close(ds.bounds, g22[f"{tag}/bounds"])
        assert len(ds) == int(g22[f"{tag}/len"]) and ds.white_back is False
        assert [os.path.basename(p) for p in ds.image_paths] == list(g22["image_names"])
        if split == "val":
            assert np.array_equal(np.float32(ds.c2w_val), g22[f"{tag}/c2w"])
            assert ds.image_path_val.endswith(str(g22["image_names"][ds.val_idx]))
            if idx:
                assert ds.val_idx_list == [ds.val_idx]
        else:
            _close(ds.poses_test, g22[f"{tag}/poses_test"])
            assert ds.poses_test.shape == ((120, 3, 4) if split == "test" else ds.poses.shape)


def test_resize_tables_reproduce_pillow(g22):
    """Host coefficient tables + a NumPy statement of the two fixed-point passes = Pillow's LANCZOS bytes, for the
    recorded size pairs and for the training images the reference resized."""
    cases = sorted(k[len("resize_"):-len("_in")] for k in g22 if k.startswith("resize_") and k.endswith("_in"))
    assert {"up", "odd", "one_px", "row", "col", "big"} <= set(cases)
    for c in cases:
        src, ref = g22[f"resize_{c}_in"], g22[f"resize_{c}_out"]
        got = image_io.resample_u8_reference(src, (ref.shape[1], ref.shape[0]))
        assert np.array_equal(got, ref), c
    pix = g22["scene_pixels"]
    val = read_val_index(g22)
    train = [k for k in range(len(pix)) if k != val]
    for (w, h) in ((80, 60), (40, 30), (56, 42)):
        got = np.concatenate([image_io.resample_u8_reference(pix[k], (w, h)).reshape(-1, 3) for k in train])
        assert np.array_equal(got, g22[f"train_{w}x{h}/rgb8"]), (w, h)


def read_val_index(g22):
    poses = g22["val_n_x_40x30/poses"]
    return int(np.argmin(np.linalg.norm(poses[..., 3], axis=1)))


def test_lanczos_table_rounding():
    """Fixed point with 22 fraction bits, half away from zero; every output's taps sum to ~1 << 22."""
    bounds, kk, ksize = image_io.lanczos_tables(504, 126)
    assert ksize == 2 * 12 + 1 and kk.dtype == np.int32 and bounds.shape == (126, 2)
    assert (np.abs(kk.sum(1) - (1 << 22)) <= ksize).all()
    assert ((bounds[:, 0] + bounds[:, 1]) <= 504).all()
    w, _ = image_io.lanczos_weights(504, 126)
    lo, ws = w[3]
    for t, v in enumerate(ws):
        x = v * (1 << 22)
        assert kk[3, t] == (int(x + 0.5) if v >= 0 else int(x - 0.5))


def _png_filters(data: bytes):
    import struct
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBB", data[pos + 8:pos + 18])
        elif tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, _, colour = hdr
    stride = w * {0: 1, 2: 3, 4: 2, 6: 4}[colour] + 1
    raw = zlib.decompress(idat)
    return {raw[y * stride] for y in range(h)}


def test_private_png_decoder_reads_pillow_files(g22, tmp_path):
    keys = sorted(k for k in g22 if k.startswith("png_") and not k.endswith("_pixels"))
    seen = set()
    for k in keys:
        data = g22[k].tobytes()
        seen |= _png_filters(data)
        assert np.array_equal(image_io.decode_png_rgb8(data), g22[k + "_pixels"]), k
        p = tmp_path / f"{k}.png"
        p.write_bytes(data)
        assert np.array_equal(image_io.load_rgb8(str(p), use_pillow=False), g22[k + "_pixels"]), k
    assert seen == {0, 1, 2, 3, 4}, seen


def test_jpeg_without_pillow_is_refused(tmp_path):
    p = tmp_path / "a.jpg"
    p.write_bytes(b"\xff\xd8\xff\xe0" + b"\0" * 32)
    with pytest.raises(ValueError, match="JPEG"):
        image_io.load_rgb8(str(p), use_pillow=False)


@pytest.mark.parametrize("n", [1, 7, 1001])
def test_random_sampler_order_matches_dataloader(n):
    """Two epochs of DataLoader(shuffle=True, generator=g), with and without a generator, index for index."""
    for seeded in (True, False):
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(11) if seeded else None
        loader = torch.utils.data.DataLoader(range(n), batch_size=64, shuffle=True, generator=g)
        ref = [torch.cat(list(loader)) for _ in range(2)]
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(11) if seeded else None
        mine = [random_sampler_order(n, g) for _ in range(2)]
        for a, b in zip(ref, mine):
            assert torch.equal(a, b)


@pytest.mark.parametrize("n", [9, 1001])
def test_distributed_sampler_order(n):
    from torch.utils.data.distributed import DistributedSampler
    for epoch in (0, 3):
        for rank in (0, 1):
            s = DistributedSampler(range(n), num_replicas=2, rank=rank, shuffle=True, seed=4, drop_last=False)
            s.set_epoch(epoch)
            assert list(s) == distributed_sampler_order(n, rank, 2, seed=4, epoch=epoch).tolist()
    s = DistributedSampler(range(2), num_replicas=5, rank=3, shuffle=True, seed=0)      # padding past n
    assert list(s) == distributed_sampler_order(2, 3, 5).tolist()


def test_refusals(g22, scene, tmp_path):
    with pytest.raises(ValueError, match="aspect ratio"):
        LLFFDataset(scene, split="val", img_wh=(50, 30))
    with pytest.raises(ValueError, match="include_idx"):
        LLFFDataset(scene, split="test", img_wh=(40, 30), include_idx=True)
    with pytest.raises(ValueError, match="include_idx"):
        LLFFDataset(scene, split="test_train", img_wh=(40, 30), include_idx=True)
    os.remove(os.path.join(scene, "images", "img_005.png"))
    for split in ("train", "val"):
        with pytest.raises(ValueError, match="Mismatch between number of images and number of poses"):
            LLFFDataset(scene, split=split, img_wh=(40, 30))
    LLFFDataset(scene, split="test", img_wh=(40, 30))          # the test splits read no image
    # an image whose aspect differs from img_wh is refused before anything reaches a device
    odd = write_scene(str(tmp_path / "odd"), g22["scene_pixels"], g22["scene_poses_bounds"])
    from hypernerf_torch_amd.inference import write_png
    write_png(os.path.join(odd, "images", "img_002.png"), g22["scene_pixels"][2][:, :70])
    with pytest.raises(ValueError, match="different aspect ratio"):
        LLFFDataset(odd, split="train", img_wh=(40, 30), device="cpu")
