"""Host-side tests of the Nerfies-format dataset (no GPU): parsing, camera scaling and recentring, the id column by
metadata key, num_embeddings, every ValueError of the loader, and the float64 statement of the camera model that the
GPU tests measure the kernels against — guarded by the closed-form forward projection, and equal to the rows in g24."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import nerfies_scene as NS
from hypernerf_torch_amd.datasets import NerfiesDataset, available_datasets, dataset_dict, dataset_names, nerfies

ROW_STEP = 7


@pytest.fixture(scope="module")
def g24(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g24_nerfies.npz")))


def _scene(g24, name):
    return NS.scene_from_arrays({k.split("/", 1)[1]: v for k, v in g24.items() if k.startswith(name + "/")})


@pytest.fixture(scope="module")
def scene_a(g24):
    return _scene(g24, "a")


@pytest.fixture(scope="module")
def root_a(scene_a, tmp_path_factory):
    return NS.write_scene(str(tmp_path_factory.mktemp("g24a")), scene_a)


@pytest.fixture()
def broken(root_a, tmp_path):
    """A private copy of scene a for a test to damage."""
    return shutil.copytree(root_a, str(tmp_path / "broken"))


def test_fixture_is_what_make_scene_writes(g24, scene_a):
    """g24 holds make_scene's output (the generator is reproducible), with the cameras the tests rely on."""
    fresh = NS.scene_to_arrays(NS.make_scene(24))
    for k, v in fresh.items():
        assert np.array_equal(v, g24[f"a/{k}"]), k
    cams = [scene_a["cameras"][i] for i in scene_a["ids"]]
    assert not any(cams[0]["radial_distortion"]) and not any(cams[0]["tangential_distortion"])
    assert cams[1]["radial_distortion"] == [-0.2, 0.05, 0.0] and cams[1]["tangential_distortion"] == [0.01, -0.01]
    assert cams[1]["skew"] == 0.3 and cams[1]["pixel_aspect_ratio"] == 1.02
    assert all(abs(c["radial_distortion"][0] - 0.04) < 0.01 and abs(c["radial_distortion"][1] + 0.10) < 0.025
               for c in cams[2:])
    assert scene_a["ids"][0] in scene_a["train_ids"] and scene_a["ids"][1] in scene_a["train_ids"]
    for key in ("ids", "train_ids", "val_ids"):          # a positional index is not the warp id, in any list
        assert all(scene_a["metadata"][i]["warp_id"] != k for k, i in enumerate(scene_a[key]))
    assert g24["b/pixels"].shape[1:] == (41, 67, 3) and len(g24["b/train_ids"]) == 3 and len(g24["b/val_ids"]) == 1


def test_dataset_dict_has_nerfies():
    assert dataset_dict['nerfies'] is NerfiesDataset
    assert available_datasets() == ['blender', 'llff', 'nerfies'] and set(dataset_names()) < set(available_datasets())
    with pytest.raises(KeyError):
        dataset_dict['dtu']


def test_parsing_scaling_and_recentring(scene_a, root_a):
    ds = NerfiesDataset(root_a, split="train", image_scale=2, device="cpu")
    assert (ds.near, ds.far) == (0.05, 1.9) and np.array_equal(ds.bounds, [0.05, 1.9]) and ds.white_back is False
    assert ds.img_wh == (24, 16) and ds.ids == scene_a["train_ids"] and len(ds) == ds.n_rays == 5 * 24 * 16
    assert ds.ray_cols == 9 and NerfiesDataset(root_a, split="val", image_scale=2, include_idx=False).ray_cols == 8
    assert ds.rgb8.dtype == torch.uint8 and tuple(ds.rgb8.shape) == (5, 16, 24, 3)
    assert np.array_equal(ds.rgb8.numpy(), np.stack([scene_a["pixels"][i] for i in scene_a["train_ids"]]))
    assert ds._all_rays is None and ds._all_rgbs is None
    assert ds.c2w is ds.cams and tuple(ds.cams.shape) == (5, 24) and ds.cams.dtype == torch.float32
    for k, i in enumerate(scene_a["train_ids"]):
        raw, cam = scene_a["cameras"][i], ds.cameras[k]
        assert cam["focal_length"] == raw["focal_length"] * 0.5
        assert np.array_equal(cam["principal_point"], np.array(raw["principal_point"]) * 0.5)
        assert cam["image_size"] == (24, 16) and raw["image_size"] == [48, 32]
        assert cam["skew"] == raw["skew"] and cam["pixel_aspect_ratio"] == raw["pixel_aspect_ratio"]
        assert np.array_equal(cam["radial_distortion"], raw["radial_distortion"])
        assert np.array_equal(cam["tangential_distortion"], raw["tangential_distortion"])
        assert np.array_equal(cam["orientation"], np.array(raw["orientation"]))
        assert np.array_equal(cam["position"], (np.array(raw["position"]) - np.array([0.4, -0.2, 1.1])) * 0.37)
        want = NS.scaled_camera(raw, 2, scene_a["scene"])
        rec = ds.cams[k].numpy()
        assert rec.shape == (24,) and np.array_equal(rec[22:], [0, 0])
        flat = np.concatenate([want["orientation"].reshape(-1), want["position"], [want["focal_length"],
                               want["pixel_aspect_ratio"], want["skew"]], want["principal_point"],
                               want["radial_distortion"], want["tangential_distortion"]])
        assert np.array_equal(rec[:22], flat.astype(np.float32))
    # image_size rounds (Python's round, as the Nerfies camera does)
    cam = nerfies.load_camera(os.path.join(root_a, "camera", scene_a["ids"][0] + ".json"), image_scale=5)
    assert cam["image_size"] == (round(48 / 5), round(32 / 5)) == (10, 6)


def test_ids_by_metadata_key_and_num_embeddings(scene_a, root_a):
    md = scene_a["metadata"]
    for key in ("warp_id", "appearance_id", "camera_id"):
        for split in ("train", "val"):
            ds = NerfiesDataset(root_a, split=split, image_scale=2, metadata_key=key, device="cpu")
            assert ds.metadata_ids == [md[i][key] for i in scene_a[f"{split}_ids"]]
    ds = NerfiesDataset(root_a, split="train", image_scale=2, device="cpu")
    assert ds.image_ids.dtype == torch.float32 and ds.image_ids.tolist() == [float(v) for v in ds.metadata_ids]
    assert ds.num_embeddings == {k: max(m[k + "_id"] for m in md.values()) + 1
                                 for k in ("warp", "appearance", "camera")}
    assert ds.num_embeddings["warp"] == 2 * 7 and ds.num_embeddings["camera"] == 2
    with pytest.raises(ValueError, match="metadata_key"):
        NerfiesDataset(root_a, split="train", image_scale=2, metadata_key="time_id", device="cpu")
    with pytest.raises(ValueError, match="split"):
        NerfiesDataset(root_a, split="trainval", image_scale=2, device="cpu")


def test_val_and_test_splits_on_the_host(scene_a, root_a):
    """The val / test constructors touch no device."""
    val = NerfiesDataset(root_a, split="val", image_scale=2)
    test = NerfiesDataset(root_a, split="test", image_scale=2, camera_path=NS.CAMERA_PATH, test_id=4)
    assert len(val) == 2 and val.ids == scene_a["val_ids"] and len(test) == 3 and test.metadata_ids == [4, 4, 4]
    assert test.ids == ["000000", "000001", "000002"] and test.img_wh == val.img_wh == (24, 16)
    assert np.array_equal(test.cameras[1]["orientation"], np.array(scene_a["camera_path"][1]["orientation"]))
    for ds in (val, test):
        with pytest.raises(IndexError):
            ds[len(ds)]
        with pytest.raises(AttributeError):
            ds.all_rays
    with pytest.raises(ValueError, match="camera_path"):
        NerfiesDataset(root_a, split="test", image_scale=2)
    with pytest.raises(ValueError, match="camera-paths.*nowhere"):
        NerfiesDataset(root_a, split="test", image_scale=2, camera_path="nowhere")


def _rewrite(path, fn):
    with open(path) as f:
        obj = json.load(f)
    fn(obj)
    with open(path, "w") as f:
        json.dump(obj, f)


def test_image_of_another_size_is_refused_before_any_upload(scene_a, broken, monkeypatch):
    """The last training image is 23 x 16: the ValueError names it, and no image was decoded before it was raised."""
    last = scene_a["train_ids"][-1]
    path = os.path.join(broken, "rgb", "2x", last + ".png")
    NS.write_png_rgb(path, scene_a["pixels"][last][:, :23])
    decoded = []
    real = nerfies.image_io.load_rgb8
    monkeypatch.setattr(nerfies.image_io, "load_rgb8", lambda p, **kw: decoded.append(p) or real(p, **kw))
    for use_pillow in (True, False):
        with pytest.raises(ValueError, match=last + r"\.png is 23 x 16.*24 x 16"):
            NerfiesDataset(broken, split="train", image_scale=2, device="cpu", use_pillow=use_pillow)
    assert decoded == []
    os.remove(path)
    with pytest.raises(ValueError, match=last + r"\.png is missing"):
        NerfiesDataset(broken, split="train", image_scale=2, device="cpu")


def test_mixed_image_sizes_within_a_split_are_refused(scene_a, broken):
    bad = scene_a["val_ids"][1]
    _rewrite(os.path.join(broken, "camera", bad + ".json"), lambda c: c.update(image_size=[48, 36]))
    with pytest.raises(ValueError, match=bad + r"\.json: image_size \(24, 18\) differs"):
        NerfiesDataset(broken, split="val", image_scale=2)
    NerfiesDataset(broken, split="train", image_scale=2, device="cpu")          # the train split is intact


def test_id_without_metadata_or_camera_is_refused(scene_a, broken):
    tid, vid = scene_a["train_ids"][2], scene_a["val_ids"][0]
    os.remove(os.path.join(broken, "camera", vid + ".json"))
    with pytest.raises(ValueError, match=r"camera.*" + vid + r"\.json is missing"):
        NerfiesDataset(broken, split="val", image_scale=2)
    _rewrite(os.path.join(broken, "metadata.json"), lambda m: m.pop(tid))
    with pytest.raises(ValueError, match=r"metadata\.json has no 'warp_id' for id '" + tid + "'"):
        NerfiesDataset(broken, split="train", image_scale=2, device="cpu")
    _rewrite(os.path.join(broken, "metadata.json"), lambda m: m.update({tid: {"appearance_id": 1}}))
    with pytest.raises(ValueError, match=r"metadata\.json has no 'warp_id'"):
        NerfiesDataset(broken, split="train", image_scale=2, device="cpu")


def test_missing_files_and_scale_folder_are_refused(broken):
    with pytest.raises(ValueError, match=r"rgb.4x is missing"):
        NerfiesDataset(broken, split="train", device="cpu")                       # image_scale defaults to 4
    _rewrite(os.path.join(broken, "scene.json"), lambda s: s.pop("near"))
    with pytest.raises(ValueError, match=r"scene\.json: 'near' is missing"):
        NerfiesDataset(broken, split="train", image_scale=2, device="cpu")
    _rewrite(os.path.join(broken, "scene.json"), lambda s: s.update(near=0.05))
    os.remove(os.path.join(broken, "dataset.json"))
    with pytest.raises(ValueError, match=r"dataset\.json is missing"):
        NerfiesDataset(broken, split="train", image_scale=2, device="cpu")


def test_restatement_reprojects_every_pixel_centre(g24):
    """rays_f64 (Newton undistortion) followed by project_f64 (closed-form distortion) returns every pixel centre of
    every camera of both scenes to within 1e-9 px, at three depths along the ray."""
    for name in ("a", "b"):
        scene = _scene(g24, name)
        for split in ("train", "val", "test"):
            for cam, _ in NS.split_cameras(scene, split):
                rows = NS.rays_f64(cam, 0.0, 1.0)
                w, h = cam["image_size"]
                j, i = np.mgrid[0:h, 0:w]
                centres = np.stack([i.reshape(-1) + 0.5, j.reshape(-1) + 0.5], -1)
                assert np.allclose(np.linalg.norm(rows[:, 3:6], axis=1), 1.0, rtol=0, atol=1e-15)
                for depth in (0.05, 1.7, 40.0):
                    err = np.abs(NS.project_f64(cam, rows[:, :3] + depth * rows[:, 3:6]) - centres).max()
                    assert err <= 1e-9, (name, split, depth, err)


def test_restatement_reproduces_g24_exactly(g24):
    for name in ("a", "b"):
        scene = _scene(g24, name)
        for split in ("train", "val", "test"):
            rows = NS.split_rays_f64(scene, split)
            assert rows.dtype == np.float64 and rows.shape[1] == 9
            assert np.array_equal(rows[::ROW_STEP], g24[f"{name}/{split}_rows"]), (name, split)
        ids = [scene["metadata"][i]["warp_id"] for i in scene["train_ids"]]
        hw = g24[f"{name}/pixels"].shape[1] * g24[f"{name}/pixels"].shape[2]
        assert np.array_equal(NS.split_rays_f64(scene, "train")[::hw, 8], ids)
