"""Host side of the Blender dataset (hypernerf_torch_amd.datasets.blender) against the reference's BlenderDataset
(tests/golden/g23_blender.npz, tests/golden/make_blender_golden.py): the NumPy statement of Pillow's RGBA LANCZOS resize
against Pillow's bytes, the private PNG reader on Pillow-written RGBA files and the files it refuses, focal and poses
from the JSON, and the inputs the dataset refuses.  No GPU."""
import os

import numpy as np
import pytest

from blender_scene import make_scene, write_png_rgba, write_scene
from hypernerf_torch_amd.datasets import BlenderDataset, dataset_dict, image_io
from hypernerf_torch_amd.datasets.blender import read_transforms

SIZES = (64, 32, 24, 80)
RESIZE_CASES = ("alpha0", "alpha255", "down", "odd", "one_axis", "same", "up")


@pytest.fixture(scope="module")
def g23(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g23_blender.npz")))


@pytest.fixture
def scene(g23, tmp_path):
    return write_scene(str(tmp_path / "scene"), {s: (g23[f"scene_{s}_pixels"], g23[f"scene_{s}_poses"])
                                                 for s in ("train", "val", "test")})


def test_scene_writer_is_the_recorded_scene(g23):
    """The seeded writer still produces the scene the golden data was recorded on."""
    for split, (pix, poses) in make_scene().items():
        assert np.array_equal(pix, g23[f"scene_{split}_pixels"]) and np.array_equal(poses, g23[f"scene_{split}_poses"])
    pix = g23["scene_train_pixels"]
    assert pix.shape == (5, 64, 64, 4) and g23["scene_val_pixels"].shape[0] == 8 and g23["scene_test_pixels"].shape[0] == 3
    assert (pix[..., :3][pix[..., 3] == 0] > 0).all()          # colour under alpha == 0, which a resize must not leak


def test_rgba_resize_reference_equals_pillow(g23):
    cases = sorted(k[len("resize_"):-len("_in")] for k in g23 if k.startswith("resize_") and k.endswith("_in"))
    assert tuple(cases) == RESIZE_CASES
    for c in cases:
        src, ref = g23[f"resize_{c}_in"], g23[f"resize_{c}_out"]
        got = image_io.resample_rgba8_reference(src, (ref.shape[1], ref.shape[0]))
        assert got.dtype == np.uint8 and np.array_equal(got, ref), c
    # the premultiplied path is not the four channels resampled alone, and equal size is a copy, not a round trip
    src, ref = g23["resize_down_in"], g23["resize_down_out"]
    assert not np.array_equal(image_io.resample_u8_reference(src, (32, 32)), ref)
    same = g23["resize_same_in"]
    assert np.array_equal(g23["resize_same_out"], same)
    assert not np.array_equal(image_io.unpremultiply_u8_reference(image_io.premultiply_u8_reference(same)), same)


def test_rgba_resize_reference_against_installed_pillow(g23):
    """Where Pillow is installed, its resize today equals the recorded bytes' restatement on the scene's own images."""
    if not image_io.have_pillow():
        pytest.skip("Pillow is not installed")
    from PIL import Image
    img = g23["scene_train_pixels"][0]
    for s in (32, 24, 80):
        ref = np.asarray(Image.fromarray(img, "RGBA").resize((s, s), Image.Resampling.LANCZOS))
        assert np.array_equal(image_io.resample_rgba8_reference(img, (s, s)), ref), s


def test_private_png_reader_keeps_alpha(g23, tmp_path):
    n_rgba = 0
    for k in range(4):
        data = g23[f"png_{k}"].tobytes()
        path = str(tmp_path / f"f{k}.png")
        with open(path, "wb") as f:
            f.write(data)
        if f"png_{k}_pixels" in g23:
            n_rgba += 1
            assert np.array_equal(image_io.decode_png_rgba8(data), g23[f"png_{k}_pixels"])
            for use_pillow in (False, True):
                got = image_io.load_rgba8(path, use_pillow=use_pillow)
                assert got.shape[2] == 4 and np.array_equal(got, g23[f"png_{k}_pixels"])
            assert np.array_equal(image_io.load_rgb8(path, use_pillow=False), g23[f"png_{k}_pixels"][..., :3])
        else:
            assert str(g23[f"png_{k}_mode"]) in ("RGB", "L")
            for use_pillow in (False, True):
                with pytest.raises(ValueError, match=f"f{k}.png"):
                    image_io.load_rgba8(path, use_pillow=use_pillow)
    assert n_rgba == 2


def test_scene_png_writer_round_trips(g23, tmp_path):
    img = g23["scene_val_pixels"][3]
    path = str(tmp_path / "x.png")
    write_png_rgba(path, img)
    for use_pillow in (False, True):
        assert np.array_equal(image_io.load_rgba8(path, use_pillow=use_pillow), img)
    assert image_io.image_size(path, use_pillow=False) == (64, 64)


def test_dataset_dict_has_blender():
    from hypernerf_torch_amd.datasets import LLFFDataset, dataset_names
    assert dataset_dict['blender'] is BlenderDataset and dataset_dict['llff'] is LLFFDataset
    assert dataset_names() == ['blender', 'llff']
    with pytest.raises(KeyError):
        dataset_dict['dtu']


def test_non_square_img_wh_is_refused(scene):
    for split in ("train", "val", "test"):
        with pytest.raises(ValueError, match="image width must equal image height!"):
            BlenderDataset(scene, split=split, img_wh=(64, 48))


def test_include_idx_is_not_a_parameter(scene):
    with pytest.raises(TypeError):
        BlenderDataset(scene, split="val", img_wh=(64, 64), include_idx=True)


def test_focal_and_poses_equal_the_reference(g23, scene):
    for s in SIZES:
        meta, focal = read_transforms(scene, "train", (s, s))
        assert isinstance(focal, float) and focal == float(g23[f"train_{s}/focal"])
        poses = np.stack([np.array(f['transform_matrix'])[:3, :4] for f in meta['frames']])
        assert poses.dtype == np.float64 and np.array_equal(poses, g23[f"train_{s}/poses"])
    for split, s in (("val", 32), ("test", 24)):
        assert read_transforms(scene, split, (s, s))[1] == float(g23[f"{split}_{s}/focal"])


def test_val_and_test_splits_on_the_host(g23, scene):
    """The val / test constructors touch no device: attributes, lengths and the index bound."""
    val = BlenderDataset(scene, split="val", img_wh=(32, 32))
    test = BlenderDataset(scene, split="test", img_wh=(24, 24))
    assert len(val) == 8 == int(g23["val_32/len"]) and len(test) == 3 == int(g23["test_24/len"])
    for ds in (val, test):
        assert ds.white_back is True and ds.near == 2.0 and ds.far == 6.0 and np.array_equal(ds.bounds, [2.0, 6.0])
        assert ds.ray_cols == 8 and len(ds.poses) == len(ds.image_paths) == len(ds.meta['frames'])
        assert all(os.path.exists(p) for p in ds.image_paths)
        with pytest.raises(IndexError):
            ds[len(ds)]
        with pytest.raises(AttributeError):
            ds.all_rays
    assert np.array_equal(np.stack(val.poses), g23["scene_val_poses"][:, :3])
