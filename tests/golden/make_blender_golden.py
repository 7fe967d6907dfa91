#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's BlenderDataset (datasets/blender.py) on a seeded synthetic scene, build container
only:

    python tests/golden/make_blender_golden.py        -> tests/golden/g23_blender.npz

The scene (tests/blender_scene.py: 5 train, 8 val and 3 test RGBA images of 64 x 64 with an object-like alpha) is
written to a temporary directory and read by the reference's own class.  Its optional dependencies are stubbed as
make_dataset_golden.py does: kornia's create_meshgrid (a pixel-index grid, x first) and torchvision's ToTensor (uint8
HWC -> float CHW / 255, the torchvision code path for 8-bit images); Pillow is the real one and its version is
recorded.

Keys:
  scene_<split>_pixels / scene_<split>_poses           the scene itself
  train_<S>/focal, poses, len                          S in 64 (the no-resize path), 32, 24, 80
  train_<S>/rgbs                                       all_rgbs, raw fp32, every row
  train_<S>/rays_sel, rays_rows                        a fixed subset of all_rays rows
  <split>_<S>_<k>/rays (every 7th row), rgbs, c2w, valid_mask; <split>_<S>/len, focal      split in val, test
  resize_<case>_in / _out                              Pillow RGBA LANCZOS pairs
  png_<k> (Pillow-written PNG bytes) with png_<k>_pixels (RGBA files) or png_<k>_mode (others)
  pillow_version
The generator asserts what the tests rely on the fixture to exercise: in every training stack each of the alpha classes
a == 0, 0 < a < 255 and a == 255 holds at least 10 % of the pixels, and for at least 2 % of the pixels a fused
multiply-add would give another all_rgbs than the reference's three rounded operations.
Written with fixed zip timestamps, so that a regeneration is byte-identical."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("HN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import PIL  # noqa: E402
from PIL import Image  # noqa: E402

from blender_scene import make_scene, write_scene  # noqa: E402

SIZES = (64, 32, 24, 80)
ROW_STEP = 7                 # val / test rays: every 7th row of the image
SAMPLES = (("val", 64, (5,)), ("val", 32, (0, 7)), ("val", 80, (2,)), ("test", 24, (0, 2)), ("test", 64, (1,)))


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def _reference_blender():
    k = types.ModuleType("kornia")

    def create_meshgrid(h, w, normalized_coordinates=True):
        assert not normalized_coordinates
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32),
                                indexing="ij")
        return torch.stack([xs, ys], -1)[None]
    k.create_meshgrid = create_meshgrid
    sys.modules["kornia"] = k

    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")

    class ToTensor:
        def __call__(self, pic):
            a = torch.from_numpy(np.array(pic, np.uint8, copy=True)).view(pic.size[1], pic.size[0], len(pic.getbands()))
            return a.permute((2, 0, 1)).contiguous().to(dtype=torch.get_default_dtype()).div(255)
    tr.ToTensor = ToTensor
    tv.transforms = tr
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.transforms"] = tr

    pkg = types.ModuleType("ref_datasets")       # datasets/__init__.py pulls the LLFF reader in: load by file
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["ref_datasets"] = pkg
    for name in ("ray_utils", "blender"):
        spec = importlib.util.spec_from_file_location(f"ref_datasets.{name}", os.path.join(REF, "datasets", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_datasets.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["ref_datasets.blender"]


def _check_fixture(tag, rgba, rgbs):
    """The conditions on the fixture (not tolerances): alpha classes and pixels a fused multiply-add would change."""
    a = rgba[:, 3]
    shares = ((a == 0).mean(), ((a > 0) & (a < 255)).mean(), (a == 255).mean())
    assert min(shares) >= 0.10, (tag, shares)
    x = torch.from_numpy(rgba).float().div(255)
    assert torch.equal(x[:, :3] * x[:, 3:] + (1 - x[:, 3:]), rgbs), tag
    fma = (x[:, :3].double() * x[:, 3:].double() + (1 - x[:, 3:]).double()).float()
    fused = float((fma != rgbs).any(1).float().mean())
    assert fused >= 0.02, (tag, fused)
    print(tag, "alpha classes %.3f %.3f %.3f, fused multiply-add differs on %.3f" % (shares + (fused,)))


def main():
    R = _reference_blender()
    scene = make_scene()
    out = {"pillow_version": np.array(PIL.__version__)}
    for split, (pix, poses) in scene.items():
        out[f"scene_{split}_pixels"] = pix
        out[f"scene_{split}_poses"] = poses
    with tempfile.TemporaryDirectory() as tmp:
        write_scene(tmp, scene)
        for s in SIZES:
            tag = f"train_{s}"
            ds = R.BlenderDataset(tmp, split="train", img_wh=(s, s))
            out[f"{tag}/focal"] = np.float64(ds.focal)
            out[f"{tag}/poses"] = np.stack(ds.poses)
            out[f"{tag}/len"] = np.int64(len(ds))
            rgba = np.concatenate([np.asarray(Image.open(p).resize((s, s), Image.LANCZOS)).reshape(-1, 4)
                                   for p in ds.image_paths])
            _check_fixture(tag, rgba, ds.all_rgbs)
            out[f"{tag}/rgbs"] = ds.all_rgbs.numpy()
            n = len(ds)
            sel = np.unique(np.linspace(0, n - 1, 600).astype(np.int64))
            out[f"{tag}/rays_sel"] = sel.astype(np.int32)
            out[f"{tag}/rays_rows"] = ds.all_rays.numpy()[sel]
        for split, s, ks in SAMPLES:
            ds = R.BlenderDataset(tmp, split=split, img_wh=(s, s))
            out[f"{split}_{s}/len"] = np.int64(len(ds))
            out[f"{split}_{s}/focal"] = np.float64(ds.focal)
            for k in ks:
                smp = ds[k]
                tag = f"{split}_{s}_{k}"
                out[f"{tag}/rays"] = smp["rays"].numpy()[::ROW_STEP]
                out[f"{tag}/rgbs"] = smp["rgbs"].numpy()
                out[f"{tag}/c2w"] = smp["c2w"].numpy()
                out[f"{tag}/valid_mask"] = smp["valid_mask"].numpy()
                assert 0.1 < smp["valid_mask"].float().mean() < 0.9, tag

    # Pillow LANCZOS on RGBA images: down, up, odd ratio, one axis kept, same size, alpha all 0, alpha all 255
    rng = np.random.RandomState(2300)
    for name, (h, w), (oh, ow), alpha in (("down", (64, 64), (32, 32), None), ("up", (50, 50), (80, 80), None),
                                          ("odd", (61, 83), (13, 17), None), ("one_axis", (40, 60), (40, 37), None),
                                          ("same", (48, 48), (48, 48), None), ("alpha0", (40, 40), (24, 24), 0),
                                          ("alpha255", (40, 40), (56, 56), 255)):
        img = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        r = np.hypot(yy - h / 2, xx - w / 2) / (min(h, w) / 2)
        img[..., 3] = np.clip((0.8 - r) * 4 * 255, 0, 255).astype(np.uint8) if alpha is None else alpha
        img[h // 2:, :w // 3, :3] = 255
        out[f"resize_{name}_in"] = img
        out[f"resize_{name}_out"] = np.asarray(Image.fromarray(img, "RGBA").resize((ow, oh), Image.Resampling.LANCZOS))

    # Pillow-written PNGs: RGBA (default and optimize), and RGB / greyscale files the RGBA reader must refuse
    h, w = 24, 32
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 8) % 256, (yy * 10) % 256, ((xx + yy) * 5) % 256], -1).astype(np.uint8)
    img[8:12] = rng.randint(0, 256, (4, w, 3))
    img[14:16] = 128
    img[18:] = (img[18:] + rng.randint(0, 3, (6, w, 3))).astype(np.uint8)
    rgba = np.concatenate([img, ((xx * 9 + yy * 3) % 256).astype(np.uint8)[..., None]], -1)
    rgba[:4, :, 3] = 0
    for k, (arr, mode, kw) in enumerate(((rgba, "RGBA", {}), (rgba, "RGBA", {"optimize": True}), (img, "RGB", {}),
                                         (img[:, :, 0], "L", {}))):
        b = io.BytesIO()
        Image.fromarray(arr, mode).save(b, "PNG", **kw)
        out[f"png_{k}"] = np.frombuffer(b.getvalue(), dtype=np.uint8)
        im = Image.open(io.BytesIO(b.getvalue()))
        if im.mode == "RGBA":
            out[f"png_{k}_pixels"] = np.asarray(im)
        else:
            out[f"png_{k}_mode"] = np.array(im.mode)
    path = os.path.join(HERE, "g23_blender.npz")
    save_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path)} B), Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
