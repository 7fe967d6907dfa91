#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's LLFFDataset (datasets/llff.py) on a seeded synthetic scene, build container only:

    python tests/golden/make_dataset_golden.py        -> tests/golden/g22_llff.npz

The scene (tests/llff_scene.py: 6 images of 60 x 80, a jittered forward-facing rig) is written to a temporary
directory and read by the reference's own class.  Its optional dependencies are stubbed as make_golden.py:g_rays does:
kornia's create_meshgrid (a pixel-index grid, x first) and torchvision's ToTensor (uint8 HWC -> float CHW / 255, the
torchvision code path for 8-bit images); Pillow is the real one and its version is recorded.

Keys, per configuration tag `<split>_<s|n>_<i|x>_<W>x<H>` (s: spheric_poses, i: include_idx):
  <tag>/focal, poses, pose_avg, bounds, len, image_paths (basenames, one string)
  train: <tag>/rays_rows, rays_sel (a fixed subset of all_rays rows; every row for two 40 x 30 configurations),
         <tag>/ids (column 8 when present); train_<W>x<H>/rgb8 (all_rgbs x 255, exact: the uint8 source of every
         value; the same for every configuration of that size)
  val:   <tag>/rays, rgb8, c2w           test: <tag>/poses_test, rays_<k> (every 7th row) / c2w_<k> for a few poses k
Plus scene_pixels / scene_poses_bounds, resize_<case>_in / _out (Pillow LANCZOS), png_<k> (Pillow-written PNG bytes
using all five scanline filters between them) with png_<k>_pixels, and pillow_version.
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

from llff_scene import make_scene, write_scene  # noqa: E402

TEST_POSES = (0, 37, 119)
TEST_ROW_STEP = 7            # test-split rays: every 7th row of the image
SIZES = ((80, 60), (40, 30), (56, 42))


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def _reference_llff():
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

    pkg = types.ModuleType("ref_datasets")       # datasets/__init__.py pulls the Blender reader in: load by file
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["ref_datasets"] = pkg
    for name in ("ray_utils", "llff"):
        spec = importlib.util.spec_from_file_location(f"ref_datasets.{name}", os.path.join(REF, "datasets", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_datasets.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["ref_datasets.llff"]


def _rgb8(rgbs):
    u8 = np.round(rgbs.numpy() * 255).astype(np.uint8)
    assert np.array_equal((torch.from_numpy(u8).float() / 255).numpy(), rgbs.numpy()), "all_rgbs is not u8 / 255"
    return u8


def _common(out, tag, ds):
    out[f"{tag}/focal"] = np.float64(ds.focal)
    out[f"{tag}/poses"] = ds.poses
    out[f"{tag}/pose_avg"] = ds.pose_avg
    out[f"{tag}/bounds"] = ds.bounds
    out[f"{tag}/len"] = np.int64(len(ds))


def main():
    R = _reference_llff()
    pix, pb = make_scene()
    out = {"scene_pixels": pix, "scene_poses_bounds": pb, "pillow_version": np.array(PIL.__version__)}
    with tempfile.TemporaryDirectory() as tmp:
        write_scene(tmp, pix, pb)
        for spheric in (False, True):
            for idx in (False, True):
                for (w, h) in SIZES:
                    tag = f"train_{'s' if spheric else 'n'}_{'i' if idx else 'x'}_{w}x{h}"
                    ds = R.LLFFDataset(tmp, split="train", img_wh=(w, h), spheric_poses=spheric, include_idx=idx)
                    _common(out, tag, ds)
                    rays = ds.all_rays.numpy()
                    n = rays.shape[0]
                    full = (w, h) == (40, 30) and spheric == idx
                    sel = np.arange(n) if full else np.unique(np.linspace(0, n - 1, 600).astype(np.int64))
                    out[f"{tag}/rays_sel"] = sel.astype(np.int32)
                    out[f"{tag}/rays_rows"] = rays[sel, :8]
                    if idx:
                        out[f"{tag}/ids"] = rays[:, 8].astype(np.int8)
                    rgb8 = _rgb8(ds.all_rgbs)
                    if not spheric and not idx:
                        out[f"train_{w}x{h}/rgb8"] = rgb8
                    else:
                        assert np.array_equal(rgb8, out[f"train_{w}x{h}/rgb8"])
                    print(tag, rays.shape)
                tag = f"val_{'s' if spheric else 'n'}_{'i' if idx else 'x'}_40x30"
                ds = R.LLFFDataset(tmp, split="val", img_wh=(40, 30), spheric_poses=spheric, include_idx=idx)
                _common(out, tag, ds)
                s = ds[0]
                out[f"{tag}/rays"] = s["rays"].numpy()
                out[f"{tag}/rgb8"] = _rgb8(s["rgbs"])
                out[f"{tag}/c2w"] = s["c2w"].numpy()
            for split in ("test", "test_train"):
                tag = f"{split}_{'s' if spheric else 'n'}_x_40x30"
                ds = R.LLFFDataset(tmp, split=split, img_wh=(40, 30), spheric_poses=spheric)
                _common(out, tag, ds)
                out[f"{tag}/poses_test"] = ds.poses_test
                for k in (TEST_POSES if split == "test" else (0, 5)):
                    s = ds[k]
                    out[f"{tag}/rays_{k}"] = s["rays"].numpy()[::TEST_ROW_STEP]
                    out[f"{tag}/c2w_{k}"] = s["c2w"].numpy()
        tag = "val_n_x_56x42"
        ds = R.LLFFDataset(tmp, split="val", img_wh=(56, 42))
        _common(out, tag, ds)
        s = ds[0]
        out[f"{tag}/rays"] = s["rays"].numpy()
        out[f"{tag}/rgb8"] = _rgb8(s["rgbs"])
        out[f"{tag}/c2w"] = s["c2w"].numpy()
        out["image_names"] = np.array([os.path.basename(p) for p in ds.image_paths])

    # Pillow LANCZOS on further size pairs: upscale, odd factors, 1-pixel edges
    rng = np.random.RandomState(2200)
    for name, (h, w), (oh, ow) in (("up", (30, 40), (58, 77)), ("odd", (61, 83), (13, 17)), ("third", (60, 80), (20, 27)),
                                   ("one_px", (60, 80), (1, 1)), ("row", (1, 80), (1, 37)), ("col", (60, 1), (23, 1)),
                                   ("big", (378, 504), (95, 126))):
        if h * w > 4096:      # large: random 14 x 14 blocks (sharp edges, compresses)
            img = np.kron(rng.randint(0, 256, (h // 14, w // 14, 3)), np.ones((14, 14, 1))).astype(np.uint8)
        else:
            img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        img[h // 2:, :w // 3] = 255
        img[:h // 4, w // 2:] = 0
        out[f"resize_{name}_in"] = img
        out[f"resize_{name}_out"] = np.asarray(Image.fromarray(img).resize((ow, oh), Image.Resampling.LANCZOS))

    # Pillow-written PNGs: RGB and RGBA, default and optimize; between them scanline filters 0-4
    h, w = 24, 32
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 8) % 256, (yy * 10) % 256, ((xx + yy) * 5) % 256], -1).astype(np.uint8)
    img[8:12] = rng.randint(0, 256, (4, w, 3))
    img[14:16] = 128
    img[18:] = (img[18:] + rng.randint(0, 3, (6, w, 3))).astype(np.uint8)
    rgba = np.concatenate([img, (img[..., :1] // 2 + 60).astype(np.uint8)], -1)
    for k, (arr, mode, kw) in enumerate(((img, "RGB", {}), (rgba, "RGBA", {}), (rgba, "RGBA", {"optimize": True}),
                                         (img[:, :, 0], "L", {}))):
        b = io.BytesIO()
        Image.fromarray(arr, mode).save(b, "PNG", **kw)
        out[f"png_{k}"] = np.frombuffer(b.getvalue(), dtype=np.uint8)
        out[f"png_{k}_pixels"] = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
    path = os.path.join(HERE, "g22_llff.npz")
    save_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path)} B), Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
