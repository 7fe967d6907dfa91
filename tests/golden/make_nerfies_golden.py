#!/usr/bin/env python3
"""Golden vectors of the Nerfies-format dataset on two seeded synthetic captures:

    python tests/golden/make_nerfies_golden.py        -> tests/golden/g24_nerfies.npz

There is no reference reader of this format to record from, so the expected rays are the float64 NumPy statement of
the documented camera model (tests/nerfies_scene.py: rays_f64), and the generator checks that statement against the
closed-form forward projection (project_f64) before it writes anything: every pixel centre of every camera must come
back to within 1e-9 px.

Scenes: 'a' = make_scene(24): 24 x 16 images at image_scale 2, 5 train + 2 val; 'b' = make_scene(25, wh=(67, 41),
n_train=3, n_val=1): odd in both dimensions.

Keys, per scene s in a, b:
  s/ids, train_ids, val_ids, metadata, cameras, path_cameras, pixels, scene, image_scale     the capture itself
                                                                   (nerfies_scene.scene_from_arrays rebuilds it)
  s/train_rows, s/val_rows, s/test_rows      every 7th row of the split's float64 ray rows [o, d, near, far, id]
                                             (id = warp_id; test rows carry test_id 0), images concatenated
Written with fixed zip timestamps, so that a regeneration is byte-identical."""
import io
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import nerfies_scene as NS  # noqa: E402

ROW_STEP = 7
SCENES = {"a": dict(seed=24), "b": dict(seed=25, wh=(67, 41), n_train=3, n_val=1)}


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def reprojection_error(scene) -> float:
    """Largest distance in pixels between a pixel centre and the forward projection of a point on its ray."""
    worst = 0.0
    for split in ("train", "val", "test"):
        for cam, _ in NS.split_cameras(scene, split):
            rows = NS.rays_f64(cam, 0.0, 1.0)
            w, h = cam["image_size"]
            j, i = np.mgrid[0:h, 0:w]
            centres = np.stack([i.reshape(-1) + 0.5, j.reshape(-1) + 0.5], -1)
            px = NS.project_f64(cam, rows[:, :3] + 1.7 * rows[:, 3:6])
            worst = max(worst, float(np.abs(px - centres).max()))
    return worst


def main():
    out = {}
    for name, kw in SCENES.items():
        scene = NS.make_scene(**kw)
        err = reprojection_error(scene)
        assert err <= 1e-9, (name, err)
        for k, v in NS.scene_to_arrays(scene).items():
            out[f"{name}/{k}"] = v
        for split in ("train", "val", "test"):
            out[f"{name}/{split}_rows"] = NS.split_rays_f64(scene, split)[::ROW_STEP]
        print(f"scene {name}: reprojection error {err:.2e} px, train rows {out[name + '/train_rows'].shape}")
    path = os.path.join(HERE, "g24_nerfies.npz")
    save_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
