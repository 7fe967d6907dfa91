#!/usr/bin/env python3
"""Golden PFM files written by the REFERENCE's own save_pfm (datasets/depth_utils.py:43-69), build container only:

    python tests/golden/make_eval_golden.py        -> tests/golden/g21_depth_pfm.npz

'depth': a float32 (7, 5) depth map with NaNs (odd H and W); 'depth_pfm': the bytes save_pfm writes for it after
np.nan_to_num, as eval.py:150-155 calls it; 'color': a float32 (5, 3, 3) colour image; 'color_pfm' and 'color_be_pfm':
the bytes save_pfm writes for it little- and big-endian.  The files are stored as uint8 arrays.
depth_utils is imported by file path (datasets/__init__.py pulls in readers whose dependencies are absent).
Written with fixed zip timestamps, so that a regeneration is byte-identical."""
import importlib.util
import io
import os
import sys
import tempfile
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HN_REFERENCE", "/root/reference")

import numpy as np


def _depth_utils():
    spec = importlib.util.spec_from_file_location("ref_depth_utils", os.path.join(REF, "datasets", "depth_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save_npz(path, arrays):
    """np.savez with a fixed timestamp on every member (np.savez stamps the current time: not reproducible)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    du = _depth_utils()
    rng = np.random.RandomState(21)
    depth = rng.uniform(0.5, 4.0, (7, 5)).astype(np.float32)
    depth[1, 2] = np.nan
    depth[6, 0] = np.nan
    depth[3, 4] = np.inf
    color = rng.uniform(-1.0, 1.0, (5, 3, 3)).astype(np.float32)
    out = {"depth": depth, "color": color}
    with tempfile.TemporaryDirectory() as tmp:
        for key, img in (("depth_pfm", np.nan_to_num(depth)), ("color_pfm", color),
                         ("color_be_pfm", color.astype(">f4"))):
            path = os.path.join(tmp, key)
            du.save_pfm(path, img)
            with open(path, "rb") as f:
                out[key] = np.frombuffer(f.read(), dtype=np.uint8)
            print(f"{key:13s} {out[key].size} bytes, header {bytes(out[key][:20]).split(bytes([10]))[:3]}")
    save_npz(os.path.join(HERE, "g21_depth_pfm.npz"), out)


if __name__ == "__main__":
    main()
