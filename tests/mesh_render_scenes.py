"""Meshes, cameras and rays shared by the mesh renderer's CPU and GPU tests (test_mesh_render_host.py,
test_gpu_mesh_render.py)."""
import functools

import numpy as np

import isosurface_restated as I
import mesh_render_restated as R
import nerfies_scene as NS
import test_isosurface_host as HT

WH = (64, 48)
DISTORTION = dict(k=(-0.2, 0.05, 0.0), p=(0.002, -0.003))
SPHERE_CENTRE = np.array([0.013, -0.021, 0.007])
GRIDS = {"sphere9": lambda: HT.sphere(9), "sphere17": lambda: HT.sphere(17), "torus33": lambda: HT.torus(33)}


def camera(name: str, wh=WH) -> np.ndarray:
    """The three cameras of the tests as 24-float records, for an image of wh: 'plain' at (0.1, -0.05, -3) looking along
    +z with f = 60 at 64 pixels of width, 'distorted' the same with radial and tangential distortion, 'inside' within the
    sphere at (0.05, 0.02, 0) with f = 14.  The principal point is the image centre; f scales with the width."""
    w, h = wh
    s = w / 64.0
    if name == "plain":
        return R.record((0.1, -0.05, -3.0), 60.0 * s, w / 2, h / 2)
    if name == "distorted":
        return R.record((0.1, -0.05, -3.0), 60.0 * s, w / 2, h / 2, **DISTORTION)
    if name == "inside":
        return R.record((0.05, 0.02, 0.0), 14.0 * s, w / 2, h / 2)
    raise KeyError(name)


CAMERAS = ("plain", "distorted", "inside")


def host_rays(rec, wh=WH) -> np.ndarray:
    """(H*W, 8) float32: the float64 statement of the record's rays (nerfies_scene.rays_f64), rounded once."""
    return NS.rays_f64(R.camera_dict(rec, wh), 0.0, 6.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_mesh(name: str) -> dict:
    return I.extract_isosurface(GRIDS[name](), 0.0, HT.UNIT)


def quad(corners) -> dict:
    """Two triangles (0, 1, 2), (0, 2, 3) over four corners."""
    return {"vertices": np.asarray(corners, dtype=np.float32), "faces": np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)}
