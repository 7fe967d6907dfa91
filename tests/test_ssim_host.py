"""CPU tests of the SSIM metric (metrics.py:15-20) and the depth output of the eval loop (eval.py:50-54, 150-158): the
float64 restatement against closed forms, the PFM writer / reader against files the reference's save_pfm wrote
(tests/golden/g21_depth_pfm.npz), and the argument checks that run before any kernel."""
import math
import os

import numpy as np
import pytest
import torch

import ssim_restated as R
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import inference, losses

C1, C2, EPS = 1e-4, 9e-4, 1e-12


def _window64(w):
    return R.window1d(w, torch.float64)


@pytest.mark.parametrize("w", [3, 5, 7, 11])
@pytest.mark.parametrize("a,b", [(0.2, 0.7), (0.0, 0.0), (1.0, 0.05), (0.5, 0.5)])
def test_restated_constant_images_closed_form(w, a, b):
    """Constant images: every moment of a normalised window is the constant itself, both variances and the covariance
    are 0 (up to fp64 rounding), so S = (2ab + C1) C2 / ((a^2 + b^2 + C1) C2 + eps)."""
    x = torch.full((1, 3, 9, 10), a, dtype=torch.float64)
    y = torch.full((1, 3, 9, 10), b, dtype=torch.float64)
    s = R.ssim_map(x, y, w, weights=_window64(w))
    want = (2 * a * b + C1) * C2 / ((a * a + b * b + C1) * C2 + EPS)
    assert float((s - want).abs().max()) <= 1e-12        # fp64 rounding of E[x^2] - mu^2 against C2
    loss = R.dssim(x, y, w, reduction="none", weights=_window64(w))
    assert torch.allclose(loss, torch.clamp((1 - s) / 2, 0, 1), rtol=0, atol=0)


@pytest.mark.parametrize("w", [3, 5, 11])
def test_restated_identical_images(w):
    """Identical images: numerator and denominator of S agree, so S = D / (D + eps): 1 within 1e-12 without eps, and
    1 - S = eps / (D + eps) <= eps / (C1 C2) (about 1.1e-5, reached on flat dark windows) with kornia's eps = 1e-12."""
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 12, 13), generator=g, dtype=torch.float64)
    s0 = R.ssim_map(x, x.clone(), w, eps=0.0)
    assert float((s0 - 1).abs().max()) <= 1e-12
    s = R.ssim_map(x, x.clone(), w)
    gap = 1 - s
    assert float(gap.min()) > 0 and float(gap.max()) <= EPS / (C1 * C2)
    assert float(R.dssim(x, x.clone(), w)) <= EPS / (C1 * C2) / 2


def test_restated_window_is_kornias():
    """The restatement's window and the host weights the kernels take are the same fp32 numbers (kornia's
    get_gaussian_kernel1d: exp(-(i - w//2)^2 / 4.5), normalised), symmetric and summing to 1 within fp32 rounding."""
    for w in (3, 5, 7, 9, 11, 13, 15):
        k = F.ssim_window(w)
        assert k.dtype == torch.float32 and k.shape == (w,)
        assert torch.equal(k.double(), R.window1d(w))
        assert torch.equal(k, k.flip(0))
        assert abs(float(k.double().sum()) - 1) < 1e-6
    e = math.exp(-1 / 4.5)
    assert torch.allclose(F.ssim_window(3).double(), torch.tensor([e, 1.0, e], dtype=torch.float64) / (1 + 2 * e),
                          rtol=0, atol=1e-7)


def test_restated_reflect_padding():
    """A one-pixel change at the corner reaches the map through the reflected taps too: with window 3, pixel (0, 0)
    feeds output (1, 1) directly and output (0, 0) with its own weight only (reflect does not repeat the edge)."""
    x = torch.zeros((1, 1, 4, 5), dtype=torch.float64)
    x[0, 0, 1, 1] = 1.0
    m = R.filt(x, 3, _window64(3))
    w = _window64(3)
    # output (0, 0) reads padded rows/cols -1, 0, 1 -> source 1, 0, 1: pixel (1, 1) appears at taps (0,0),(0,2),(2,0),(2,2)
    assert abs(float(m[0, 0, 0, 0]) - 4 * float(w[0] * w[0])) < 1e-15
    assert abs(float(m[0, 0, 1, 1]) - float(w[1] * w[1])) < 1e-15


def test_write_pfm_matches_reference_bytes(golden_dir, tmp_path):
    """inference.write_pfm writes the bytes the reference's save_pfm wrote: greyscale depth (odd H and W, after
    nan_to_num as eval.py does), colour little-endian and colour big-endian."""
    g = np.load(os.path.join(golden_dir, "g21_depth_pfm.npz"))
    cases = (("depth_pfm", np.nan_to_num(g["depth"])), ("color_pfm", g["color"]), ("color_be_pfm", g["color"].astype(">f4")))
    for key, img in cases:
        path = str(tmp_path / key)
        inference.write_pfm(path, img)
        assert open(path, "rb").read() == g[key].tobytes(), key
    # a tensor argument is written as its numpy array
    path = str(tmp_path / "t.pfm")
    inference.write_pfm(path, torch.nan_to_num(torch.from_numpy(g["depth"])))
    assert open(path, "rb").read() == g["depth_pfm"].tobytes()
    assert g["depth_pfm"].tobytes().startswith(b"Pf\n5 7\n-1.000000\n")


def test_read_pfm_reads_reference_files(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "g21_depth_pfm.npz"))
    for key, want, color in (("depth_pfm", np.nan_to_num(g["depth"]), False), ("color_pfm", g["color"], True),
                             ("color_be_pfm", g["color"], True)):
        path = str(tmp_path / key)
        with open(path, "wb") as f:
            f.write(g[key].tobytes())
        data, scale = inference.read_pfm(path)
        assert scale == 1.0
        assert data.shape == (want.shape if color else want.shape[:2])
        assert np.array_equal(np.asarray(data, dtype=np.float32), want), key


def test_pfm_round_trip_and_refusals(tmp_path):
    a = np.arange(12, dtype=np.float32).reshape(3, 4) - 5.5
    path = str(tmp_path / "a.pfm")
    inference.write_pfm(path, a)
    back, scale = inference.read_pfm(path)
    assert scale == 1.0 and np.array_equal(back, a)
    inference.write_pfm(path, a[..., None])          # (H, W, 1) is greyscale
    assert np.array_equal(inference.read_pfm(path)[0], a)
    with pytest.raises(ValueError):
        inference.write_pfm(path, a.astype(np.float64))
    with pytest.raises(ValueError):
        inference.write_pfm(path, np.zeros((2, 3, 2), dtype=np.float32))
    with open(path, "wb") as f:
        f.write(b"P6\n1 1\n255\n\x00\x00\x00")
    with pytest.raises(ValueError):
        inference.read_pfm(path)


def test_ssim_argument_errors():
    """ValueErrors before any kernel: an even or < 3 window (or one past the kernels' 15), H or W not larger than
    window // 2 (torch's reflect padding refuses the same), shapes that differ or are not 4-D, an unknown reduction."""
    x = torch.rand(1, 3, 8, 9)
    for w in (1, 2, 4, 17, 0, -3):
        with pytest.raises(ValueError):
            F.ssim_dssim(x, x, w)
    with pytest.raises(ValueError):
        F.ssim_dssim(x, x, 3, reduction="max")
    with pytest.raises(ValueError):
        losses.ssim(x, x, reduction="avg")
    with pytest.raises(ValueError):
        F.ssim_dssim(x, torch.rand(1, 3, 8, 8))
    with pytest.raises(ValueError):
        F.ssim_dssim(x[0], x[0])
    with pytest.raises(ValueError):
        F.ssim_dssim(x.double(), x.double())
    for shape, w in (((1, 3, 1, 9), 3), ((1, 3, 8, 1), 3), ((1, 3, 2, 9), 5), ((1, 3, 9, 5), 11)):
        y = torch.rand(shape)
        with pytest.raises(ValueError):
            F.ssim_dssim(y, y, w)
        with pytest.raises(RuntimeError):       # torch's reflect padding refuses the same sizes
            torch.nn.functional.pad(y, [w // 2] * 4, mode="reflect")
    y = torch.rand(1, 3, 2, 2)                  # the smallest image window 3 admits
    torch.nn.functional.pad(y, [1] * 4, mode="reflect")


def test_ssim_refuses_cpu_tensors():
    x = torch.rand(1, 3, 8, 9)
    with pytest.raises(L.HnError):
        F.ssim_dssim(x, x)
    with pytest.raises(L.HnError):
        losses.ssim(x, x)


def test_evaluate_images_depth_arguments():
    """save_depth without save_dir, and an unknown depth format, are refused before anything renders."""
    with pytest.raises(ValueError):
        inference.evaluate_images(None, [], save_depth=True)
    with pytest.raises(ValueError):
        inference.evaluate_images(None, [], save_dir="/nonexistent", depth_format="png")
