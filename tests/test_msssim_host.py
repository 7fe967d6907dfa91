"""CPU tests of multi-scale SSIM: the float64 torch restatement (tests/msssim_restated.py) against the NumPy / SciPy
statement of the original algorithm (tests/golden/g25_msssim.npz, and SciPy itself where it is installed), closed-form
properties, and the host arithmetic and argument checks of hn_msssim_* that run before any kernel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import msssim_restated as R
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses


def _nchw(img):
    """(H, W, C) numpy -> (1, C, H, W) float64 torch."""
    return torch.from_numpy(np.ascontiguousarray(img)).double().permute(2, 0, 1)[None]


def test_restated_matches_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g25_msssim.npz"))
    assert len(g["names"]) >= 4
    for name in g["names"]:
        pred, gt = _nchw(g[f"{name}_pred"]), _nchw(g[f"{name}_gt"])
        lv = R.levels(pred, gt)
        err = float((lv[0] - torch.from_numpy(g[f"{name}_levels"])).abs().max())
        assert err <= 1e-10, (name, err)
        want = float(g[f"{name}_product"])
        got = float(R.product(lv)[0])
        if np.isnan(want):
            assert np.isnan(got), name
        else:
            assert abs(got - want) <= 1e-10, (name, got, want)
    assert any(np.isnan(float(g[f"{n}_product"])) for n in g["names"])       # the negative-cs case is in the file
    assert np.array_equal(g["row7_halved"], [0.5, 2.5, 4.5, 6.0])


def test_restated_matches_scipy_on_fresh_inputs():
    pytest.importorskip("scipy")
    from scipy import ndimage, signal
    rng = np.random.default_rng(7)
    for h, w, c in ((9, 12, 3), (20, 17, 1), (41, 36, 3)):
        gt = rng.random((h, w, c))
        pred = np.clip(gt + 0.1 * rng.standard_normal((h, w, c)), 0, 1)
        a, b = pred.copy(), gt.copy()
        want = []
        for _ in range(5):
            size = min(11, a.shape[0], a.shape[1])
            x = np.arange(size) - (size - 1) / 2.0
            k = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * (size * 1.5 / 11) ** 2))
            k = (k / k.sum())[:, :, None]
            conv = lambda im: signal.fftconvolve(im, k, mode="valid")      # noqa: E731
            mu1, mu2 = conv(a), conv(b)
            s11, s22, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
            v1, v2 = 2 * s12 + 9e-4, s11 + s22 + 9e-4
            want.append([np.mean((2 * mu1 * mu2 + 1e-4) * v1 / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * v2)), np.mean(v1 / v2)])
            a, b = (ndimage.convolve(im, np.ones((2, 2, 1)) / 4.0, mode="reflect")[::2, ::2] for im in (a, b))
        lv = R.levels(_nchw(pred), _nchw(gt))
        assert float((lv[0] - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-10, (h, w, c)


def test_restated_identical_images_give_exactly_one():
    g = torch.Generator().manual_seed(4)
    for shape in ((1, 3, 5, 7), (2, 3, 16, 16), (1, 1, 37, 53)):
        x = torch.rand(shape, generator=g, dtype=torch.float64)
        lv = R.levels(x, x.clone())
        assert torch.equal(lv, torch.ones_like(lv))
        assert torch.equal(R.product(lv), torch.ones(shape[0], dtype=torch.float64))


def test_restated_downsample_of_a_row():
    row = torch.arange(7, dtype=torch.float64).view(1, 1, 1, 7)
    assert torch.equal(R.downsample(row).flatten(), torch.tensor([0.5, 2.5, 4.5, 6.0], dtype=torch.float64))
    col = R.downsample(row.transpose(2, 3))
    assert col.shape == (1, 1, 4, 1) and torch.equal(col.flatten(), torch.tensor([0.5, 2.5, 4.5, 6.0], dtype=torch.float64))
    assert R.downsample(torch.rand(1, 2, 1, 1, dtype=torch.float64)).shape == (1, 2, 1, 1)      # a side of 1 stays 1


def test_windows_are_the_restatements():
    """The host taps the kernel takes are the restatement's float64 taps; even sizes sit on half-integer offsets."""
    for size in range(1, 12):
        k = F.msssim_window(size)
        assert k.dtype == torch.float64 and k.shape == (size,)
        assert torch.equal(k, R.window1d(size)) and torch.equal(k, k.flip(0))
        assert abs(float(k.sum()) - 1) < 1e-15
    sigma = 2 * 1.5 / 11
    e = np.exp(-0.25 / (2 * sigma * sigma))
    assert torch.allclose(F.msssim_window(2), torch.tensor([e, e], dtype=torch.float64) / (2 * e), rtol=0, atol=1e-16)
    assert F.msssim_pyramid(5, 7) == [(5, 7, 5), (3, 4, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1)]
    assert [s for _, _, s in F.msssim_pyramid(16, 16)] == [11, 8, 4, 2, 1]
    assert tuple(F.MSSSIM_WEIGHTS) == R.WEIGHTS


SHAPES = [(1, 3, 5, 7), (1, 3, 16, 16), (2, 3, 37, 53), (1, 1, 64, 48), (1, 3, 1, 1), (3, 2, 15, 33), (1, 3, 378, 504)]


def test_symbols_and_version():
    assert {"hn_msssim_workspace_bytes", "hn_msssim_forward"} <= set(L.EXPORTS)
    lib = L.load()
    assert hasattr(lib, "hn_msssim_workspace_bytes") and hasattr(lib, "hn_msssim_forward")
    assert lib.hn_version() == 340


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_bytes_match_python(shape):
    lib = L.load()
    n, c, h, w = shape
    nbytes = C.c_int64(-1)
    assert lib.hn_msssim_workspace_bytes(n, c, h, w, C.byref(nbytes)) == 0
    assert nbytes.value == F.msssim_workspace_bytes(n, c, h, w) and nbytes.value % 16 == 0
    # by hand for the smallest: levels 5x7, 3x4, 2x2, 1x1, 1x1; one tile per plane at every level
    if shape == (1, 3, 5, 7):
        floats = 2 * 3 * (12 + 4 + 1 + 1) + 2 * 3 * 5
        assert nbytes.value == (floats * 4 + 15) // 16 * 16


def test_workspace_bytes_refusals():
    lib = L.load()
    nbytes = C.c_int64(0)
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8)):
        assert lib.hn_msssim_workspace_bytes(*bad, C.byref(nbytes)) == -2
    assert lib.hn_msssim_workspace_bytes(1, 3, 8, 8, None) == -2


def test_forward_refuses_bad_arguments_before_any_launch():
    """Every refusal is -2 and comes before the first launch: the pointers below are never dereferenced on a device (a
    machine without a GPU runs this test), the host arrays only as far as the checks read them."""
    lib = L.load()
    strides = (C.c_int64 * 4)(3 * 8 * 9, 8 * 9, 9, 1)
    taps = (C.c_float * 55)(*([0.1] * 55))
    sizes = (C.c_int * 5)(8, 4, 2, 1, 1)                # 8 x 9, 4 x 5, 2 x 3, 1 x 2, 1 x 1
    fake = 0x1000                                       # a non-NULL device address nothing reads

    def call(n=1, c=3, h=8, w=9, x=fake, xs=strides, y=fake, ys=strides, t=taps, s=sizes, out=fake, ws=fake):
        return lib.hn_msssim_forward(x, xs, y, ys, n, c, h, w, t, s, 1e-4, 9e-4, out, ws, None)

    for kw in (dict(n=0), dict(c=0), dict(h=0), dict(w=0), dict(n=-2), dict(x=None), dict(y=None), dict(xs=None),
               dict(ys=None), dict(t=None), dict(s=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -2, kw
    for bad in ((0, 4, 2, 1, 1), (12, 4, 2, 1, 1), (8, 4, 2, 1, 2), (9, 4, 2, 1, 1), (8, 5, 2, 1, 1), (8, 4, 2, 1, -1)):
        assert call(s=(C.c_int * 5)(*bad)) == -2, bad


def test_ms_ssim_argument_errors():
    x = torch.rand(1, 3, 8, 9)
    with pytest.raises(ValueError):
        losses.ms_ssim(x[0], x[0])
    with pytest.raises(ValueError):
        losses.ms_ssim(x, torch.rand(1, 3, 8, 8))
    with pytest.raises(ValueError):
        losses.ms_ssim(x, x, reduction="sum")
    with pytest.raises(ValueError):
        F.msssim_levels(x.double(), x.double())
    with pytest.raises(L.HnError):                      # no CPU fallback
        losses.ms_ssim(x, x)
