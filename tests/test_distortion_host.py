"""CPU tests of the distortion loss: closed-form properties of the float64 restatement (tests/distortion_restated.py),
the refusals of losses.DistortionLoss and functional.distortion_loss, and the argument checks of hn_distortion_* that
run before any launch."""
import numpy as np
import pytest
import torch

import distortion_restated as R
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses

NEW_SYMBOLS = ("hn_distortion_forward", "hn_distortion_forward_grad", "hn_distortion_backward")
SPACINGS = ("linear", "disparity")


def _ray(seed, s, near=2.0, far=6.0):
    rng = np.random.default_rng(seed)
    z = np.sort(rng.uniform(near, far, s))
    w = rng.uniform(0.0, 1.0, s) ** 3
    return w / max(w.sum(), 1e-30) * 0.9, z


# ---- the restated loss ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("s", [2, 3, 17])
def test_restated_gradient_agrees_with_central_differences(s, spacing):
    w, z = _ray(10 + s, s)
    g = R.ray_grad(w, z, 2.0, 6.0, spacing)
    for i in range(s):
        # the loss is quadratic in w: a central difference is exact up to rounding, whatever the step
        h = 1e-3
        wp, wm = w.copy(), w.copy()
        wp[i] += h
        wm[i] -= h
        fd = (R.ray_loss(wp, z, 2.0, 6.0, spacing) - R.ray_loss(wm, z, 2.0, 6.0, spacing)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-11, (i, fd, g[i])
    # and the torch form of the same loss, through autograd
    wt = torch.from_numpy(w[None]).requires_grad_(True)
    lt = R.loss_torch(wt, torch.from_numpy(z[None]), 2.0, 6.0, spacing)
    assert abs(float(lt.detach()) - R.ray_loss(w, z, 2.0, 6.0, spacing)) <= 1e-14
    lt.backward()
    assert np.allclose(wt.grad.numpy()[0], g, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 100])
def test_uniform_ray_gives_one_third(n):
    """S = N + 1 samples at z_i = i / N on [0, 1], weights 1 / N with the last weight 0: N intervals of equal width and
    equal mass, the discretisation of a uniform density, whose distortion is 1/3 for every N — the bilateral part
    (N^2 - 1) / (3 N^2), the width part 1 / (3 N^2)."""
    z = np.arange(n + 1) / n
    w = np.full(n + 1, 1.0 / n)
    w[-1] = 0.0
    m, d = R.intervals(z, 0.0, 1.0, "linear")
    both = sum(w[i] * w[j] * abs(m[i] - m[j]) for i in range(n + 1) for j in range(n + 1))
    width = float((w * w * d).sum() / 3)
    assert abs(both - (n * n - 1) / (3.0 * n * n)) <= 1e-12
    assert abs(width - 1 / (3.0 * n * n)) <= 1e-15
    assert abs(R.ray_loss(w, z, 0.0, 1.0) - 1.0 / 3.0) <= 1e-12


@pytest.mark.parametrize("spacing", SPACINGS)
def test_one_hot_zero_and_single_sample_rays(spacing):
    s = 9
    _, z = _ray(3, s)
    m, d = R.intervals(z, 2.0, 6.0, spacing)
    assert np.all(d[:-1] > 0) and d[-1] == 0.0 and np.all(np.diff(m) > 0)
    for i in (0, 4, s - 2):
        w = np.zeros(s)
        w[i] = 1.0
        assert abs(R.ray_loss(w, z, 2.0, 6.0, spacing) - d[i] / 3) <= 1e-15
        g = R.ray_grad(w, z, 2.0, 6.0, spacing)
        assert abs(g[i] - 2 * d[i] / 3) <= 1e-15
        others = np.delete(np.arange(s), i)
        assert np.allclose(g[others], 2 * np.abs(m[others] - m[i]), rtol=0, atol=1e-15)
    last = np.zeros(s)
    last[-1] = 1.0
    assert R.ray_loss(last, z, 2.0, 6.0, spacing) == 0.0 and R.ray_grad(last, z, 2.0, 6.0, spacing)[-1] == 0.0
    assert R.ray_loss(np.zeros(s), z, 2.0, 6.0, spacing) == 0.0
    assert not R.ray_grad(np.zeros(s), z, 2.0, 6.0, spacing).any()
    assert R.ray_loss([0.7], [3.0], 2.0, 6.0, spacing) == 0.0 and R.ray_grad([0.7], [3.0], 2.0, 6.0, spacing)[0] == 0.0


def test_linear_loss_is_unchanged_by_a_shift_and_scale_of_the_depths():
    w, z = _ray(5, 33)
    want = R.ray_loss(w, z, 2.0, 6.0)
    for a, b in ((3.0, 0.0), (1.0, -7.5), (0.125, 40.0)):
        assert abs(R.ray_loss(w, a * z + b, a * 2.0 + b, a * 6.0 + b) - want) <= 1e-13
    # disparity spacing: unchanged by a scale (a shift changes the reciprocals)
    want = R.ray_loss(w, z, 2.0, 6.0, "disparity")
    assert abs(R.ray_loss(w, 3.0 * z, 6.0, 18.0, "disparity") - want) <= 1e-13


def test_disparity_spacing_of_a_ray_uniform_in_disparity_is_linear_spacing_of_a_uniform_ray():
    s, near, far = 21, 0.5, 8.0
    w, _ = _ray(7, s)
    z_disp = 1.0 / np.linspace(1.0 / near, 1.0 / far, s)
    z_lin = np.linspace(near, far, s)
    assert np.allclose(R.normalised(z_disp, near, far, "disparity"), np.arange(s) / (s - 1), rtol=0, atol=1e-14)
    a, b = R.ray_loss(w, z_disp, near, far, "disparity"), R.ray_loss(w, z_lin, near, far, "linear")
    assert abs(a - b) <= 1e-13 and a > 0
    assert np.allclose(R.ray_grad(w, z_disp, near, far, "disparity"), R.ray_grad(w, z_lin, near, far, "linear"), atol=1e-13)


def test_batch_mean_and_per_ray():
    rays = [_ray(20 + i, 12) for i in range(5)]
    w, z = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
    for spacing in SPACINGS:       # the matrix form the batch helpers use is the double loop
        for wr, zr in rays:
            lo, go = R.ray_loss_grad_outer(wr, zr, 2.0, 6.0, spacing)
            assert abs(lo - R.ray_loss(wr, zr, 2.0, 6.0, spacing)) <= 1e-15
            assert np.allclose(go, R.ray_grad(wr, zr, 2.0, 6.0, spacing), rtol=0, atol=1e-15)
    assert np.allclose(R.grad_rays(w, z, 2.0, 6.0), np.stack([R.ray_grad(wr, zr, 2.0, 6.0) for wr, zr in rays]), rtol=0, atol=1e-15)
    pr = R.per_ray(w, z, 2.0, 6.0)
    assert pr.shape == (5,) and abs(R.loss(w, z, 2.0, 6.0) - pr.mean()) <= 1e-15
    lt = R.loss_torch(torch.from_numpy(w), torch.from_numpy(z), 2.0, 6.0)
    assert abs(float(lt) - pr.mean()) <= 1e-14


# ---- losses.DistortionLoss -------------------------------------------------------------------------------------------
def test_distortion_loss_constructor():
    ok = losses.DistortionLoss()
    assert (ok.weight, ok.levels, ok.spacing, ok.near, ok.far) == (0.01, ("fine",), None, None, None)       # the paper's lambda
    both = losses.DistortionLoss(weight=0.0, levels=["coarse", "fine"], spacing="disparity", near=1, far=3)
    assert (both.weight, both.levels, both.spacing, both.near, both.far) == (0.0, ("coarse", "fine"), "disparity", 1.0, 3.0)
    assert losses.DistortionLoss(levels="coarse").levels == ("coarse",)
    for kw in (dict(levels=("medium",)), dict(levels=("fine", "fine")), dict(levels=()), dict(levels=[]),
               dict(spacing="log"), dict(spacing=""), dict(weight=-0.01), dict(weight=float("nan"))):
        with pytest.raises(ValueError):
            losses.DistortionLoss(**kw)


def test_distortion_loss_refuses_what_does_not_come_from_one_forward_pass():
    class Model:
        near, far, use_linear_disparity = 2.0, 6.0, False
    dl = losses.DistortionLoss(levels=("coarse", "fine"))
    res = {"coarse": {"weights": torch.zeros(4, 8)}, "fine": {"weights": torch.zeros(4, 16)}}
    with pytest.raises(ValueError, match="last_sampling"):
        dl(Model(), res)
    m = Model()
    m.last_sampling = {"z_coarse": torch.zeros(4, 8), "z_fine": torch.zeros(4, 12)}
    with pytest.raises(ValueError, match="fine"):
        losses.DistortionLoss(levels=("fine",))(m, res)
    with pytest.raises(ValueError, match="fine"):
        losses.DistortionLoss(levels=("fine",))(m, {"coarse": res["coarse"]})
    with pytest.raises(L.HnError):                           # no CPU fallback
        losses.DistortionLoss(levels=("coarse",))(m, res)


def test_functional_argument_errors():
    w, z = torch.zeros(4, 8), torch.ones(4, 8)
    for args, kw in (((w[:, :7], z, 2.0, 6.0), {}), ((w[0], z[0], 2.0, 6.0), {}), ((w.double(), z, 2.0, 6.0), {}),
                     ((w, z.double(), 2.0, 6.0), {}), ((w[:0], z[:0], 2.0, 6.0), {}), ((w[:, :0], z[:, :0], 2.0, 6.0), {}),
                     ((w, z, 2.0, 2.0), {}), ((w, z, float("nan"), 6.0), {}), ((w, z, 2.0, float("inf")), {}),
                     ((w, z, 2.0, 6.0, "log"), {}), ((w, z, 2.0, 6.0), dict(reduction="sum")),
                     ((w, z, 0.0, 6.0, "disparity"), {}), ((w, z, -1.0, 6.0, "disparity"), {}),
                     ((w, z, 2.0, 6.0), dict(root=float("nan"))),
                     ((torch.zeros(2, F.MAX_SAMPLES + 1), torch.zeros(2, F.MAX_SAMPLES + 1), 2.0, 6.0), {})):
        with pytest.raises(ValueError):
            F.distortion_loss(*args, **kw)
    with pytest.raises(L.HnError):
        F.distortion_loss(w, z, 2.0, 6.0)
    with pytest.raises(L.HnError):
        F.distortion_loss(w, z, 0.0, 6.0, reduction="none")   # near = 0 is fine under linear spacing
    with pytest.raises(ValueError):
        F.backward_all([])


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    assert set(NEW_SYMBOLS) <= set(L.EXPORTS)
    assert "hn_regularizers.hip" in L.SOURCES and "hn_wave.h" in L.CSRC_HEADERS
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    with open(L.HEADER) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert {"distortion_loss", "backward_all", "SPACINGS"} <= set(dir(F)) and hasattr(losses, "DistortionLoss")


FAKE = 0x1000          # a non-NULL device address nothing reads: every refusal comes before the first launch


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.load()

    def fwd(w=FAKE, z=FAKE, b=8, s=16, near=2.0, far=6.0, spacing=0, per_ray=FAKE, out=FAKE, ticket=FAKE):
        return lib.hn_distortion_forward(w, z, b, s, near, far, spacing, per_ray, out, ticket, None)

    def fwd_grad(w=FAKE, z=FAKE, b=8, s=16, near=2.0, far=6.0, spacing=0, scale=1.0, per_ray=FAKE, out=FAKE, ticket=FAKE,
                 dw=FAKE):
        return lib.hn_distortion_forward_grad(w, z, b, s, near, far, spacing, scale, per_ray, out, ticket, dw, None)

    def bwd(w=FAKE, z=FAKE, b=8, s=16, near=2.0, far=6.0, spacing=0, g=FAKE, per_ray_g=0, dw=FAKE):
        return lib.hn_distortion_backward(w, z, b, s, near, far, spacing, g, per_ray_g, dw, None)

    common = (dict(w=None), dict(z=None), dict(b=0), dict(b=-1), dict(s=0), dict(s=-4), dict(s=513), dict(far=2.0),
              dict(near=6.0), dict(near=float("nan")), dict(far=float("nan")), dict(spacing=2), dict(spacing=-1),
              dict(spacing=1, near=0.0), dict(spacing=1, near=-2.0))
    for kw in common + (dict(per_ray=None), dict(ticket=None)):
        assert fwd(**kw) == -2, kw
    for kw in common + (dict(per_ray=None), dict(out=None), dict(ticket=None), dict(dw=None), dict(scale=float("nan"))):
        assert fwd_grad(**kw) == -2, kw
    for kw in common + (dict(g=None), dict(dw=None)):
        assert bwd(**kw) == -2, kw
