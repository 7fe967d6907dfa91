"""CPU tests of the background regularization: closed-form properties of the float64 restatement
(tests/background_restated.py), the host loader of points.npy, the refusals of losses.BackgroundLoss, and the argument
checks of hn_bg_* that run before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import background_restated as R
import nerfies_scene as NS
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses
from hypernerf_torch_amd.datasets import NerfiesDataset, nerfies

NEW_SYMBOLS = ("hn_bg_sample", "hn_bg_loss_forward", "hn_bg_loss_forward_grad", "hn_bg_loss_backward")


# ---- the restated loss ---------------------------------------------------------------------------------------------
def test_restated_loss_is_zero_at_zero_residual():
    p = np.random.default_rng(0).standard_normal((17, 3))
    assert R.loss(p, p, 0.001) == 0.0
    assert np.array_equal(R.grad(p, p, 0.001), np.zeros((17, 3)))


def test_restated_loss_tends_to_two():
    p = np.zeros((5, 3))
    prev = 0.0
    for r in (1e-3, 1e-2, 1e-1, 1.0, 1e3):
        w = p + np.array([r, 0.0, 0.0])
        v = R.loss(w, p, 0.001)
        assert prev < v < 2.0, (r, v)
        prev = v
    assert abs(R.loss(p + np.array([1.0, 0.0, 0.0]), p, 0.001) - 2.0) < 1e-5       # x = 1e6: 2 - 8 / (x + 4)
    # x = 4 is the half-way point: 2 * 4 / 8 = 1
    assert abs(R.loss(p + np.array([0.0, 0.002, 0.0]), p, 0.001) - 1.0) < 1e-12


@pytest.mark.parametrize("scale", [0.001, 0.05, 1.0])
def test_restated_gradient_agrees_with_central_differences(scale):
    rng = np.random.default_rng(3)
    n = 11
    p = rng.standard_normal((n, 3))
    # residuals from far inside the quadratic bowl to far out on the flat tail
    norms = scale * 10.0 ** np.linspace(-2, 2, n)
    d = rng.standard_normal((n, 3))
    w = p + d / np.linalg.norm(d, axis=-1, keepdims=True) * norms[:, None]
    g = R.grad(w, p, scale, g=0.37)
    for row in range(n):
        for c in range(3):
            # the mean is a sum of per-row terms: difference this row's own term (the others cancel exactly, and
            # their O(1) values would only add cancellation noise), step 1e-4 of the residual
            h = 1e-4 * norms[row]
            wp, wm = w[row:row + 1].copy(), w[row:row + 1].copy()
            wp[0, c] += h
            wm[0, c] -= h
            fd = 0.37 * (R.loss(wp, p[row:row + 1], scale) - R.loss(wm, p[row:row + 1], scale)) / (2 * h) / n
            assert abs(fd - g[row, c]) <= 1e-6 * np.abs(g[row]).max(), (row, c, fd, g[row, c])
    # and the torch form of the same loss, through autograd
    wt = torch.from_numpy(w).requires_grad_(True)
    lt = R.loss_torch(wt, torch.from_numpy(p), scale)
    assert abs(float(lt.detach()) - R.loss(w, p, scale)) <= 1e-14
    (0.37 * lt).backward()
    assert np.allclose(wt.grad.numpy(), g, rtol=1e-12, atol=0)


def test_restated_sampler_indices():
    pts = np.arange(9, dtype=np.float32).reshape(3, 3)
    ids = np.array([7, 3, 11, 5, 2], dtype=np.int64)
    last = np.float32(1.0 - 2.0 ** -24)
    u = np.array([[0.0, 0.0], [last, last], [0.34, 0.59], [0.67, 0.81]], dtype=np.float32)
    out, oid, i, j = R.sample(pts, ids, u, np.ones((4, 3), dtype=np.float32), 0.0)
    assert i.tolist() == [0, 2, 1, 2] and j.tolist() == [0, 4, 2, 4]
    assert np.array_equal(out, pts[i]) and np.array_equal(oid, ids[j])
    out2 = R.sample(pts, ids, u, np.full((4, 3), 2.0, dtype=np.float32), 0.25)[0]
    assert out2.dtype == np.float32 and np.array_equal(out2, pts[i] + np.float32(0.5))


# ---- points.npy ---------------------------------------------------------------------------------------------------
def test_load_points_applies_centre_and_scale(tmp_path):
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((40, 3)) * 3
    path = str(tmp_path / "points.npy")
    np.save(path, raw)
    centre, scale = [0.4, -0.2, 1.1], 0.37
    got = nerfies.load_points(path, centre, scale)
    assert got.dtype == np.float32 and got.shape == (40, 3)
    assert np.array_equal(got, ((raw - np.asarray(centre)) * scale).astype(np.float32))
    assert np.array_equal(nerfies.load_points(path), raw.astype(np.float32))
    np.save(path, raw.astype(np.float32))                    # float32 on disk: still moved in float64
    assert np.array_equal(nerfies.load_points(path, centre, scale),
                          ((raw.astype(np.float32).astype(np.float64) - np.asarray(centre)) * scale).astype(np.float32))
    for bad in (np.zeros((4, 2)), np.zeros((0, 3)), np.zeros(6)):
        np.save(path, bad)
        with pytest.raises(ValueError, match="points.npy"):
            nerfies.load_points(path)


def test_missing_points_file_raises_naming_the_path(tmp_path):
    path = str(tmp_path / "nowhere" / "points.npy")
    with pytest.raises(ValueError) as e:
        nerfies.load_points(path)
    assert path in str(e.value)


def test_dataset_background_points_and_warp_ids(tmp_path):
    scene = NS.make_scene(11, wh=(8, 6), n_train=4, n_val=2)
    root = NS.write_scene(str(tmp_path / "scene"), scene)
    ds = NerfiesDataset(root, split="train", image_scale=2, device="cpu")
    with pytest.raises(ValueError) as e:
        ds.background_points
    assert os.path.join(root, "points.npy") in str(e.value)
    raw = np.random.default_rng(2).standard_normal((25, 3))
    np.save(os.path.join(root, "points.npy"), raw)
    pts = ds.background_points
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (25, 3) and pts.device == ds.device
    want = ((raw - np.asarray(scene["scene"]["center"])) * scene["scene"]["scale"]).astype(np.float32)
    assert np.array_equal(pts.numpy(), want)
    assert ds.background_points is pts                      # read once
    want_ids = sorted({scene["metadata"][i]["warp_id"] for i in scene["train_ids"]})
    assert ds.warp_ids == want_ids and len(want_ids) == 4
    # the val split of the same capture names the same training ids
    assert NerfiesDataset(root, split="val", image_scale=2, device="cpu").warp_ids == want_ids


# ---- losses.BackgroundLoss --------------------------------------------------------------------------------------------
def test_background_loss_constructor_refusals():
    pts = torch.zeros(10, 3)
    ok = losses.BackgroundLoss(pts, [3, 1, 2])
    assert (ok.batch_size, ok.noise_std, ok.scale, ok.weight) == (16384, 0.001, 0.001, 1.0)       # upstream's defaults
    assert ok.warp_ids.dtype == torch.int64 and ok.warp_ids.tolist() == [3, 1, 2]
    assert losses.BackgroundLoss(pts, torch.tensor([4, 9])).warp_ids.tolist() == [4, 9]
    for kw in (dict(points=torch.zeros(0, 3)), dict(warp_ids=[]), dict(warp_ids=torch.zeros(0, dtype=torch.int64)),
               dict(batch_size=0), dict(batch_size=-5), dict(scale=0.0), dict(scale=-1.0), dict(noise_std=-1e-3),
               dict(points=torch.zeros(10, 2)), dict(points=torch.zeros(10)), dict(points=torch.zeros(2, 5, 3)),
               dict(warp_ids=[1, 1]), dict(warp_ids=[-1, 2])):
        args = dict(points=pts, warp_ids=[0, 1])
        args.update(kw)
        with pytest.raises(ValueError):
            losses.BackgroundLoss(**args)
    losses.BackgroundLoss(pts, [0], noise_std=0.0)           # no noise is allowed


def test_background_loss_refuses_a_model_without_warp_and_cpu_tensors():
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    emb = {"warp": [0, 1], "camera": [0], "appearance": [0, 1], "time": [0, 1]}
    bg = losses.BackgroundLoss(torch.zeros(10, 3), [0, 1], batch_size=8)
    with pytest.raises(ValueError, match="use_warp"):
        bg(NerfModel(emb, n_samples_coarse=4, n_samples_fine=4, use_warp=False))
    m = NerfModel(emb, n_samples_coarse=4, n_samples_fine=4)
    with pytest.raises(ValueError, match="warp id"):
        losses.BackgroundLoss(torch.zeros(10, 3), [0, 2], batch_size=8)(m)
    rng = {"bg_u": torch.zeros(8, 2), "bg_n": torch.zeros(8, 3)}
    with pytest.raises(ValueError):
        bg(m, rng={"bg_u": torch.zeros(7, 2), "bg_n": torch.zeros(8, 3)})
    with pytest.raises(L.HnError):                           # no CPU fallback
        bg(m, rng=rng)


def test_functional_argument_errors():
    pts, ids = torch.zeros(4, 3), torch.zeros(2, dtype=torch.int64)
    u, nrm = torch.zeros(5, 2), torch.zeros(5, 3)
    for args in ((pts[:, :2], ids, u, nrm, 0.0), (pts, ids.float(), u, nrm, 0.0), (pts, ids, u[:, :1], nrm, 0.0),
                 (pts, ids, u, nrm[:4], 0.0), (pts, ids, u, nrm, -1.0), (pts[:0], ids, u, nrm, 0.0), (pts, ids[:0], u, nrm, 0.0)):
        with pytest.raises(ValueError):
            F.bg_sample(*args)
    big = torch.zeros(1, 3).expand((1 << 24) + 1, 3)         # a view: no memory behind it
    with pytest.raises(ValueError, match="2\\^24"):
        F.bg_sample(big, ids, u, nrm, 0.0)
    with pytest.raises(ValueError, match="2\\^24"):
        F.bg_sample(pts, torch.zeros(1, dtype=torch.int64).expand((1 << 24) + 1), u, nrm, 0.0)
    with pytest.raises(ValueError):
        F.bg_loss(nrm, nrm[:4], 0.001)
    with pytest.raises(ValueError):
        F.bg_loss(nrm, nrm, 0.0)
    with pytest.raises(L.HnError):
        F.bg_sample(pts, ids, u, nrm, 0.0)
    with pytest.raises(L.HnError):
        F.bg_loss(nrm, nrm, 0.001)


def test_train_step_refuses_background_draws_without_the_term():
    from hypernerf_torch_amd.training import TrainStep
    ts = TrainStep.__new__(TrainStep)                        # _split_rng is host bookkeeping only
    ts.background_loss = None
    assert ts._split_rng(None) == (None, None)
    rng = {"t_rand": torch.zeros(2, 3)}
    assert ts._split_rng(rng) == (rng, None)
    with pytest.raises(ValueError):
        ts._split_rng({"bg_u": torch.zeros(2, 2), "bg_n": torch.zeros(2, 3)})
    ts.background_loss = object()
    with pytest.raises(ValueError):
        ts._split_rng({"bg_u": torch.zeros(2, 2)})
    rest, bg = ts._split_rng({"t_rand": rng["t_rand"], "bg_u": torch.zeros(2, 2), "bg_n": torch.zeros(2, 3)})
    assert set(rest) == {"t_rand"} and set(bg) == {"bg_u", "bg_n"}
    rest, bg = ts._split_rng({"bg_u": torch.zeros(2, 2), "bg_n": torch.zeros(2, 3)})
    assert rest is None and set(bg) == {"bg_u", "bg_n"}


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    assert set(NEW_SYMBOLS) <= set(L.EXPORTS)
    assert "hn_regularizers.hip" in L.SOURCES
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    with open(L.HEADER) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name


FAKE = 0x1000          # a non-NULL device address nothing reads: every refusal comes before the first launch


def test_sampler_refuses_bad_arguments_before_any_launch():
    lib = L.load()

    def call(points=FAKE, m=10, ids=FAKE, k=3, u=FAKE, nrm=FAKE, n=8, std=0.001, out_points=FAKE, out_ids=FAKE):
        return lib.hn_bg_sample(points, m, ids, k, u, nrm, n, std, out_points, out_ids, None)

    for kw in (dict(points=None), dict(ids=None), dict(u=None), dict(nrm=None), dict(out_points=None), dict(out_ids=None),
               dict(n=0), dict(n=-3), dict(m=0), dict(m=-1), dict(k=0), dict(k=-2), dict(m=(1 << 24) + 1),
               dict(k=(1 << 24) + 1)):
        assert call(**kw) == -2, kw


def test_loss_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.load()

    def fwd(w=FAKE, p=FAKE, n=8, scale=0.001, out=FAKE):
        return lib.hn_bg_loss_forward(w, p, n, scale, out, None)

    def fwd_grad(w=FAKE, p=FAKE, n=8, scale=0.001, out=FAKE, dw=FAKE):
        return lib.hn_bg_loss_forward_grad(w, p, n, scale, out, dw, None)

    def bwd(w=FAKE, p=FAKE, n=8, scale=0.001, g=FAKE, dw=FAKE):
        return lib.hn_bg_loss_backward(w, p, n, scale, g, dw, None)

    common = (dict(w=None), dict(p=None), dict(n=0), dict(n=-1), dict(scale=0.0), dict(scale=-0.001),
              dict(scale=float("nan")))
    for kw in common + (dict(out=None),):
        assert fwd(**kw) == -2, kw
    for kw in common + (dict(out=None), dict(dw=None)):
        assert fwd_grad(**kw) == -2, kw
    for kw in common + (dict(g=None), dict(dw=None)):
        assert bwd(**kw) == -2, kw
