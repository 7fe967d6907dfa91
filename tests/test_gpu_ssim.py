"""GPU tests (MI355X) of the SSIM metric (metrics.py:15-20, kornia's ssim loss) and of the SSIM and depth outputs of the
eval loop (eval.py:50-54, 150-158), all against the float64 restatement in tests/ssim_restated.py.

Bounds, from the worst errors measured over this matrix (MI355X): per-pixel map 7.6e-6 abs, mean 9.4e-8 abs, sum
9.0e-6 rel (the 2 x 2 image, whose sum is smallest), gradients 6.8e-6 rel L2 (the 2 x 2 image).  The map's error is set
by the fp32 cancellation in E[x^2] - mu^2 next to C2 = 9e-4; on flat, dark windows it can reach 2e-4 per pixel, which
these random images do not have.  The errors of a run are logged through gpu_common (HN_PARITY_REPORT)."""
import os

import numpy as np
import pytest
import torch

import hashprng as H
import ssim_restated as R
from gpu_common import DEV, _record, assert_close, load_hash
import hypernerf_torch_amd as HN
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses
from hypernerf_torch_amd.hypernerf import models
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 2, 2), (1, 3, 4, 5), (1, 3, 17, 33), (2, 3, 63, 64), (1, 3, 65, 129), (1, 3, 378, 504)]
WINDOWS = [3, 5, 7, 11]
CASES = [(s, w) for s in SHAPES for w in WINDOWS if min(s[2], s[3]) > w // 2]
# the other radii the library is built for (15 is the dispatch's default branch), on one partial tile that reflects at
# both borders
CASES += [((1, 3, 17, 33), w) for w in (9, 13, 15)]
MAP_TOL, MEAN_TOL, SUM_REL_TOL, GRAD_REL_L2 = 3e-5, 3e-7, 1e-5, 3e-5


def _images(shape, content, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    if content == "noise":
        y = (x + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif content == "independent":
        y = torch.rand(shape, generator=g)
    else:
        y = x.clone()
    return x, y


def _on_gpu(t, layout):
    """(N, C, H, W) on the GPU, contiguous or as the (C, H, W) permute of (H, W, C) storage (N images side by side)."""
    if layout == "contiguous":
        return t.to(DEV)
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)


def _cid(case):
    s, w = case
    return "x".join(map(str, s)) + f"-w{w}"


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("layout", ["contiguous", "hwc"])
@pytest.mark.parametrize("content", ["noise", "independent", "identical"])
def test_ssim_forward_vs_restated(case, layout, content):
    shape, w = case
    x, y = _images(shape, content, 11 + w)
    ref = R.dssim(x, y, w, reduction="none")
    xg, yg = _on_gpu(x, layout), _on_gpu(y, layout)
    if layout == "hwc":
        assert not xg.is_contiguous()
    got = F.ssim_dssim(xg, yg, w, reduction="none")
    assert got.shape == shape and got.dtype == torch.float32
    err = float((got.double().cpu() - ref).abs().max())
    _record(f"ssim map {_cid(case)} {layout} {content}", "abs per pixel", err, MAP_TOL)
    assert err <= MAP_TOL, err
    mean = float(F.ssim_dssim(xg, yg, w, reduction="mean"))
    err = abs(mean - float(ref.mean()))
    _record(f"ssim mean {_cid(case)} {layout} {content}", "abs", err, MEAN_TOL)
    assert err <= MEAN_TOL, err
    total = float(F.ssim_dssim(xg, yg, w, reduction="sum"))
    rs = float(ref.sum())
    err = abs(total - rs) / max(abs(rs), 1e-30) if content != "identical" else abs(total - rs) / ref.numel()
    _record(f"ssim sum {_cid(case)} {layout} {content}", "rel" if content != "identical" else "abs / numel", err,
            SUM_REL_TOL)
    assert err <= SUM_REL_TOL, err
    if content == "identical":       # the dissimilarity of an image with itself is 0 up to eps / (C1 C2)
        assert float(got.max()) <= 1e-5


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("content", ["noise", "independent"])
def test_ssim_backward_vs_autograd(case, reduction, content):
    """d/dpred and d/dgt against torch.autograd through the restatement (F.pad reflect + conv2d): the smallest shapes
    put most pixels within the window radius of a border, where the reflected taps add to mirrored pixels."""
    shape, w = case
    x, y = _images(shape, content, 101 + w)
    up = torch.rand(shape, generator=torch.Generator().manual_seed(7)) - 0.3 if reduction == "none" else None
    xr, yr = x.double().requires_grad_(), y.double().requires_grad_()
    out = R.dssim(xr, yr, w, reduction=reduction)
    out.backward(up.double() if up is not None else None)
    layout = "hwc" if w == 5 else "contiguous"
    xg = _on_gpu(x, layout).requires_grad_()
    yg = _on_gpu(y, layout).requires_grad_()
    outg = F.ssim_dssim(xg, yg, w, reduction=reduction)
    outg.backward(up.to(DEV) if up is not None else None)
    for name, a, b in (("d_pred", xg.grad, xr.grad), ("d_gt", yg.grad, yr.grad)):
        err = _rel_l2(a, b)
        _record(f"ssim {name} {_cid(case)} {reduction} {content}", "rel L2", err, GRAD_REL_L2)
        assert err <= GRAD_REL_L2, (name, err)


@pytest.mark.parametrize("which", ["pred", "gt"])
def test_ssim_backward_one_input(which):
    """Only one image needs a gradient: the other stays None and the one asked for equals the two-input result."""
    shape, w = (1, 3, 17, 33), 5
    x, y = _images(shape, "noise", 5)
    xg, yg = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    losses.ssim(xg, yg).backward()
    x1, y1 = x.to(DEV).requires_grad_(which == "pred"), y.to(DEV).requires_grad_(which == "gt")
    losses.ssim(x1, y1).backward()
    if which == "pred":
        assert y1.grad is None and torch.equal(x1.grad, xg.grad)
    else:
        assert x1.grad is None and torch.equal(y1.grad, yg.grad)


def test_losses_ssim_is_metrics_ssim():
    """metrics.py:15-20: 1 - 2 * dssim(pred, gt, 3, reduction), in [-1, 1], on (1, 3, H, W) images."""
    x, y = _images((1, 3, 40, 50), "noise", 9)
    got = losses.ssim(x.to(DEV), y.to(DEV))
    assert got.shape == () and abs(float(got) - float(R.ssim(x.double(), y.double()))) <= 4e-6
    m = losses.ssim(x.to(DEV), y.to(DEV), reduction="none")
    assert m.shape == (1, 3, 40, 50)
    assert float((m.double().cpu() - R.ssim(x.double(), y.double(), reduction="none")).abs().max()) <= 4e-4
    assert float(losses.ssim(x.to(DEV), x.to(DEV))) > 1 - 2e-5


@pytest.mark.parametrize("w", [3, 11])
def test_ssim_runs_are_bit_identical(w):
    shape = (1, 3, 378, 504)
    x, y = _images(shape, "noise", 21)
    res = []
    for _ in range(2):
        xg, yg = _on_gpu(x, "hwc").requires_grad_(), _on_gpu(y, "hwc").requires_grad_()
        s = F.ssim_dssim(xg, yg, w, reduction="sum")
        m = F.ssim_dssim(xg, yg, w, reduction="none")
        (s + (m * 0.5).sum()).backward()
        torch.cuda.synchronize()
        res.append([t.detach().cpu() for t in (s, m, xg.grad, yg.grad)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_ssim_backward_graph_replay_matches_eager():
    """losses.ssim(...).backward() captured in a HIP graph and replayed on new image contents gives the eager result
    bit for bit (the upstream gradient stays on the device, the workspace comes from the graph's pool)."""
    shape = (1, 3, 65, 129)
    x0, y0 = _images(shape, "noise", 31)
    x1, y1 = _images(shape, "independent", 32)
    pred = _on_gpu(x0, "contiguous").requires_grad_()
    gt = _on_gpu(y0, "hwc")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            pred.grad = None
            losses.ssim(pred, gt).backward()
    torch.cuda.current_stream().wait_stream(s)
    pred.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = losses.ssim(pred, gt)
        loss.backward()
    with torch.no_grad():
        pred.copy_(x1.to(DEV))
        gt.copy_(_on_gpu(y1, "hwc"))
    graph.replay()
    torch.cuda.synchronize()
    got_loss, got_grad = loss.detach().cpu().clone(), pred.grad.detach().cpu().clone()
    pe = _on_gpu(x1, "contiguous").requires_grad_()
    le = losses.ssim(pe, _on_gpu(y1, "hwc"))
    le.backward()
    assert torch.equal(got_loss, le.detach().cpu())
    assert torch.equal(got_grad, pe.grad.cpu())
    assert abs(float(got_loss) - float(R.ssim(x1.double(), y1.double()))) <= 4e-6


# ------------------------------------------------------------------------------------------------------------------
# eval loop: the setup of tests/test_gpu_training.py::test_eval_image_loop_vs_oracle_deterministic
# ------------------------------------------------------------------------------------------------------------------
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
EMB = {"warp": list(range(100)), "camera": [0], "appearance": list(range(100)), "time": list(range(100))}


def small_model(seed, nc=16, nf=16, noise_std=None, precision="fp32"):
    HN.set_precision(precision)
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=noise_std, **KW)
    sd = load_hash(m, seed)
    return m.to(DEV), sd


def test_eval_ssim_and_depth_files(tmp_path):
    """evaluate_images adds 'ssims' / 'mean_ssim' (metrics.ssim of every image with ground truth) and, with
    save_depth, writes the depth maps as PFM or raw float32; everything it returned before is unchanged."""
    from hypernerf_torch_amd.inference import evaluate_images, read_pfm, read_png
    h, w, focal = 6, 8, 7.5
    m, sd = small_model(61, 16, 16, noise_std=None, precision="fp32")
    m = m.eval()
    m.use_stratified_sampling = False
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.2], [0.0, 0.0, 1.0, 1.5]])
    cfg = O.ModelCfg(n_samples_coarse=16, n_samples_fine=16, noise_std=None, **KW)
    samples, refs = [], []
    for img_id in (3, 7):
        rays = F.generate_rays(h, w, focal, c2w.to(DEV), near=0.0, far=1.0, ndc=False, image_id=img_id)
        ref_rays = O.image_rays(h, w, focal, c2w, 0.0, 1.0, False, image_id=img_id)
        o, d = ref_rays[:, 0:3], ref_rays[:, 3:6]
        idx = torch.full((h * w,), img_id, dtype=torch.int64)
        u = torch.linspace(0, 1, 16).expand(h * w, -1).contiguous()
        ref = O.nerf_model_forward({k: v.clone() for k, v in sd.items()}, cfg, o, d, idx, {"t_rand": None, "u": u})
        gt = (ref["fine"]["rgb"] + 0.02 * H.uniform(61 + img_id, "gt", (h * w, 3), -1, 1)).clamp(0, 1)
        refs.append((ref["fine"]["rgb"], ref["fine"]["depth"], gt))
        samples.append({"rays": rays, "rgbs": gt.to(DEV), "hw": (h, w)})
    base_dir, pfm_dir, raw_dir = (str(tmp_path / d) for d in ("base", "pfm", "raw"))
    base = evaluate_images(m, samples, chunk=20, save_dir=base_dir)
    res = evaluate_images(m, samples, chunk=20, save_dir=pfm_dir, save_depth=True)
    raw = evaluate_images(m, samples, chunk=20, save_dir=raw_dir, save_depth=True, depth_format="bytes")
    assert len(res["ssims"]) == 2
    for i, (rgb, depth, gt) in enumerate(refs):
        chw = lambda t: t.view(h, w, 3).permute(2, 0, 1)[None].double()      # noqa: E731
        want = float(R.ssim(chw(rgb), chw(gt)))
        _record(f"eval ssim image {i} vs restated on the oracle's image", "abs", abs(res["ssims"][i] - want), 1e-5)
        assert abs(res["ssims"][i] - want) <= 1e-5, (res["ssims"][i], want)
        for r in (base, res, raw):
            assert r["ssims"][i] == res["ssims"][i]
            assert torch.equal(r["depths"][i], base["depths"][i]) and torch.equal(r["images"][i], base["images"][i])
            assert r["psnrs"][i] == base["psnrs"][i]
        d_pfm, scale = read_pfm(os.path.join(pfm_dir, f"depth_{i:03d}.pfm"))
        assert scale == 1.0 and np.array_equal(d_pfm, res["depths"][i].numpy())
        d_raw = np.fromfile(os.path.join(raw_dir, f"depth_{i:03d}"), dtype=np.float32).reshape(h, w)
        assert np.array_equal(d_raw, res["depths"][i].numpy())
        for dd in (pfm_dir, raw_dir):
            assert np.array_equal(read_png(os.path.join(dd, f"{i:03d}.png")), read_png(os.path.join(base_dir, f"{i:03d}.png")))
        assert_close(res["depths"][i], depth.view(h, w), 1e-4, f"image {i} depth")
    assert not os.path.exists(os.path.join(base_dir, "depth_000.pfm"))
    assert not any(n.startswith("depth_") for n in os.listdir(raw_dir) if n.endswith(".pfm"))
    assert abs(res["mean_ssim"] - sum(res["ssims"]) / 2) < 1e-12
    assert base["mean_psnr"] == res["mean_psnr"]
    none = evaluate_images(m, [{"rays": samples[0]["rays"], "hw": (h, w)}], chunk=20)
    assert none["ssims"] == [] and none["mean_ssim"] is None
