"""GPU tests (MI355X) of multi-scale SSIM (hn_msssim_*, functional.msssim_levels, losses.ms_ssim) and of its output in
the eval loop, against the float64 restatement in tests/msssim_restated.py.

Tolerance of the per-level values: not a fixed number.  The restatement is evaluated once in float32 on the CPU for
every input of the matrix below; the largest float32-vs-float64 difference of any per-level value, times 4, is what the
kernel may differ from the float64 values by (it sums in another order and adds the rounding of the tile sums).  The
derived figure is about 1e-4 (it comes from the fp32 cancellation in E[x^2] - mu^2 next to c2 = 9e-4); the derived
bound and the kernel's worst error of a run are logged through gpu_common (HN_PARITY_REPORT) and quoted in DESIGN.md.
The product of the five terms is compared where the restatement's is finite, with the first-order bound
prod * sum_l w_l * TOL / term_l that the per-level tolerance implies (plus 1e-6 for fp32 pow and the product); where a
term is negative both sides must be NaN."""
import functools

import pytest
import torch

import hashprng as H
import msssim_restated as R
from gpu_common import DEV, _record, load_hash
import hypernerf_torch_amd as HN
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses
from hypernerf_torch_amd.hypernerf import models

pytestmark = pytest.mark.gpu

# the level kernel stages a 32 x 16 tile + a 10-pixel halo (42 x 26): 29 x 45 exceeds that by 3 in both axes
SHAPES = [(1, 3, 5, 7), (1, 3, 16, 16), (2, 3, 37, 53), (1, 1, 64, 48), (1, 3, 29, 45)]
CONTENTS = ["sigma0.02", "sigma0.1", "sigma0.3", "independent", "identical"]


def _images(shape, content, seed=0):
    """gt = smooth pattern + 0.05 noise, clipped; pred = clip(gt + sigma noise), independent uniform noise, or gt."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ch = torch.arange(c, dtype=torch.float32).view(1, c, 1, 1)
    im = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1)
    base = 0.5 + 0.35 * torch.sin(0.31 * xx + 0.17 * yy + 0.7 * im) * torch.cos(0.9 * ch + 0.05 * yy)
    gt = (base + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    if content == "independent":
        # the correlation of two independent draws scatters around 0: this draw's level-0 values at 37 x 53 are negative
        # for both images (the NaN case)
        g = torch.Generator().manual_seed(1000 * h + w + 2)
        torch.randn(shape, generator=g)
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if content == "identical":
        return gt.clone(), gt
    sigma = float(content[len("sigma"):])
    return (gt + sigma * torch.randn(shape, generator=g)).clamp(0, 1), gt


@functools.lru_cache(maxsize=None)
def _reference(shape, content):
    """(pred, gt, float64 levels, float32-vs-float64 difference): computed once, shared by every test, never changed."""
    pred, gt = _images(shape, content)
    lv64 = R.levels(pred, gt)
    lv32 = R.levels(pred, gt, dtype=torch.float32)
    return pred, gt, lv64, float((lv32.double() - lv64).abs().max())


@functools.lru_cache(maxsize=None)
def _tolerance():
    tol = 4 * max(_reference(s, c)[3] for s in SHAPES for c in CONTENTS)
    _record("ms-ssim per-level tolerance = 4 x worst fp32-vs-fp64 restatement difference", "abs", tol, tol)
    return tol


def _product_bound(lv64):
    """What the per-level tolerance allows the product to differ by, to first order, + 1e-6 for fp32 pow / product."""
    terms = torch.cat([lv64[:, :4, 1], lv64[:, 4:, 0]], dim=1)
    w = torch.tensor(R.WEIGHTS, dtype=torch.float64)
    return R.product(lv64).abs() * (w * _tolerance() / terms.abs()).sum(dim=1) + 1e-6


def _on_gpu(t, layout):
    if layout == "contiguous":
        return t.to(DEV)
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)


def _sid(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("layout", ["contiguous", "hwc"])
@pytest.mark.parametrize("content", CONTENTS)
def test_levels_vs_restated(shape, layout, content):
    pred, gt, lv64, _ = _reference(shape, content)
    tol = _tolerance()
    assert 1e-6 < tol < 1e-3, tol
    terms = torch.cat([lv64[:, :4, 1], lv64[:, 4:, 0]], dim=1)
    assert float(terms.abs().min()) > 2 * tol            # no term so close to 0 that its sign is within the tolerance
    if content.startswith("sigma"):
        assert float(terms.min()) > 0
    if content == "independent" and shape == (2, 3, 37, 53):
        assert bool((lv64[:, 0] < 0).all())
    xg, yg = _on_gpu(pred, layout), _on_gpu(gt, layout)
    if layout == "hwc" and shape[1] > 1:
        assert not xg.is_contiguous()
    got = F.msssim_levels(xg, yg)
    assert got.shape == (shape[0], 5, 2) and got.dtype == torch.float32 and not got.requires_grad
    err = float((got.double().cpu() - lv64).abs().max())
    print(f"ms-ssim levels {_sid(shape)} {layout} {content}: err {err:.3e} tol {tol:.3e}")
    _record(f"ms-ssim levels {_sid(shape)} {layout} {content}", "abs per level", err, tol)
    assert err <= tol, (err, tol)
    want = R.product(lv64)
    prod = losses.ms_ssim(xg, yg, reduction="none").double().cpu()
    assert prod.shape == (shape[0],)
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(prod), ~finite)
    if content.startswith("sigma") or content == "identical":
        assert bool(finite.all())
    if finite.any():
        bound = _product_bound(lv64)
        perr = (prod - want).abs()
        print(f"ms-ssim product {_sid(shape)} {layout} {content}: err {float(perr[finite].max()):.3e}")
        assert bool((perr[finite] <= bound[finite]).all()), (perr, bound)
    if content == "identical":
        assert float((got.double().cpu() - 1).abs().max()) <= 1e-6 and float((prod - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_losses_ms_ssim_is_the_product_of_the_levels(reduction):
    shape = (2, 3, 37, 53)
    pred, gt, lv64, _ = _reference(shape, "sigma0.1")
    want = R.product(lv64)
    got = losses.ms_ssim(pred.to(DEV), gt.to(DEV), reduction=reduction)
    assert not got.requires_grad and got.dtype == torch.float32
    bound = _product_bound(lv64)
    if reduction == "mean":
        assert got.shape == () and abs(float(got) - float(want.mean())) <= float(bound.max())
    else:
        assert got.shape == (2,) and bool(((got.double().cpu() - want).abs() <= bound).all())
    # inputs that require grad do not make the metric differentiable
    assert not losses.ms_ssim(pred.to(DEV).requires_grad_(), gt.to(DEV)).requires_grad


def test_runs_are_bit_identical():
    pred, gt, _, _ = _reference((2, 3, 37, 53), "sigma0.3")
    res = []
    for _ in range(2):
        xg, yg = _on_gpu(pred, "hwc"), _on_gpu(gt, "contiguous")
        lv = F.msssim_levels(xg, yg)
        p = losses.ms_ssim(xg, yg, reduction="none")
        torch.cuda.synchronize()
        res.append((lv.cpu(), p.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_graph_replay_matches_eager():
    """losses.ms_ssim captured in a HIP graph and replayed on new image contents gives the eager result bit for bit
    (the host taps and sizes are consumed at the launch, the workspace comes from the graph's pool)."""
    shape = (1, 3, 29, 45)
    x0, y0, _, _ = _reference(shape, "sigma0.02")
    x1, y1, lv64, _ = _reference(shape, "sigma0.3")
    pred, gt = _on_gpu(x0, "contiguous"), _on_gpu(y0, "hwc")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            losses.ms_ssim(pred, gt)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = losses.ms_ssim(pred, gt)
    pred.copy_(x1.to(DEV))
    gt.copy_(_on_gpu(y1, "hwc"))
    graph.replay()
    torch.cuda.synchronize()
    got = out.cpu().clone()
    eager = losses.ms_ssim(_on_gpu(x1, "contiguous"), _on_gpu(y1, "hwc")).cpu()
    assert torch.equal(got, eager)
    assert abs(float(got) - float(R.product(lv64))) <= float(_product_bound(lv64))


# ------------------------------------------------------------------------------------------------------------------
# eval loop: the small-model setup of tests/test_gpu_ssim.py
# ------------------------------------------------------------------------------------------------------------------
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
EMB = {"warp": list(range(100)), "camera": [0], "appearance": list(range(100)), "time": list(range(100))}


def small_model(seed, nc=16, nf=16, noise_std=None, precision="fp32"):
    HN.set_precision(precision)
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=noise_std, **KW)
    load_hash(m, seed)
    return m.to(DEV)


def test_eval_loop_reports_ms_ssim():
    """evaluate_images(ms_ssim=True) adds 'ms_ssims' / 'mean_ms_ssim' (losses.ms_ssim of every frame with ground truth,
    on the frame it rendered); the default returns exactly today's keys."""
    from hypernerf_torch_amd.inference import evaluate_images, render_image
    h, w, focal = 12, 10, 9.5
    m = small_model(61).eval()
    m.use_stratified_sampling = False
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.2], [0.0, 0.0, 1.0, 1.5]])
    samples, frames = [], []
    with torch.no_grad():
        for img_id in (3, 7):
            rays = F.generate_rays(h, w, focal, c2w.to(DEV), near=0.0, far=1.0, ndc=False, image_id=img_id)
            img = render_image(m, rays, chunk=50, keys=("rgb", "depth"))["rgb"].view(h, w, 3)
            gt = (img.cpu() + 0.02 * H.uniform(61 + img_id, "gt", (h, w, 3), -1, 1)).clamp(0, 1).to(DEV)
            frames.append((img, gt))
            samples.append({"rays": rays, "rgbs": gt.view(h * w, 3), "hw": (h, w)})
    base = evaluate_images(m, samples, chunk=50)
    res = evaluate_images(m, samples, chunk=50, ms_ssim=True)
    assert set(base) == {"images", "depths", "psnrs", "mean_psnr", "ssims", "mean_ssim"}
    assert set(res) == set(base) | {"ms_ssims", "mean_ms_ssim"}
    assert len(res["ms_ssims"]) == 2
    for i, (img, gt) in enumerate(frames):
        want = float(losses.ms_ssim(img.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None]))
        assert res["ms_ssims"][i] == want and 0 < want <= 1, (res["ms_ssims"][i], want)
        assert res["psnrs"][i] == base["psnrs"][i] and res["ssims"][i] == base["ssims"][i]
        assert torch.equal(res["images"][i], base["images"][i])
    assert abs(res["mean_ms_ssim"] - sum(res["ms_ssims"]) / 2) < 1e-12
    none = evaluate_images(m, [{"rays": samples[0]["rays"], "hw": (h, w)}], chunk=50, ms_ssim=True)
    assert none["ms_ssims"] == [] and none["mean_ms_ssim"] is None
