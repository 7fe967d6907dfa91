"""GPU tests (MI355X) of LPIPS (hn_lpips_*, ops.lpips, losses.lpips) and of its output in the eval loop, with seeded random
weights, against the float64 restatement in tests/lpips_restated.py.

Per-layer features: every convolution is fed the kernel's OWN previous output and compared with the float64 convolution of
that same input, elementwise, under the bound of a K-term fp32 fma chain plus the bias add:
    |err| <= (K + 2) * 2^-24 * (conv(|x|, |w|) + |b|),   K = cin * k * k.
Max pools are compared bit for bit.

Final values: relative tolerance 8 * F32_DEVIATION.  F32_DEVIATION = 1.49e-6 is the worst relative deviation of the
restatement itself run in float32 on the CPU from its float64 run, over the five layer terms and their sum of the six cases
of lpips_restated.CASES (lpips_restated.float32_deviation(); per case 1.12e-6, 9.66e-7, 9.57e-7, 1.49e-6, 8.06e-7,
1.05e-7).  The kernels are in the same arithmetic class (fp32 products and sums) and differ in the order of the sums over
channels and pixels: a factor of 8 over the CPU's own float32 run.  Neither figure comes from the kernels' output."""
import functools

import pytest
import torch

import hashprng as H
import lpips_restated as R
from gpu_common import DEV, EMB, _record, load_hash
import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import losses
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.ops import lpips as P

pytestmark = pytest.mark.gpu

F32_DEVIATION = 1.49e-6          # measured on the CPU, see the module docstring
TOL = 8 * F32_DEVIATION
U = 2.0 ** -24
REFUSED = (ValueError, L.HnError)


@functools.lru_cache(maxsize=None)
def _raw(net):
    return R.random_weights(net, R.WEIGHT_SEED[net])


@functools.lru_cache(maxsize=None)
def _weights(net):
    return P.lpips_weights_from_state_dicts(net, *R.split_state_dicts(net, _raw(net))).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(net, n, h, w):
    """(pred, gt, float64 layer terms (N, 5)) of one case, computed once."""
    pred, gt = R.image_pair(n, h, w, h * w)
    return pred, gt, R.lpips_layers(net, _raw(net), pred, gt)


def _close(what, got, want):
    got, want = got.double().cpu(), want.double()
    rel = float(((got - want).abs() / want.abs()).max())
    print(f"{what}: worst relative error {rel:.3e} (bound {TOL:.3e})")
    _record(what, "lpips", rel, TOL)
    assert ((got - want).abs() <= TOL * want.abs()).all(), (what, rel, TOL, got, want)


# ---- per-layer features -----------------------------------------------------------------------------------------------------
# 49 output pixels and K = 363 (odd) / 7 x 11 pixels, two pairs / 35 x 64 / a 1 x 1 last tap and K up to 4608 / odd sides
# through four floor-mode pools
LAYER_CASES = [("alex", 1, 31, 31), ("alex", 2, 32, 47), ("alex", 1, 35, 64), ("vgg", 1, 16, 16), ("vgg", 2, 17, 23)]


@pytest.mark.parametrize("net,n,h,w", LAYER_CASES)
def test_every_layer_against_float64_on_the_kernels_own_input(net, n, h, w):
    pred, gt, _ = _case(net, n, h, w)
    weights, raw = _weights(net), _raw(net)
    x = R.prepare(torch.cat([pred, gt]), torch.float32).to(DEV)
    walked, ci, worst = [], 0, 0.0
    for layer in R.NETS[net]:
        x_cpu = x.cpu()
        if layer[0] == "pool":
            x = P.lpips_maxpool(x, layer[2], layer[3])
            assert torch.equal(x.cpu(), R.pool_layer(x_cpu, layer)), layer
            continue
        wgt, bias = raw["convs"][ci]
        y = P.lpips_conv(x, weights.convs[ci], layer[4], layer[5], layer[6])
        for tile in (1, 2, 3):      # the three tile shapes give the same bits
            assert torch.equal(P.lpips_conv(x, weights.convs[ci], layer[4], layer[5], layer[6], tile=tile), y), (layer, tile)
        ci += 1
        k = layer[2] * layer[4] * layer[4]
        pre = R.conv_layer(x_cpu.double(), layer, wgt, bias, relu=False)
        bound = (k + 2) * U * R.conv_bound(x_cpu, layer, wgt, bias)
        got = y.cpu().double()
        assert got.shape == pre.shape
        err = (got - pre.clamp(min=0)).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (layer, float((err / bound).max()))
        assert (got[pre < -bound] == 0).all() and (got[pre > bound] > 0).all() and (got >= 0).all(), layer
        x = y
        if layer[7]:
            walked.append(y)
    print(f"{net} {n}x{h}x{w}: worst |err| / bound over the layers {worst:.3f}")
    _record(f"lpips layers {net} {n}x{h}x{w}", "err/bound", worst, 1.0)
    # lpips_features is this walk
    taps = P.lpips_features(R.prepare(torch.cat([pred, gt]), torch.float32).to(DEV), weights)
    assert len(taps) == len(walked) == 5 and all(torch.equal(a, b) for a, b in zip(taps, walked))


def test_prepare_is_the_scaling_and_an_outside_tap_is_zero():
    """hn_lpips_prepare against float64, and conv1's zero padding in the SCALED domain: on an image whose scaled value is
    a constant c, a corner output misses exactly the taps outside the image (they count 0, not the scaled value of 0)."""
    pred, gt, _ = _case("alex", 2, 32, 47)
    x = P.lpips_prepare(pred.to(DEV), gt.to(DEV), "alex").cpu()
    want = R.prepare(torch.cat([pred, gt]))
    assert x.shape == want.shape and ((x.double() - want).abs() <= 4 * U * want.abs() + 2 * U).all()
    layer, (wgt, bias) = R.NETS["alex"][0], _raw("alex")["convs"][0]
    const = torch.full((1, 3, 31, 31), 0.75)
    y = P.lpips_conv(const.to(DEV), _weights("alex").convs[0], 11, 4, 2, relu=False).cpu().double()
    pre = R.conv_layer(const.double(), layer, wgt, bias, relu=False)
    assert ((y - pre).abs() <= 365 * U * R.conv_bound(const, layer, wgt, bias)).all()
    assert not torch.allclose(pre[0, :, 0, 0], pre[0, :, 3, 3])      # the corner does see the padding


# ---- final values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n,h,w", R.CASES)
def test_layer_terms_and_sum_against_float64(net, n, h, w):
    pred, gt, want = _case(net, n, h, w)
    got = P.lpips_layers(pred.to(DEV), gt.to(DEV), _weights(net))
    assert got.shape == (n, 5) and got.dtype == torch.float32 and not got.requires_grad
    _close(f"lpips layer terms {net} {n}x{h}x{w}", got, want)
    total = losses.lpips(pred.to(DEV), gt.to(DEV), _weights(net), reduction="none")
    assert total.shape == (n,)
    _close(f"lpips {net} {n}x{h}x{w}", total, want.sum(1))
    mean = losses.lpips(pred.to(DEV), gt.to(DEV), _weights(net))
    assert mean.shape == () and abs(float(mean) - float(want.sum(1).mean())) <= TOL * float(want.sum(1).mean())


# ---- exact facts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,h,w", [("alex", 32, 47), ("vgg", 17, 23)])
def test_exact_facts(net, h, w):
    pred, gt, _ = _case(net, 2, h, w)
    pred, gt, weights = pred.to(DEV), gt.to(DEV), _weights(net)
    ab = P.lpips_layers(pred, gt, weights)
    assert (ab > 0).all()
    assert torch.equal(P.lpips_layers(pred, pred, weights), torch.zeros(2, 5, device=DEV))      # lpips(x, x) == 0
    assert float(losses.lpips(gt, gt, weights)) == 0.0
    assert torch.equal(P.lpips_layers(gt, pred, weights), ab)                                   # symmetric, bit for bit
    assert torch.equal(P.lpips_layers(pred, gt, weights), ab)                                   # run to run
    for i in range(2):                                                                          # N = 2 is two N = 1 calls
        assert torch.equal(P.lpips_layers(pred[i:i + 1], gt[i:i + 1], weights), ab[i:i + 1])
    # an (H, W, 3) frame as a strided view gives the bits of its contiguous copy
    frame_p, frame_g = pred[0].permute(1, 2, 0).contiguous(), gt[0].permute(1, 2, 0).contiguous()
    view_p, view_g = frame_p.permute(2, 0, 1)[None], frame_g.permute(2, 0, 1)[None]
    assert not view_p.is_contiguous()
    assert torch.equal(P.lpips_layers(view_p, view_g, weights), ab[:1])
    assert torch.equal(P.lpips_layers(view_p, gt[:1], weights), ab[:1])


def test_constant_images():
    """Features that are the same at every interior pixel: nothing degenerates, and the value is the restatement's."""
    pred, gt = torch.full((1, 3, 33, 40), 0.3), torch.full((1, 3, 33, 40), 0.6)
    for net in ("alex", "vgg"):
        want = R.lpips_layers(net, _raw(net), pred, gt)
        got = P.lpips_layers(pred.to(DEV), gt.to(DEV), _weights(net))
        assert torch.isfinite(got).all()
        _close(f"lpips constant images {net}", got, want)


def test_a_tap_that_is_all_zero_gives_a_finite_value_and_a_zero_term():
    raw = R.random_weights("alex", R.WEIGHT_SEED["alex"])
    raw["convs"][2] = (raw["convs"][2][0], torch.full_like(raw["convs"][2][1], -10.0))
    weights = P.lpips_weights_from_state_dicts("alex", R.full_state_dict("alex", raw)).to(DEV)
    pred, gt, _ = _case("alex", 2, 32, 47)
    got = P.lpips_layers(pred.to(DEV), gt.to(DEV), weights)
    taps = P.lpips_features(P.lpips_prepare(pred.to(DEV), gt.to(DEV), "alex"), weights)
    assert not taps[2].any() and taps[1].any()
    assert torch.isfinite(got).all() and (got[:, 2] == 0).all() and (got[:, :2] > 0).all()
    assert torch.equal(got[:, :2], P.lpips_layers(pred.to(DEV), gt.to(DEV), _weights("alex"))[:, :2])
    assert torch.isfinite(losses.lpips(pred.to(DEV), gt.to(DEV), weights))
    _close("lpips with a dead tap", got[:, :2], R.lpips_layers("alex", raw, pred, gt)[:, :2])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    pred, gt, _ = _case("alex", 1, 31, 31)
    a, b, weights = pred.to(DEV), gt.to(DEV), _weights("alex")
    cpu_weights = P.lpips_weights_from_state_dicts("alex", *R.split_state_dicts("alex", _raw("alex")))
    assert cpu_weights.to(DEV) is cpu_weights.to(DEV) and cpu_weights.to(DEV).device == torch.device(DEV)
    vgg_small = torch.rand(1, 3, 15, 20, device=DEV)
    for call in (lambda: losses.lpips(pred, gt, weights),                      # CPU tensors
                 lambda: losses.lpips(a, gt, weights),
                 lambda: losses.lpips(a[:, :2], b[:, :2], weights),            # C != 3
                 lambda: losses.lpips(a.double(), b.double(), weights),        # float64
                 lambda: losses.lpips(a[..., :30], b[..., :30], weights),      # a side below the minimum
                 lambda: losses.lpips(a[:, :, :30], b[:, :, :30], weights),
                 lambda: losses.lpips(vgg_small, vgg_small, _weights("vgg")),
                 lambda: losses.lpips(a, b[..., :30], weights),                # mismatched shapes
                 lambda: losses.lpips(a[0], b[0], weights),
                 lambda: losses.lpips(a, b, cpu_weights),                      # weights on another device
                 lambda: losses.lpips(a, b, P.lpips_weights_from_state_dicts(
                     "vgg", *R.split_state_dicts("vgg", _raw("vgg")))),        # the other net's, on another device
                 lambda: losses.lpips(a, b, "alex"),
                 lambda: losses.lpips(a, b, weights, reduction="sum"),
                 lambda: P.lpips_features(a.cpu(), weights),
                 lambda: P.lpips_features(a[..., :30], weights)):
        with pytest.raises(REFUSED):
            call()
    # the other net's weights on the right device are a legal request: a 31 x 31 image is large enough for 'vgg'
    assert torch.isfinite(losses.lpips(a, b, _weights("vgg")))


# ---- eval loop --------------------------------------------------------------------------------------------------------------
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)


def test_eval_loop_reports_lpips():
    """evaluate_images(lpips=weights) adds 'lpips' / 'mean_lpips' (losses.lpips of every frame with ground truth, on the
    frame it rendered); the default returns exactly today's keys."""
    from hypernerf_torch_amd.inference import evaluate_images, render_image
    old = HN.get_precision()
    try:
        HN.set_precision("fp32")
        h, w, focal = 32, 36, 30.5
        m = models.NerfModel(EMB, n_samples_coarse=16, n_samples_fine=16, noise_std=None, **KW)
        load_hash(m, 61)
        m = m.to(DEV).eval()
        m.use_stratified_sampling = False
        weights = _weights("alex")
        c2w = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.2], [0.0, 0.0, 1.0, 1.5]])
        samples, frames = [], []
        with torch.no_grad():
            for img_id in (3, 7):
                rays = F.generate_rays(h, w, focal, c2w.to(DEV), near=0.0, far=1.0, ndc=False, image_id=img_id)
                img = render_image(m, rays, chunk=h * w, keys=("rgb", "depth"))["rgb"].view(h, w, 3)
                gt = (img.cpu() + 0.02 * H.uniform(61 + img_id, "gt", (h, w, 3), -1, 1)).clamp(0, 1).to(DEV)
                frames.append((img, gt))
                samples.append({"rays": rays, "rgbs": gt.view(h * w, 3), "hw": (h, w)})
        base = evaluate_images(m, samples, chunk=h * w)
        res = evaluate_images(m, samples, chunk=h * w, lpips=weights)
        assert set(base) == {"images", "depths", "psnrs", "mean_psnr", "ssims", "mean_ssim"}
        assert set(res) == set(base) | {"lpips", "mean_lpips"}
        assert len(res["lpips"]) == 2
        for i, (img, gt) in enumerate(frames):
            want = float(losses.lpips(img.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None], weights))
            assert res["lpips"][i] == want and want > 0, (res["lpips"][i], want)
            assert res["psnrs"][i] == base["psnrs"][i] and res["ssims"][i] == base["ssims"][i]
            assert torch.equal(res["images"][i], base["images"][i])
        assert abs(res["mean_lpips"] - sum(res["lpips"]) / 2) < 1e-12
        none = evaluate_images(m, [{"rays": samples[0]["rays"], "hw": (h, w)}], chunk=h * w, lpips=weights)
        assert none["lpips"] == [] and none["mean_lpips"] is None
    finally:
        HN.set_precision(old)
