"""GPU parity of the per-ray render kernels up to their 512-sample limit (MI355X).

Compositing (hn_composite_*) against the oracle in float64, the inverse-CDF sampler (hn_sample_pdf[_split],
hn_composite_sample_pdf) bit for bit against the oracle, hn_depth_index bit for bit against NumPy on weights whose
partial sums are exact, and whole models at 512 samples per ray — every segment of 64 samples of a ray, and the merge
of more than 256 coarse depths, which the rank merge does not cover (it falls back to the bitonic sort there)."""
import os

import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
from gpu_common import DEV, EMB, _record, assert_close, assert_grad_close, load_hash, rays_for
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import model_utils as MU
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.models import nerf as legacy_nerf
from hypernerf_torch_amd.models import rendering as legacy_rendering
from oracle import hypernerf_oracle as O
from test_gpu_model import grad_stats_close, rng_from_fixture

pytestmark = pytest.mark.gpu

COMP_S = [63, 64, 65, 255, 256, 257, 320, 383, 384, 448, 511, 512]
G19 = "g19_long_rays.npz"


def g19(golden_dir):
    return np.load(os.path.join(golden_dir, G19))


# ---- compositing --------------------------------------------------------------------------------------------------
def comp_inputs(s, seed):
    """Rays of S samples: one transparent, one opaque at its first sample, one with density only from sample k on for
    k in every segment of 64 (the carried transmittance and the median crossing in that segment), random ones."""
    nseg = (s + 63) // 64
    onsets = [min(s - 1, 64 * k + 17 * k % 64) for k in range(nseg)] + [s - 1]
    b = 2 + len(onsets) + 4
    o, d, _ = rays_for(seed, b)
    rgb = H.uniform(seed, "rgb", (b, s, 3), 0, 1)
    raw = H.uniform(seed, "raw", (b, s), -3, 4)
    raw[0] = -40.0
    raw[1] = -40.0
    raw[1, 0] = 30.0
    for r, k in enumerate(onsets, start=2):
        raw[r, :k] = -40.0
        raw[r, k:] += 3.0
    z, _ = torch.sort(H.uniform(seed, "z", (b, s), 0, 1), dim=-1)
    noise = H.normal(seed, "noise", (b, s))
    warped = H.uniform(seed, "wp", (b, s, 7), -1, 1)
    keep = (H.uniform(seed, "keep", (b, s), 0, 1) > 0.1).float()
    return o, d, rgb, raw, z, noise, warped, keep


def ref_composite(rgb, raw, z, d, variant, white_bg, sai, noise, noise_scale, dust, keep):
    """The compositing in float64: variant 0 = model_utils.volumetric_rendering on softplus densities (the oracle),
    variant 1 = the legacy nerf_pl arithmetic (models/rendering.py:150-165, restated as in test_composite_vs_oracle).
    Returns (rgb, depth, acc, weights)."""
    x = raw + noise * noise_scale if noise is not None else raw
    sigma = torch.nn.functional.softplus(x) if variant == 0 else torch.relu(x)
    if dust is not None:
        sigma = (sigma >= dust) * sigma
    if keep is not None:
        sigma = keep * sigma
    if variant == 0:
        r = O.volumetric_rendering(rgb, sigma, z, d, white_bg=white_bg, sample_at_infinity=sai)
        return r["rgb"], r["depth"], r["acc"], r["weights"]
    deltas = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(d[:, None, :], dim=-1)
    alphas = 1 - torch.exp(-deltas * sigma)
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-10], -1)
    w = alphas * torch.cumprod(shifted, -1)[:, :-1]
    acc = w.sum(1)
    out = (w[..., None] * rgb).sum(-2)
    if white_bg:
        out = out + 1 - acc[:, None]
    return out, (w * z).sum(-1), acc, w


def clear_of_dust(raw, noise, scale, dust):
    """Nudge raw densities whose activated value lies within 1e-3 (relative) of the dust threshold: fp32 and fp64 must
    not disagree on which side of it a sample is."""
    s = torch.nn.functional.softplus(raw.double() + noise.double() * scale)
    near = ((s - dust).abs() <= 1e-3 * dust)
    raw = raw.clone()
    raw[near] += 0.05
    return raw


def check_median(med_depth, med_points, w64, z, warped, what):
    """The median index exactly: the kernel's median depth / point is z / warped[..., 0] at the oracle's index (0
    where the threshold is never reached), except on rays whose fp64 inclusive sum passes within 1e-5 of 0.5."""
    cs = torch.cumsum(w64, -1)
    ambiguous = ((cs - 0.5).abs() <= 1e-5).any(-1)
    mask, idx = O.median_depth_index(w64)
    found = mask.any(-1)
    zr = torch.where(found, torch.gather(z, 1, idx[:, None])[:, 0], torch.zeros(()))
    ok = ~ambiguous
    _record(what + " median: ambiguous rays", "count", int(ambiguous.sum()), 2)
    assert int(ambiguous.sum()) <= 2, f"{what}: {int(ambiguous.sum())} rays with a median sum within 1e-5 of 0.5"
    assert torch.equal(med_depth.cpu()[ok], zr[ok]), what + " median depth (index)"
    if med_points is not None:
        pr = torch.gather(warped[..., 0], 1, idx[:, None])[:, 0]
        assert torch.equal(med_points.cpu()[ok], pr[ok]), what + " median points (index)"


COMP_CFGS = {   # variant, white_bg, sample_at_infinity, noise_scale (None: no noise), dust threshold, keep
    "v0_inf_noise_dust_keep": (0, False, True, 0.7, 0.05, True),
    "v0_noinf_white": (0, True, False, None, None, False),
    "v1_white_noise": (1, True, True, 1.0, None, False),
    "v1_black": (1, False, True, None, None, True),
}


@pytest.mark.parametrize("cfg", sorted(COMP_CFGS))
@pytest.mark.parametrize("s", COMP_S)
def test_composite_long_rays_vs_fp64_oracle(s, cfg):
    """hn_composite_forward / _backward at 63 .. 512 samples against the float64 oracle: forward 2e-5 of the tensor's
    scale, d rgb 5e-5, d raw 2e-4 (as test_per_ray_kernels_random_sizes_fuzz), median index exact."""
    variant, wb, sai, ns, dust, use_keep = COMP_CFGS[cfg]
    seed = 4000 + s
    o, d, rgb, raw, z, noise, warped, keep = comp_inputs(s, seed)
    if dust is not None:
        raw = clear_of_dust(raw, noise if ns else torch.zeros_like(raw), ns or 0.0, dust)
    keep = keep if use_keep else None
    what = f"composite S={s} {cfg}"
    rgb64, raw64 = rgb.double().requires_grad_(True), raw.double().requires_grad_(True)
    refs = ref_composite(rgb64, raw64, z.double(), d.double(), variant, wb, sai,
                         noise.double() if ns else None, ns or 0.0, dust, keep.double() if keep is not None else None)
    rgb_g, raw_g = rgb.to(DEV).requires_grad_(True), raw.to(DEV).requires_grad_(True)
    outs = F.composite(rgb_g, raw_g, noise.to(DEV) if ns else None, z.to(DEV), d.to(DEV),
                       warped.to(DEV) if variant == 0 else None, variant=variant, white_bg=wb, sample_at_infinity=sai,
                       want_median=(variant == 0), dust_threshold=dust, keep=keep.to(DEV) if keep is not None else None,
                       noise_scale=ns or 1.0)
    for i, name in enumerate(["rgb", "depth", "acc", "weights"]):
        assert_close(outs[i], refs[i], 2e-5, f"{what} {name}")
    if variant == 0:
        check_median(outs[4], outs[5], refs[3].detach(), z, warped, what)
    gr = [H.uniform(seed, f"g{i}", tuple(refs[i].shape), -1, 1) for i in range(4)]
    sum((r * g.double()).sum() for r, g in zip(refs, gr)).backward()
    sum((outs[i] * gr[i].to(DEV)).sum() for i in range(4)).backward()
    assert_grad_close(rgb_g.grad, rgb64.grad, 5e-5, what + " d rgb")
    assert_grad_close(raw_g.grad, raw64.grad, 2e-4, what + " d raw")


@pytest.mark.parametrize("s,nc", [(257, 129), (257, 64), (512, 257), (512, 64)])
def test_composite_two_parts_long_rays_vs_fp64_oracle(s, nc):
    """A level in two parts (perm, split) at 257 and 512 samples against the float64 oracle of the level in sorted
    order: forward, median, sorted warped rows and the gradients scattered back to the parts."""
    seed = 4600 + s + nc
    o, d, rgb, raw, z_unused, noise, warped, keep = comp_inputs(s, seed)
    b = raw.shape[0]
    z_old, _ = torch.sort(H.uniform(seed, "zo", (b, nc), 0, 1), dim=-1)
    z_new = H.uniform(seed, "zn", (b, s - nc), 0, 1)
    z_all, perm = torch.sort(torch.cat([z_old, z_new], 1), dim=1, stable=True)
    g = lambda t, p: torch.gather(t, 1, p if t.dim() == 2 else p[..., None].expand(-1, -1, t.shape[-1]))
    # rgb / raw / warped are given in cat(z_old, z_new) order; the oracle sees them in sorted order
    rgb_s, raw_s, warped_s = g(rgb, perm), g(raw, perm), g(warped, perm)
    raw_s = clear_of_dust(raw_s, noise, 0.7, 0.05)
    raw = torch.zeros_like(raw).scatter_(1, perm, raw_s)
    what = f"composite two parts S={s} nc={nc}"
    rgb64, raw64 = rgb_s.double().requires_grad_(True), raw_s.double().requires_grad_(True)
    refs = ref_composite(rgb64, raw64, z_all.double(), d.double(), 0, False, True, noise.double(), 0.7, 0.05,
                         keep.double())
    parts = [t.contiguous().to(DEV).requires_grad_(True) for t in (rgb[:, :nc], raw[:, :nc], rgb[:, nc:], raw[:, nc:])]
    two = F.composite(parts[0], parts[1], noise.to(DEV), z_all.to(DEV), d.to(DEV), warped[:, :nc].contiguous().to(DEV),
                      variant=0, sample_at_infinity=True, want_median=True, dust_threshold=0.05, keep=keep.to(DEV),
                      noise_scale=0.7, rgb1=parts[2], raw1=parts[3], warped1=warped[:, nc:].contiguous().to(DEV),
                      perm=perm.int().to(DEV))
    for i, name in enumerate(["rgb", "depth", "acc", "weights"]):
        assert_close(two[i], refs[i], 2e-5, f"{what} {name}")
    check_median(two[4], two[5], refs[3].detach(), z_all, warped_s, what)
    assert torch.equal(two[6].cpu(), warped_s), what + " sorted warped rows"
    gr = [H.uniform(seed, f"g{i}", tuple(refs[i].shape), -1, 1) for i in range(4)]
    sum((r * q.double()).sum() for r, q in zip(refs, gr)).backward()
    sum((two[i] * gr[i].to(DEV)).sum() for i in range(4)).backward()
    d_rgb = torch.zeros(b, s, 3, dtype=torch.float64).scatter_(1, perm[..., None].expand(-1, -1, 3), rgb64.grad)
    d_raw = torch.zeros(b, s, dtype=torch.float64).scatter_(1, perm, raw64.grad)
    assert_grad_close(torch.cat([parts[0].grad, parts[2].grad], 1), d_rgb, 5e-5, what + " d rgb")
    assert_grad_close(torch.cat([parts[1].grad, parts[3].grad], 1), d_raw, 2e-4, what + " d raw")


@pytest.mark.parametrize("s", [256, 257, 384, 512])
def test_golden_g19_compositing(golden_dir, s):
    """model_utils.volumetric_rendering / compute_depth_index against the reference's own outputs at 256 .. 512
    samples (g19), every combination of sample_at_infinity and white background."""
    g = g19(golden_dir)
    pre = f"comp/S{s}/"
    T = lambda k: torch.from_numpy(g[pre + k]).to(DEV)
    for inf in (True, False):
        for wb in (True, False):
            tag = f"inf{int(inf)}_wb{int(wb)}/"
            r = MU.volumetric_rendering(T("rgb"), T("sigma"), T("z"), T("d"), wb, sample_at_infinity=inf)
            for k in ("rgb", "depth", "acc", "weights", "med_depth"):
                assert_close(r[k], torch.from_numpy(g[pre + tag + k]), 2e-5, f"g19 S={s} {tag}{k}")
            di = MU.compute_depth_index(r["weights"])
            assert np.array_equal(di.cpu().numpy(), g[pre + tag + "dindex"]), f"g19 S={s} {tag}median index"


# ---- inverse-CDF sampler ------------------------------------------------------------------------------------------
def pdf_inputs(b, nc, nf, seed, nb=None):
    o, d, _ = rays_for(seed, b)
    z, _ = torch.sort(H.uniform(seed, "z", (b, nc), 0, 1), dim=-1)
    w = H.uniform(seed, "w", (b, nb if nb is not None else nc), 0, 1) ** 3
    w[0] = 0.0                                             # all-zero weights
    w[1] = 0.0
    w[1, w.shape[1] // 2] = 1.0                            # one-hot
    u = H.uniform(seed, "u", (b, nf), 0, 1)
    if nf > 3:
        u[2, 3] = u[2, 1]                                  # two equal new samples
    return o, d, z, w, u


def check_merge(z_all, perm, pts, z, zs, o, d, what):
    """z_all == sort(cat(z, z_samples)) and perm == its stable argsort, bit for bit; the points of the sorted depths."""
    ref, ref_perm = torch.sort(torch.cat([z, zs.cpu()], 1), dim=1, stable=True)
    bad = int((z_all.cpu() != ref).sum())
    assert bad == 0, f"{what}: {bad} merged depths differ from sort(cat(z, z_samples))"
    if perm is not None:
        bad = int((perm.cpu().long() != ref_perm).sum())
        assert bad == 0, f"{what}: {bad} perm entries differ from the stable argsort"
    assert torch.equal(pts.cpu(), o[:, None, :] + ref[..., None] * d[:, None, :]), what + ": points"


def run_sampler(w, z, u, o, d, bins, what):
    """hn_sample_pdf and hn_sample_pdf_split on the same input: identical shared outputs, returned with perm."""
    T = lambda t: t.to(DEV) if t is not None else None
    a = F.sample_pdf(T(w), T(z), T(u), T(o), T(d), bins=T(bins))
    s = F.sample_pdf(T(w), T(z), T(u), T(o), T(d), bins=T(bins), split=True)
    for x, y, name in zip(a, s[:4], ["z_all", "pts", "inds", "z_samples"]):
        assert torch.equal(x, y), f"{what}: hn_sample_pdf {name} != hn_sample_pdf_split"
    assert torch.equal(s[5].cpu(), o[:, None, :] + s[3].cpu()[..., None] * d[:, None, :]), what + ": new points"
    return s


FUSED = sorted({(nc, nf) for nc in (3, 64, 255, 256, 257) for nf in (1, 64, 255, 512 - nc)})


@pytest.mark.parametrize("nc,nf", FUSED)
def test_sample_pdf_fused_form_bitexact_up_to_512(nc, nf):
    """The fused form (bins = midpoints of z, weights = columns 1 .. nc-2) against O.sample_pdf /
    O.piecewise_constant_pdf: indices, samples, merged depths and points bit for bit, perm = the stable argsort.
    nc = 257 is past the rank merge's 256 coarse depths."""
    b = 9
    o, d, z, w, u = pdf_inputs(b, nc, nf, 4100 + nc + nf)
    what = f"fused nc={nc} nf={nf}"
    mid = 0.5 * (z[:, 1:] + z[:, :-1])
    z_ref, p_ref, inds_ref = O.sample_pdf(mid, w[:, 1:-1], o, d, z, u)
    zs_ref, _ = O.piecewise_constant_pdf(mid, w[:, 1:-1], u)
    z_all, pts, inds, zs, perm, _ = run_sampler(w, z, u, o, d, None, what)
    assert torch.equal(inds.cpu(), inds_ref), what + ": indices"
    assert torch.equal(zs.cpu(), zs_ref), what + ": samples"
    assert torch.equal(z_all.cpu(), z_ref), what + ": merged depths"
    assert torch.equal(pts.cpu(), p_ref), what + ": points"
    check_merge(z_all, perm, pts, z, zs, o, d, what)


@pytest.mark.parametrize("nb", [254, 255])
@pytest.mark.parametrize("nc", [257, 300, 448])
@pytest.mark.parametrize("order", ["sorted", "swapped"])
def test_sample_pdf_bins_form_merges_more_than_256_depths(nb, nc, order):
    """The bins form with nb = 254 / 255 bins and nc = 257 .. 448 depths to merge, nf = 512 - nc: sorted depths (the
    rank merge's predicate holds, but it ranks only 256 of them) and two depths swapped (the bitonic sort) — both the
    stable sort of cat(z, z_samples) with its permutation, indices and samples bit-exact against the oracle."""
    b, nf = 7, 512 - nc
    seed = 4300 + nb + nc
    o, d, z, w, u = pdf_inputs(b, nc, nf, seed, nb=nb)
    bins, _ = torch.sort(H.uniform(seed, "bins", (b, nb + 1), 0, 1), dim=-1)
    if order == "swapped":
        z[:, [10, nc - 5]] = z[:, [nc - 5, 10]]
    what = f"bins nb={nb} nc={nc} ({order})"
    zs_ref, inds_ref = O.piecewise_constant_pdf(bins, w, u)
    z_ref, p_ref, _ = O.sample_pdf(bins, w, o, d, z, u)
    z_all, pts, inds, zs, perm, _ = run_sampler(w, z, u, o, d, bins, what)
    assert torch.equal(inds.cpu(), inds_ref), what + ": indices"
    assert torch.equal(zs.cpu(), zs_ref), what + ": samples"
    check_merge(z_all, perm, pts, z, zs, o, d, what)
    assert torch.equal(z_all.cpu(), z_ref) and torch.equal(pts.cpu(), p_ref), what + ": vs O.sample_pdf"


@pytest.mark.parametrize("s", [255, 256, 257])
def test_composite_then_pdf_long_rays_equals_the_two_launches(s):
    """hn_composite_sample_pdf at S = 255 .. 257 coarse samples and 512 - S fine ones: bit-equal to hn_composite_forward
    followed by hn_sample_pdf[_split], with and without the split outputs."""
    b, nf = 11, 512 - s
    seed = 4500 + s
    o, d, rgb, raw, z, noise, warped, _ = comp_inputs(s, seed)
    b = raw.shape[0]
    u = H.uniform(seed, "u", (b, nf), 0, 1)
    for split in (False, True):
        sep = F.composite(rgb.to(DEV), raw.to(DEV), noise.to(DEV), z.to(DEV), d.to(DEV), warped.to(DEV), noise_scale=0.5)
        pdf = F.sample_pdf(sep[3], z.to(DEV), u.to(DEV), o.to(DEV), d.to(DEV), split=split)
        fused = F.composite(rgb.to(DEV), raw.to(DEV), noise.to(DEV), z.to(DEV), d.to(DEV), warped.to(DEV), noise_scale=0.5,
                            then_pdf=dict(u=u.to(DEV), origins=o.to(DEV), directions=d.to(DEV), split=split))
        assert len(fused) == len(sep) + len(pdf)
        for i, (x, y) in enumerate(zip(sep + pdf, fused)):
            assert torch.equal(x, y), f"S={s} split={split}: output {i}"
        if split:
            check_merge(pdf[0], pdf[4], pdf[1], z, pdf[3], o, d, f"composite+pdf S={s}")


def test_golden_g19_sampler(golden_dir):
    """The fused-form sampler on the reference's own inputs at nc = 256 / 257, nf = 512 - nc (g19): indices exactly as
    the reference (every u > 1e-5 from every cdf entry), everything bit-exact against the oracle; depths within 5e-5
    of the reference (its fp32 normaliser vs the fp64 one: see test_g19_long_rays_sampler)."""
    g = g19(golden_dir)
    for nc in (256, 257):
        pre = f"pdf/nc{nc}/"
        T = lambda k: torch.from_numpy(g[pre + k])
        z, w, u, o, d = T("z"), T("w"), T("u"), T("o"), T("d")
        z_all, pts, inds, zs, perm, _ = run_sampler(w, z, u, o, d, None, f"g19 nc={nc}")
        assert np.array_equal(inds.cpu().numpy(), g[pre + "inds"]), f"g19 nc={nc}: indices vs the reference"
        mid = 0.5 * (z[:, 1:] + z[:, :-1])
        z_ref, p_ref, _ = O.sample_pdf(mid, w[:, 1:-1], o, d, z, u)
        assert torch.equal(z_all.cpu(), z_ref) and torch.equal(pts.cpu(), p_ref), f"g19 nc={nc}: vs the oracle"
        check_merge(z_all, perm, pts, z, zs, o, d, f"g19 nc={nc}")
        for k, v in (("z_samples", zs), ("z_all", z_all), ("pts", pts)):
            err = float(np.abs(v.cpu().numpy() - g[pre + k]).max())
            _record(f"g19 nc={nc} {k} vs reference", "max abs", err, 5e-5)
            assert err <= 5e-5, (nc, k, err)


# ---- hn_depth_index -----------------------------------------------------------------------------------------------
def grid_weights(s, thr, seed):
    """Weights on a 2^-12 grid (every partial sum exact in any order): a ray crossing `thr` in each segment — the
    crossing exactly AT the threshold on every other one — one that never reaches it, one crossing at sample 0."""
    q = int(round(float(np.float32(thr)) * 4096))
    nseg = (s + 63) // 64
    rows = []
    rs = np.random.RandomState(seed)
    for k in range(nseg):
        c = min(s - 1, 64 * k + rs.randint(0, 64))
        w = np.zeros(s)
        w[:c] = rs.randint(0, 3, size=c)
        while w[:c].sum() >= q:
            w[rs.randint(0, c)] = 0
        w[c] = q - w[:c].sum() + (k % 2)                  # reaches thr exactly (k even) or one step past it
        w[c + 1:] = rs.randint(0, 4, size=s - c - 1)
        rows.append(w)
    w = np.zeros(s); w[: s // 2] = 1; w[0] = 0            # never reaches thr
    while w.sum() >= q:
        w[np.nonzero(w)[0][-1]] = 0
    rows.append(w)
    w = np.zeros(s); w[0] = q; w[1:] = 1                  # at sample 0
    rows.append(w)
    return np.stack(rows) / 4096.0


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("s", [64, 65, 256, 257, 512])
def test_depth_index_bitexact_on_exact_sums(s, thr):
    """hn_depth_index through compute_depth_index / compute_depth_map / compute_opaqueness_mask against NumPy fp64:
    index, depth and mask bit for bit (weights on a 2^-12 grid make every partial sum exact in any order)."""
    w64 = grid_weights(s, thr, 4700 + s)
    b = w64.shape[0]
    z = np.sort(H.uniform(4700 + s, "z", (b, s), 0, 1).numpy(), axis=-1)
    cs = np.cumsum(w64, -1)
    reach = cs >= float(np.float32(thr))
    found = reach.any(-1)
    idx = np.where(found, reach.argmax(-1), 0)
    depth = np.where(found, z[np.arange(b), idx], 0.0).astype(np.float32)
    mask = np.zeros((b, s), np.float32)
    mask[np.arange(b)[found], idx[found]] = 1.0
    assert found[:-2].all() and not found[-2] and idx[-1] == 0
    wt = torch.from_numpy(w64.astype(np.float32)).to(DEV)
    zt = torch.from_numpy(z).to(DEV)
    what = f"depth index S={s} thr={thr}"
    assert np.array_equal(MU.compute_depth_index(wt, thr).cpu().numpy(), idx), what + ": index"
    assert np.array_equal(MU.compute_depth_map(wt, zt, thr).cpu().numpy(), depth), what + ": depth"
    assert np.array_equal(MU.compute_opaqueness_mask(wt, thr).cpu().numpy(), mask), what + ": mask"


# ---- whole models -------------------------------------------------------------------------------------------------
MODEL_KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True)
_ORACLE = {}


def model_oracle(nc, nf):
    """The oracle's forward + gradients for a 6-ray bendy_cond model at nc + nf samples (computed once per size)."""
    if (nc, nf) not in _ORACLE:
        b, seed = 6, 4800 + nc
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **MODEL_KW)
        sd = load_hash(m, seed)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5,
               "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **MODEL_KW)
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        O.mse_loss(ref, gt).backward()
        _ORACLE[(nc, nf)] = (sd, o, d, idx, rng, gt, ref, {k: v.grad for k, v in p.items()})
    return _ORACLE[(nc, nf)]


@pytest.mark.parametrize("composite_pdf", [True, False], ids=["composite_pdf", "separate_pdf"])
@pytest.mark.parametrize("reuse", [True, False], ids=["reuse", "noreuse"])
@pytest.mark.parametrize("nc,nf", [(256, 256), (257, 255), (64, 448)])
def test_model_512_samples_vs_oracle(nc, nf, reuse, composite_pdf, monkeypatch):
    """NerfModel at 512 samples per ray in fp32 against O.nerf_model_forward at test_model_vs_oracle_larger's bounds,
    with the fine level re-using the coarse samples (the sampler's perm feeds its compositing) or not, and the fine
    samples drawn in the coarse compositing launch or by a launch of their own."""
    monkeypatch.setattr(models.NerfModel, "REUSE_COARSE", reuse)
    monkeypatch.setattr(F, "COMPOSITE_PDF", composite_pdf)
    HN.set_precision("fp32")
    sd, o, d, idx, rng, gt, ref, ref_grads = model_oracle(nc, nf)
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **MODEL_KW)
    m.load_state_dict(sd)
    m = m.to(DEV)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
    assert (m._reused_coarse is not None) == reuse, m._reused_coarse
    what = f"model {nc}+{nf} reuse={reuse} composite_pdf={composite_pdf}"
    for k in ("rgb", "depth", "acc", "weights", "warped_points"):
        assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"{what} coarse/{k}")
    same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
    _record(what + " fine indices agreeing", "fraction", same, 0.999)
    assert same > 0.999, f"only {same:.4f} of fine-sample indices agree"
    for k in ("rgb", "depth", "acc", "weights"):
        assert_close(out["fine"][k], ref["fine"][k], 1e-4, f"{what} fine/{k}")
    loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
    loss.backward()
    for k, prm in m.named_parameters():
        assert_grad_close(prm.grad, ref_grads[k], 5e-3, f"{what} d {k}")


def test_golden_g19_model(golden_dir):
    """The 257 + 255-sample bendy_cond model of g19 against the reference's own outputs, at test_golden_model_fp32's
    bounds: every fine-sample index, outputs 1e-4, loss, gradient summaries 5e-3."""
    HN.set_precision("fp32")
    z = g19(golden_dir)
    g = {k[len("model/"):]: z[k] for k in z.files if k.startswith("model/")}
    nc, nf, b, seed = int(g["nc"]), int(g["nf"]), int(g["b"]), int(g["seed"])
    m = models.NerfModel(EMB, near=0.0, far=1.0, n_samples_coarse=nc, n_samples_fine=nf, noise_std=None,
                         view_fourier_dim=6, **MODEL_KW)
    assert sorted(m.state_dict().keys()) == g["keys"].tolist()
    load_hash(m, seed)
    m = m.to(DEV)
    o, d, idx = rays_for(seed, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng_from_fixture(g).items()})
    flips = int((m.last_sampling["inds"].cpu().numpy() != g["fine/inds"]).sum())
    assert flips == 0, f"{flips} fine-sample indices differ from the reference"
    for lvl in ("coarse", "fine"):
        for k in ("points", "warped_points", "rgb", "depth", "med_depth", "acc", "weights", "med_points"):
            assert_close(out[lvl][k], torch.from_numpy(g[f"{lvl}/{k}"]), 1e-4, f"g19 model {lvl}/{k}")
    gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0).to(DEV)
    loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4 * max(1.0, float(g["loss"]))
    loss.backward()
    grad_stats_close({k: v.grad for k, v in m.named_parameters()}, g, "grad/", 5e-3)


def test_legacy_render_rays_257_plus_255_vs_oracle():
    """nerf_pl render_rays at N_samples = 257, N_importance = 255 (the fused-form sampler merging 257 coarse depths)
    against O.legacy_render_rays in fp32: outputs 1e-4, fine-sample indices."""
    HN.set_precision("fp32")
    b, n, ni, seed = 6, 257, 255, 4900
    coarse, fine = legacy_nerf.NeRF(), legacy_nerf.NeRF()
    sc, sf = load_hash(coarse, seed), load_hash(fine, seed + 1)
    o, d, _ = rays_for(seed, b)
    rays = torch.cat([o, d, torch.full((b, 1), 0.2), torch.full((b, 1), 1.5)], 1)
    rng = {"perturb_rand": H.uniform(seed, "t", (b, n), 0, 1), "noise_coarse": H.normal(seed, "n1", (b, n)),
           "u": H.uniform(seed, "u", (b, ni), 0, 1), "noise_fine": H.normal(seed, "n2", (b, n + ni))}
    kw = dict(N_samples=n, N_importance=ni, perturb=1, noise_std=0.5)
    ref = O.legacy_render_rays([sc, sf], (10, 4), rays, rng, **kw)
    emb = [legacy_nerf.Embedding(3, 10), legacy_nerf.Embedding(3, 4)]
    res = legacy_rendering.render_rays([coarse.to(DEV), fine.to(DEV)], emb, rays.to(DEV),
                                       rng={k: v.to(DEV) for k, v in rng.items()}, **kw)
    for k in ("rgb_coarse", "depth_coarse", "opacity_coarse"):
        assert_close(res[k], ref[k], 1e-4, f"legacy 257+255 {k}")
    same = (legacy_rendering.render_rays.last_sampling["inds"].cpu() == ref["_inds"]).float().mean().item()
    _record("legacy 257+255 fine indices agreeing", "fraction", same, 0.999)
    assert same > 0.999, f"only {same:.4f} of fine-sample indices agree"
    for k in ("rgb_fine", "depth_fine", "opacity_fine"):
        assert_close(res[k], ref[k], 1e-4, f"legacy 257+255 {k}")


# ---- refusal ------------------------------------------------------------------------------------------------------
def test_sizes_past_the_limits_raise_before_any_launch():
    """F.composite at 513 samples, F.sample_pdf with 256 bins and composite(then_pdf=...) at 258 coarse samples raise
    HnError (status -2 from the entry point's check): nothing is launched, the stream stays clean."""
    b = 3
    o, d, _ = rays_for(1, b)
    for s in (513,):
        z, _ = torch.sort(torch.rand(b, s), dim=-1)
        with pytest.raises(L.HnError):
            F.composite(torch.rand(b, s, 3, device=DEV), torch.rand(b, s, device=DEV), None, z.to(DEV), d.to(DEV))
    z, _ = torch.sort(torch.rand(b, 300), dim=-1)
    bins, _ = torch.sort(torch.rand(b, 257), dim=-1)
    with pytest.raises(L.HnError):
        F.sample_pdf(torch.rand(b, 256, device=DEV), z.to(DEV), torch.rand(b, 8, device=DEV), o.to(DEV), d.to(DEV),
                     bins=bins.to(DEV))
    s = 258
    z, _ = torch.sort(torch.rand(b, s), dim=-1)
    with pytest.raises(L.HnError):
        F.composite(torch.rand(b, s, 3, device=DEV), torch.rand(b, s, device=DEV), None, z.to(DEV), d.to(DEV),
                    then_pdf=dict(u=torch.rand(b, 8, device=DEV), origins=o.to(DEV), directions=d.to(DEV)))
    torch.cuda.synchronize()
