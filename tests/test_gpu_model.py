"""GPU parity tests (MI355X): the fused MLP machine and the full render path against the CPU oracle and the
committed golden fixtures (outputs of the reference itself).

Tolerances (measured worst cases of a GPU run: profiles/r02_parity_errors.json, summarised in DESIGN.md §4).
fp32 mode (v_mfma_f32_32x32x2_f32, exact fp32 products): the north-star's 1e-4, ELEMENT-wise relative with an absolute
floor for near-zero elements (gpu_common.assert_close); every forward tensor of every fixture measures <= 2.5e-5 on
that scale, so there are no per-tensor exceptions.  Gradients: max error <= 5e-3 of the tensor's largest entry
(measured <= 3.1e-3; the worst are layers fed by sin(2^9 x) features, where two fp32 summation orders of the same sum
differ).  bf16 mode (bf16 operands, fp32 accumulate): forward 1e-2 (measured <= 4.2e-3), gradients as relative L2 of
the tensor <= 0.25 on these 40-1000-point batches (measured <= 0.18: a ReLU that flips under bf16 rounding moves one
summand of a small-batch gradient by O(1)).  The tight statement for bf16 mode is
test_bf16_mode_vs_bf16_operand_oracle (oracle under the same arithmetic contract: forward 1e-3, gradients 8e-2);
its acceptance criterion is PSNR (tools/psnr_parity.py)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
from gpu_common import oracle_threads, DEV, EMB, assert_close, assert_grad_close, load_hash, rays_for
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import models, modules, warping
from hypernerf_torch_amd.models import nerf as legacy_nerf
from hypernerf_torch_amd.models import rendering as legacy_rendering
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16": 1e-2}
GTOL = {"fp32": 2e-3, "bf16": 2.5e-1}


@pytest.fixture(params=["fp32", "bf16"])
def precision(request):
    old = HN.get_precision()
    HN.set_precision(request.param)
    yield request.param
    HN.set_precision(old)


def test_mlp_standalone(precision):
    m = modules.MLP(in_ch=20, out_ch=3, depth=6, width=128)
    sd = load_hash(m, 3)
    x = H.uniform(3, "x", (7, 9, 20), -1, 1)
    y_ref = O.mlp({"m." + k: v.clone().requires_grad_(True) for k, v in sd.items()}, "m", x, depth=6)
    m = m.to(DEV)
    y = m(x.to(DEV))
    assert_close(y, y_ref, TOL[precision], "MLP forward", elementwise=precision == "fp32")


def test_mlp_random_shapes_fuzz():
    """modules.MLP on 40 seeded random configurations (input width 1..190, hidden width 8..256 incl. widths that are
    no multiple of 32, depth 0..8, random skip layers, 1..40 outputs incl. the wide-output path, 1..700 points, output
    activations) in fp32 mode against the oracle's MLP: forward 1e-4 element-wise, input and weight gradients 5e-3.
    A configuration the machine does not implement must say so (NotImplementedError), not mis-compute."""
    HN.set_precision("fp32")
    rs = np.random.RandomState(1234)
    done = refused = 0
    why = []
    try:
        for case in range(40):
            in_ch = int(rs.choice([1, 3, 7, 20, 33, 64, 71, 115, 167, 190]))
            width = int(rs.choice([8, 24, 32, 53, 64, 96, 128, 160, 200, 256]))
            depth = int(rs.randint(0, 9))
            out_ch = int(rs.choice([1, 2, 3, 4, 5, 8, 17, 32, 40]))
            n_hidden = max(depth, 1)
            skips = sorted(set(int(v) for v in rs.randint(0, max(1, n_hidden - 1), size=rs.randint(0, 3)))) if n_hidden > 1 else []
            if rs.rand() < 0.1:
                skips = sorted(set(skips + [n_hidden - 1]))          # the reference shape-errors on this one
            out_act = [None, torch.nn.ReLU(), torch.nn.Sigmoid()][int(rs.randint(0, 3))]
            n = int(rs.choice([1, 5, 31, 32, 33, 100, 257, 700]))
            what = f"fuzz {case}: in {in_ch} width {width} depth {depth} out {out_ch} skips {skips} act {type(out_act).__name__} n {n}"
            try:
                m = modules.MLP(in_ch=in_ch, out_ch=out_ch, depth=depth, width=width, skips=skips, output_activation=out_act)
                sd = load_hash(m, 300 + case)
                m = m.to(DEV)
                x = H.uniform(300 + case, "x", (n, in_ch), -1, 1)
                want_dx = in_ch <= 24          # the machine differentiates w.r.t. <= 32 source components
                xg = x.to(DEV).requires_grad_(want_dx)
                y = m(xg)
            except NotImplementedError as e:
                refused += 1
                why.append(what + " -> " + str(e)[:90])
                continue
            except RuntimeError:
                y = None         # must be a configuration the reference fails on as well (checked below)
            tp = {"m." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
            xr = x.clone().requires_grad_(True)
            okw = dict(depth=depth, skips=tuple(skips),
                       out_act={"NoneType": "none", "ReLU": "relu", "Sigmoid": "sigmoid"}[type(out_act).__name__])
            if y is None:
                with pytest.raises(RuntimeError):
                    O.mlp(tp, "m", xr, **okw)
                refused += 1
                continue
            y_ref = O.mlp(tp, "m", xr, **okw)
            assert_close(y, y_ref, 1e-4, what + " forward")
            g = H.uniform(300 + case, "g", tuple(y_ref.shape), -1, 1)
            (y_ref * g).sum().backward()
            (y * g.to(DEV)).sum().backward()
            if want_dx:
                assert_grad_close(xg.grad, xr.grad, 5e-3, what + " d x")
            for k, prm in m.named_parameters():
                assert_grad_close(prm.grad, tp["m." + k].grad, 5e-3, what + " d " + k)
            done += 1
    finally:
        HN.set_precision("bf16")
    assert done >= 24, (done, refused, why)       # the rest: explicit refusals (wide sigmoid outputs, ...)


@pytest.mark.parametrize("n", [64, 100, 1000])
def test_translation_field(precision, n):
    tf = warping.TranslationField(in_ch=3, in_ch_embed=8)
    sd = load_hash(tf, 5)
    b, s = n // 4 if n % 4 == 0 else n, 4 if n % 4 == 0 else 1
    pts = H.uniform(5, "pts", (b, s, 3), -1.2, 1.2)
    emb = H.uniform(5, "emb", (b, 8), -0.5, 0.5)
    tp = {"w." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    er = emb.clone().requires_grad_(True)
    y_ref = O.translation_field(tp, "w", pts, er[:, None, :].expand(b, s, 8))
    tf = tf.to(DEV)
    eg = emb.to(DEV).requires_grad_(True)
    y = tf.warp(pts.to(DEV), eg, None)
    assert_close(y, y_ref, TOL[precision], "warp forward", elementwise=precision == "fp32")
    g = H.uniform(6, "g", (b, s, 3), -1, 1)
    (y_ref * g).sum().backward()
    (y * g.to(DEV)).sum().backward()
    fro = precision == "bf16"
    assert_grad_close(eg.grad, er.grad, GTOL[precision], "d embed", frobenius=fro)
    for k, prm in tf.named_parameters():
        assert_grad_close(prm.grad, tp["w." + k].grad, GTOL[precision], "d " + k, frobenius=fro)


def test_hyper_sheet_and_broadcast_embed(precision):
    hs = modules.HyperSheetMLP(out_ch=4, in_ch_embed=8)
    sd = load_hash(hs, 6)
    b, s = 6, 16
    pts = H.uniform(5, "pts", (b, s, 3), -1.2, 1.2)
    emb = H.uniform(5, "emb", (b, 8), -0.5, 0.5)
    y_ref = O.hyper_sheet({"h." + k: v for k, v in sd.items()}, "h", pts, emb[:, None, :].expand(b, s, 8))
    hs = hs.to(DEV)
    y1 = hs(pts.to(DEV), emb.to(DEV))                                   # per-ray embedding
    y2 = hs(pts.to(DEV), emb.to(DEV)[:, None, :].expand(b, s, 8))       # the reference's broadcast form
    assert_close(y1, y_ref, TOL[precision], "sheet (per-ray)", elementwise=precision == "fp32")
    assert_close(y2, y_ref, TOL[precision], "sheet (broadcast)", elementwise=precision == "fp32")


def test_golden_fields(golden_dir, precision):
    g = np.load(os.path.join(golden_dir, "g05_fields.npz"))
    pts, emb = torch.from_numpy(g["pts"]).to(DEV), torch.from_numpy(g["emb"]).to(DEV)
    tf = warping.TranslationField(in_ch=3, in_ch_embed=8); load_hash(tf, 5)
    hs = modules.HyperSheetMLP(out_ch=4, in_ch_embed=8); load_hash(hs, 6)
    assert_close(tf.to(DEV)(pts, emb, None)["warped_points"], torch.from_numpy(g["y_warp"]), TOL[precision], "G5", elementwise=precision == "fp32")
    assert_close(hs.to(DEV)(pts, emb), torch.from_numpy(g["y_sheet"]), TOL[precision], "G6", elementwise=precision == "fp32")


def test_golden_nerfmlp(golden_dir, precision):
    g = np.load(os.path.join(golden_dir, "g07_nerfmlp.npz"))
    for tag, acd in (("cond", 8), ("nocond", 0)):
        nm = modules.NerfMLP(in_ch=115, trunk_depth=8, trunk_width=256, rgb_branch_depth=4, rgb_branch_width=128,
                             hidden_activation=torch.nn.ReLU(), skips=[4], rgb_activation=torch.nn.Sigmoid(),
                             alpha_condition_dim=acd, rgb_condition_dim=39)
        load_hash(nm, 7)
        nm = nm.to(DEV)
        ac = torch.from_numpy(g["ac"]).to(DEV) if acd else None
        y = nm(torch.from_numpy(g["x"]).to(DEV), alpha_condition=ac, rgb_condition=torch.from_numpy(g["rc"]).to(DEV))
        assert_close(y["rgb"], torch.from_numpy(g["rgb_" + tag]), TOL[precision], "G7 rgb " + tag, elementwise=precision == "fp32")
        assert_close(y["alpha"], torch.from_numpy(g["alpha_" + tag]), TOL[precision], "G7 alpha " + tag, elementwise=precision == "fp32")


CASES = {
    "bendy": dict(hyper_slice_method="bendy_sheet", use_nerf_embed=False, use_alpha_cond=False),
    "bendy_cond": dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True),
    "bendy_rgbcond": dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True,
                          use_rgb_cond=True),
    "nowarp": dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=False, use_alpha_cond=False),
    "nowarp_cond": dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=True, use_alpha_cond=True),
    "warp_noslice": dict(use_warp=True, hyper_slice_method=None, use_nerf_embed=False, use_alpha_cond=False,
                         hyper_slice_out_dim=0),
    "axis": dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=False,
                 use_alpha_cond=False),
}


def fixtures(golden_dir):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "g11_model_*.npz")))


def rng_from_fixture(g):
    kinds = g["draw_kinds"].tolist()
    draws = [torch.from_numpy(g[f"draw{i}"]) for i in range(len(kinds))]
    rng, it = {}, iter(zip(kinds, draws))
    k, t = next(it); rng["t_rand"] = t
    k, t = next(it)
    if k == "randn":
        rng["noise_coarse"] = t * float(g["noise_std"]); k, t = next(it)
    rng["u"] = t
    rest = list(it)
    if rest:
        rng["noise_fine"] = rest[0][1] * float(g["noise_std"])
    return rng


def grad_stats_close(named_grads, g, prefix, tol):
    """Compare with the reference's gradient summaries (sum / abs-sum / L2 + 16 sampled entries)."""
    for name, grad in named_grads.items():
        if prefix + name + "/none" in g:
            assert grad is None or float(grad.abs().sum()) == 0.0, name
            continue
        stats = g[prefix + name + "/stats"]
        gd = grad.detach().double().cpu().reshape(-1)
        mine = np.array([gd.sum().item(), gd.abs().sum().item(), gd.pow(2).sum().sqrt().item()])
        assert abs(mine[2] - stats[2]) <= tol * max(stats[2], 1e-12), (name, "L2", mine, stats)
        assert abs(mine[1] - stats[1]) <= tol * max(stats[1], 1e-12), (name, "abs-sum", mine, stats)
        idx = torch.from_numpy(g[prefix + name + "/idx"])
        ref = g[prefix + name + "/val"]
        assert float(np.abs(gd[idx].numpy() - ref).max()) <= tol * float(gd.abs().max()) + 1e-12, (name, "samples")


@pytest.mark.parametrize("fixture", fixtures(os.path.join(os.path.dirname(__file__), "golden")))
def test_golden_model_fp32(golden_dir, fixture):
    """Full NerfModel forward + loss + backward in fp32 mode vs the outputs of the reference itself."""
    HN.set_precision("fp32")
    g = np.load(os.path.join(golden_dir, fixture + ".npz"))
    case = [c for c in sorted(CASES, key=len, reverse=True) if fixture.startswith("g11_model_" + c + "_")][0]
    nc, nf, b, seed = int(g["nc"]), int(g["nf"]), int(g["b"]), int(g["seed"])
    m = models.NerfModel(EMB, near=0.0, far=1.0, n_samples_coarse=nc, n_samples_fine=nf,
                         noise_std=float(g["noise_std"]) or None, view_fourier_dim=6, **CASES[case])
    assert sorted(m.state_dict().keys()) == g["keys"].tolist()
    load_hash(m, seed)
    m = m.to(DEV)
    o, d, idx = rays_for(seed, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    rng = {k: v.to(DEV) for k, v in rng_from_fixture(g).items()}
    out = m(rays, {}, rng=rng)
    inds = m.last_sampling["inds"].cpu().numpy()
    flips = int((inds != g["fine/inds"]).sum())
    assert flips == 0, f"{flips} fine-sample indices differ from the reference (tie margin of the fixture is 1e-5)"
    for lvl in ("coarse", "fine"):
        for k in ("points", "warped_points", "rgb", "depth", "med_depth", "acc", "weights", "med_points"):
            assert_close(out[lvl][k], torch.from_numpy(g[f"{lvl}/{k}"]), 1e-4, f"{fixture} {lvl}/{k}")
    gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0).to(DEV)
    loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4 * max(1.0, float(g["loss"]))
    loss.backward()
    grad_stats_close({k: v.grad for k, v in m.named_parameters()}, g, "grad/", 5e-3)


@pytest.mark.parametrize("case", ["bendy_cond", "nowarp", "axis"])
def test_model_vs_oracle_larger(case, precision):
    """B=96 rays x (32+32): full tensors and full gradients against the oracle (same draws)."""
    kw = CASES[case]
    nc = nf = 32
    b, seed = 96, 77
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
    sd = load_hash(m, seed)
    m = m.to(DEV)
    o, d, idx = rays_for(seed, b)
    rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
           "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5, "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
    cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
    gt = H.uniform(seed, "gt", (b, 3), 0, 1)
    O.mse_loss(ref, gt).backward()
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
    tol = TOL[precision]
    for k in ("rgb", "depth", "acc", "weights", "warped_points"):
        assert_close(out["coarse"][k], ref["coarse"][k], tol, f"{case} coarse/{k}", elementwise=precision == "fp32")
    if precision == "fp32":
        same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.999, f"only {same:.4f} of fine-sample indices agree"
        for k in ("rgb", "depth", "acc", "weights"):
            assert_close(out["fine"][k], ref["fine"][k], 1e-4, f"{case} fine/{k}")
    loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
    loss.backward()
    # gradients.  fp32: every tensor to 5e-3 of its largest entry (the <=0.1 % of fine samples that land in a
    # neighbouring pdf bin and sin(2^9 x) features bound what two fp32 summation orders can agree on).
    # bf16: relative L2 error of the WHOLE gradient (<= 0.3: in bf16 mode the fine samples are drawn from bf16 coarse
    # weights, i.e. the fine level is evaluated at slightly different depths than the oracle), and per tensor where
    # the tensor carries >= 1 % of it.
    named = dict(m.named_parameters())
    if precision == "fp32":
        for k, prm in named.items():
            assert_grad_close(prm.grad, p[k].grad, 5e-3, f"{case} d {k}")
    else:
        ks = [k for k in named if p[k].grad is not None]
        ga = torch.cat([named[k].grad.detach().cpu().double().reshape(-1) for k in ks])
        ra = torch.cat([p[k].grad.double().reshape(-1) for k in ks])
        tot = float(ra.norm())
        assert float((ga - ra).norm()) <= 0.2 * tot, f"{case}: whole-gradient rel L2 {float((ga - ra).norm()) / tot:.3f}"
        # per tensor (round 5): against the fp32 oracle a bf16 gradient tensor is only good to ~0.2 — a bound that would
        # not notice a wrong small layer.  Every tensor that carries >= 0.1 % of the gradient is therefore compared with
        # the oracle under the SAME arithmetic contract (O.bf16_operands(): bf16 matmul operands, fp32 accumulate) at
        # 6e-2; the old 0.25 stays for the tail below that only (0.01 % .. 0.1 % of the gradient).
        pc = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        with O.bf16_operands():
            O.mse_loss(O.nerf_model_forward(pc, cfg, o, d, idx, rng), gt).backward()
        worst = 0.0
        for k in ks:
            if float(p[k].grad.norm()) >= 1e-3 * tot:
                assert_grad_close(named[k].grad, pc[k].grad, 6e-2, f"{case} d {k} (bf16 contract)", frobenius=True)
                worst = max(worst, float((named[k].grad.detach().cpu().double() - pc[k].grad.double()).norm()
                                         / (pc[k].grad.double().norm() + 1e-30)))
            elif float(p[k].grad.norm()) >= 1e-4 * tot:
                # the tail: sums of a few mixed-sign terms (single-element biases ...) whose relative error is large by
                # nature; below 0.01 % of the gradient a tensor is covered by the whole-gradient bound only
                assert_grad_close(named[k].grad, pc[k].grad, 0.25, f"{case} d {k} (tail, bf16 contract)", frobenius=True)
        print(f"{case}: worst per-tensor rel L2 vs the bf16-operand oracle (tensors >= 0.1 % of the gradient): {worst:.3e}")


@pytest.mark.parametrize("case,size", [("bendy_cond", (96, 32, 32)), ("axis", (96, 32, 32)), ("bendy_cond", (1024, 64, 64))],
                         ids=["bendy_cond", "axis", "bendy_cond_config2_full_size"])
def test_bf16_mode_vs_bf16_operand_oracle(case, size):
    """bf16 product mode against the oracle run under `O.bf16_operands()` — the same arithmetic contract (every
    Linear rounds its matmul operands to bf16, forward and backward, and accumulates in fp32; everything else fp32).
    What is left is summation order, the fast sin/cos of bf16 mode and the ReLUs / pdf bins that sit on a rounding
    boundary, so the bounds are ~10x tighter than against the fp32 oracle: forward 1e-3 of the tensor's scale
    (measured <= 2.6e-4), the whole gradient to a relative L2 of 2.5e-2 (measured 1.13e-2 / 9.9e-3 since the encoders
    take their sines on an exactly reduced argument — x / 2pi staged as hi + lo, hn_features4; 4.8e-2 / 4.2e-2 with the
    one-FMA argument of rounds 1-2, 1.6e-2 / 1.8e-2 with libm sines; against the fp32 oracle the same quantity is
    ~0.18), every gradient tensor that carries >= 1 % of it to 0.06.  Round 4: also once at config 2's FULL size
    (1024 rays x (64+64): the throughput mode itself, not only its fp32 sibling, against the oracle at the size the
    metric is quoted on)."""
    HN.set_precision("bf16")
    try:
        kw = CASES[case]
        b, nc, nf = size
        seed = 79
        torch.set_num_threads(oracle_threads(64))
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
        sd = load_hash(m, seed)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5,
               "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        with O.bf16_operands():
            ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
            O.mse_loss(ref, gt).backward()
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
        for k in ("rgb", "depth", "acc", "weights", "warped_points"):
            assert_close(out["coarse"][k], ref["coarse"][k], 1e-3, f"bf16-contract {case} coarse/{k}", elementwise=False)
        same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.99, f"only {same:.4f} of fine-sample indices agree"
        for k in ("rgb", "acc"):
            assert_close(out["fine"][k], ref["fine"][k], 1e-3, f"bf16-contract {case} fine/{k}", elementwise=False)
        loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
        ref_loss = float(O.mse_loss(ref, gt).detach())
        assert abs(float(loss.detach()) - ref_loss) <= 1e-3 * ref_loss
        loss.backward()
        named = dict(m.named_parameters())
        ks = [k for k in named if p[k].grad is not None]
        ga = torch.cat([named[k].grad.detach().cpu().double().reshape(-1) for k in ks])
        ra = torch.cat([p[k].grad.double().reshape(-1) for k in ks])
        tot = float(ra.norm())
        rel = float((ga - ra).norm()) / tot
        from gpu_common import _record
        _record(f"bf16-contract {case}: whole gradient", "rel L2", rel, 2.5e-2)
        per = {k: float((named[k].grad.detach().cpu().double() - p[k].grad.double()).norm() / (p[k].grad.double().norm() + 1e-30))
               for k in ks if float(p[k].grad.norm()) >= 1e-3 * tot}
        print(f"bf16-contract {case}: whole-gradient rel L2 {rel:.3e}; per tensor: " +
              ", ".join(f"{k.replace('.weight', '.w').replace('.bias', '.b')}={v:.3f}" for k, v in sorted(per.items())))
        assert rel <= 2.5e-2, f"{case}: whole-gradient rel L2 {rel:.3e} against the bf16-operand oracle"
        for k in ks:
            if float(p[k].grad.norm()) >= 1e-3 * tot:       # every tensor with >= 0.1 % of the gradient (round 5; 1 % before)
                assert_grad_close(named[k].grad, p[k].grad, 0.06, f"bf16-contract {case} d {k}", frobenius=True)
    finally:
        HN.set_precision("bf16")


def test_hi_only_staging_when_the_planes_do_not_fit_into_lds():
    """A program with 30 ENCODED source components: hi + lo planes of x / 2pi for all of them do not fit into LDS
    beside the weight ring, so the bf16 forward stages hi alone (HnMlpArgs.trig_lo_planes = 0, one shared zero plane).
    No model of the render path gets there (its encoders read <= 15 components); built directly on the machine and
    checked against torch under the bf16-operand contract, forward and gradients."""
    from hypernerf_torch_amd import functional as HF
    from hypernerf_torch_amd.machine import AuxSpec, GradIn, Layer, OutSpec, Program, posenc_features
    HN.set_precision("bf16")
    n, c = 777, 30
    x = H.uniform(23, "wide_x", (n, c), -1.0, 1.0)
    l0, l1 = torch.nn.Linear(c * 5, 64), torch.nn.Linear(64, 3)
    with torch.no_grad():
        for i, prm in enumerate(list(l0.parameters()) + list(l1.parameters())):
            prm.copy_(H.uniform(23, f"wide_p{i}", tuple(prm.shape), -0.3, 0.3))
    feats = posenc_features(0, range(c), 2, need_grad=False)
    layers = [Layer("l0", l0.weight, l0.bias, aux=AuxSpec(feats), act="relu"),
              Layer("l1", l1.weight, l1.bias, main=(0, 64), act="none", out=OutSpec(0, 0, "none"), grad_in=GradIn(4, 0))]
    l0.to(DEV), l1.to(DEV)
    call = HF.ProgramCall(Program(layers, n_src=1, name="wide_encoder"), [False], [3], [("g", 0)])
    assert call.program.n_trig_comps == c
    (y,) = HF.run_program(call, [x.to(DEV)], 1)
    g = H.normal(23, "wide_g", (n, 3))
    (y * g.to(DEV)).sum().backward()
    # reference: posenc_orig order [x, sin(1x), cos(1x), sin(2x), cos(2x)], every Linear with bf16-rounded operands
    r16 = lambda t: t.to(torch.bfloat16).float()
    w0, b0, w1, b1 = (t.detach().cpu().clone().requires_grad_(True) for t in (l0.weight, l0.bias, l1.weight, l1.bias))
    f = torch.cat([x, torch.sin(x), torch.cos(x), torch.sin(2 * x), torch.cos(2 * x)], -1)
    with O.bf16_operands():
        hcpu = torch.relu(O._linear({"a.weight": w0, "a.bias": b0}, "a", f))
        ref = O._linear({"b.weight": w1, "b.bias": b1}, "b", hcpu)
    (ref * g).sum().backward()
    assert_close(y, ref, 2e-3, "hi-only staging: forward", elementwise=False)
    for name, got, want in (("l0.weight", l0.weight.grad, w0.grad), ("l0.bias", l0.bias.grad, b0.grad),
                            ("l1.weight", l1.weight.grad, w1.grad), ("l1.bias", l1.bias.grad, b1.grad)):
        assert_grad_close(got, want, 3e-2, f"hi-only staging d {name}", frobenius=True)
    # and the launch really ran in the compact mode
    a = call.runner._args(call.runner._tables(torch.device(DEV), 1), 1, n, 1, False, call.runner._ops(torch.device(DEV), 1, n)[0],
                          len(call.program.fwd_ops), 0, 1, [(x.to(DEV), False)], [y.detach()], None, None, None)
    assert a.n_trig_comps == c and a.trig_lo_planes == 0
    HN.set_precision("bf16")


OPTION_CASES = {
    # call-time use_warp=False on a model built without a warp field (models.py:695, 723: `self.use_warp and use_warp`)
    "call_nowarp": (dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=True, use_alpha_cond=True), dict(use_warp=False)),
    # view directions given separately from the ray directions (models.py:717-720)
    "viewdirs": (dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True), dict(viewdirs=True)),
    # every size argument of the constructor off its default
    "dims": (dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, use_rgb_cond=True,
                  GLO_dim=4, xyz_fourier_dim=6, hyper_fourier_dim=3, view_fourier_dim=2, hyper_slice_out_dim=2), {}),
    # GLO_dim 24: 3 + 3 + 24 + 7 = 37 source components for the fused level program, 5 more than the LDS staging
    # holds, and surplus copies of a GATHERED table cannot be read directly -> per-network launches, not an error
    "glo24": (dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, GLO_dim=24), {}),
    # GLO_dim 25: 25 + the 8 reserved head rows exceed the 32 source-gradient rows of ONE fused program -> the level
    # falls back to per-network launches instead of raising
    "glo25": (dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, GLO_dim=25), {}),
    # near / far overridden per call (models.py:690-693)
    "near_far": (dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=False, use_alpha_cond=False),
                 dict(near=0.15, far=0.85)),
}


def test_call_time_nowarp_on_a_warp_model_shape_errors_like_the_reference():
    """A model built with use_warp=True sizes its template for 3 + hyper input channels (models.py:268); calling it
    with use_warp=False hands the template bare points (models.py:556-557) and the reference dies in the first
    Linear with a shape RuntimeError.  Same exception type here (raised by the program compiler), and the oracle."""
    kw = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True)
    nc = nf = 8
    b, seed = 8, 95
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, **kw)
    sd = load_hash(m, seed)
    m = m.to(DEV)
    o, d, idx = rays_for(seed, b)
    rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1)}
    with pytest.raises(RuntimeError):
        O.nerf_model_forward(dict(sd), O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, **kw), o, d, idx, rng,
                             use_warp=False)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    with pytest.raises(RuntimeError):
        m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()}, use_warp=False)


@pytest.mark.parametrize("case", sorted(OPTION_CASES))
def test_model_option_matrix_vs_oracle(case):
    """Constructor sizes and forward() keyword arguments the fixtures do not vary, fp32 against the oracle (1e-4
    element-wise on every returned per-ray tensor of both levels, gradients 1e-2), plus — for the default model —
    `metadata_encoded=True` fed with the gathered rows (per-network launches) against the index path (one fused
    launch per level): the same arithmetic per point, 1e-5."""
    HN.set_precision("fp32")
    try:
        kw, call = OPTION_CASES[case]
        nc, nf, b, seed = 16, 16, 40, 91
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.3, **kw)
        sd = load_hash(m, seed)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        vd = None
        if call.get("viewdirs"):
            vd = H.uniform(seed, "vd", (b, 3), -1, 1)
            vd = vd / vd.norm(dim=-1, keepdim=True)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.3, "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.3}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.3, near=call.get("near", 0.0),
                         far=call.get("far", 1.0), **kw)
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng, viewdirs=vd, use_warp=call.get("use_warp", True))
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        O.mse_loss(ref, gt).backward()
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None if vd is None else vd.to(DEV),
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        fkw = {k: call[k] for k in ("use_warp", "near", "far") if k in call}
        drng = {k: v.to(DEV) for k, v in rng.items()}
        out = m(rays, {}, rng=drng, **fkw)
        same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.995, f"only {same:.4f} of fine-sample indices agree"
        for lvl in ("coarse", "fine"):
            for k in ("rgb", "depth", "acc", "weights", "warped_points"):
                assert out[lvl][k].shape == ref[lvl][k].shape, (lvl, k)
                if lvl == "coarse" or same == 1.0:
                    assert_close(out[lvl][k], ref[lvl][k], 1e-4, f"options {case} {lvl}/{k}")
        loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
        loss.backward()
        for k, prm in m.named_parameters():
            # 1e-2 of the tensor's largest entry: measured worst 6.2e-3, the skip layer of the un-warped model, which
            # multiplies dZ with sin(2^9 x) features of raw points (two fp32 summation orders of ~1300 such terms)
            assert_grad_close(prm.grad, p[k].grad, 1e-2 if same == 1.0 else 2e-2, f"options {case} d {k}")
        if case == "glo24":
            # 37 source components for the fused level program, 5 more than the LDS staging holds, and the surplus
            # belongs to the GATHERED table, which the direct global read does not gather: per-network launches
            assert "fuse" in m._no_fit and not any(k[0] == "level" for k in m._template_calls)
        if case == "glo25":
            assert "fuse" in m._no_fit and not any(k[0] == "level" for k in m._template_calls)
        if case == "viewdirs":
            # the same forward with the embeddings looked up by the caller (metadata_encoded, models.py:609-622, 425-436)
            with torch.no_grad():
                row = m.warp_embed(idx.to(DEV))
                enc = dict(rays, metadata={"encoded_warp": row, "encoded_hyper": row, "encoded_nerf": row})
                out2 = m(enc, {}, rng=drng, metadata_encoded=True)
                out1 = m(rays, {}, rng=drng)
            for lvl in ("coarse", "fine"):
                for k in ("rgb", "depth", "acc"):
                    assert_close(out2[lvl][k], out1[lvl][k], 1e-5, f"metadata_encoded {lvl}/{k}")
    finally:
        HN.set_precision("bf16")


@pytest.mark.parametrize("case", ["bendy_cond", "axis", "nowarp_cond"])
def test_per_network_launch_path_matches_fused_level(case):
    """NerfModel.FUSE_LEVELS=False keeps the round-1 structure (one launch per network, torch glue in between; still
    used for pre-encoded metadata and hyper_point overrides).  Same model, same draws, fp32: outputs to 1e-5
    element-wise and every gradient to 1e-4 of the fused path's (same arithmetic per point; only the order in which
    float atomics land in the weight gradients differs)."""
    HN.set_precision("fp32")
    try:
        kw = CASES[case]
        nc, nf, b, seed = 32, 32, 24, 93
        rays_cpu = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5, "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
        gt = H.uniform(seed, "gt", (b, 3), 0, 1).to(DEV)
        res = {}
        for fuse in (True, False):
            m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, **kw)
            load_hash(m, seed)
            m = m.to(DEV)
            m.FUSE_LEVELS = fuse
            o, d, idx = rays_cpu
            rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                    "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
            L.KERNEL_TIMES = {}
            try:
                out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
                loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
                loss.backward()
                torch.cuda.synchronize()
                L.collect_kernel_times()
                launches = sorted(k for k, v in L.KERNEL_TIMES.items() if k.startswith("hn_mlp_forward") for _ in v)
            finally:
                L.KERNEL_TIMES = None
            res[fuse] = (out, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}, launches)
        # fused: one launch per level — the fine level as two when it re-uses the coarse samples' warp (REUSE_COARSE)
        assert len(res[True][2]) <= 3 and all("level" in k or "template" in k for k in res[True][2]), res[True][2]
        if case != "nowarp_cond":
            assert len(res[False][2]) > len(res[True][2]), (res[True][2], res[False][2])
        for lvl in ("coarse", "fine"):
            for k in ("rgb", "depth", "acc", "weights", "warped_points"):
                assert_close(res[False][0][lvl][k], res[True][0][lvl][k].cpu(), 1e-5, f"unfused {case} {lvl}/{k}")
        assert res[False][1].keys() == res[True][1].keys()
        for k, g in res[True][1].items():
            assert_grad_close(res[False][1][k], g, 1e-4, f"unfused {case} d {k}")
    finally:
        HN.set_precision("bf16")


@pytest.mark.parametrize("case", ["bendy", "bendy_cond", "bendy_rgbcond", "warp_noslice", "axis", "se3_axis", "se3_axis_cond",
                                  "se3_noslice"])
@pytest.mark.parametrize("sizes", [(32, 32, 24), (64, 128, 9), (8, 8, 16), (12, 20, 7)])
def test_fine_level_reusing_coarse_warp_matches_full_fine_level(case, sizes):
    """NerfModel.REUSE_COARSE: the fine level runs the fine template alone over the coarse level's warped points and the
    whole level program over the NEW samples only, composited through the merge permutation — against the reference's
    structure (every fine sample through warp field, hyper sheet and template: REUSE_COARSE = False) on the same model
    and draws, fp32.  Same function values: every returned tensor of both levels BIT-identical, fine sample indices
    included; gradients — the fine loss now reaches the shared networks through the coarse program's external
    `warped_points` gradient, so sums are taken in another order — to 1e-4 of the tensor's largest entry; also with a
    loss on `warped_points` itself, a bounding box and a dust threshold (filter_sigma) and a white background."""
    HN.set_precision("fp32")
    try:
        se3 = case.startswith("se3")
        kw = {"se3_axis": CASES["axis"], "se3_axis_cond": dict(CASES["axis"], use_nerf_embed=True, use_alpha_cond=True),
              "se3_noslice": CASES["warp_noslice"]}[case] if se3 else CASES[case]
        nc, nf, b = sizes
        seed = 97
        rays_cpu = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5, "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
        gt = H.uniform(seed, "gt", (b, 3), 0, 1).to(DEV)
        res = {}
        for reuse in (True, False):
            m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, **kw)
            if se3:         # BASELINE config 5: the warp field is its own program in front of a gathered template
                m.warp_field = warping.SE3Field(in_ch=3)
            load_hash(m, seed)
            m = m.to(DEV)
            m.REUSE_COARSE = reuse
            m.use_white_background = True
            o, d, idx = rays_cpu
            rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                    "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
            L.KERNEL_TIMES = {}
            try:
                out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()},
                        render_opts={"dust_threshold": 0.05, "bounding_box": (-0.9, 0.9, -0.9, 0.9, -0.9, 0.9)})
                gw = H.uniform(seed, "gw", tuple(out["fine"]["warped_points"].shape), -1, 1).to(DEV)
                loss = (((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
                        + 1e-3 * (out["fine"]["warped_points"] * gw).sum() + 0.1 * out["fine"]["depth"].mean())
                loss.backward()
                torch.cuda.synchronize()
                L.collect_kernel_times()
                launches = {k: len(v) for k, v in L.KERNEL_TIMES.items() if k.startswith("hn_mlp_forward")}
            finally:
                L.KERNEL_TIMES = None
            res[reuse] = (out, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                          launches, m.last_sampling["inds"].clone(), m.compiled_programs(b))
        if case == "se3_noslice":
            # no embedding reaches the template: the level runs through map_points / query_template network by network
            # and the fine level is not split (REUSE_COARSE covers the fused and the gathered-template levels)
            assert res[True][2] == res[False][2] and res[True][4][0][2] == res[False][4][0][2]
        elif se3:
            # field program: coarse + NEW samples only; the fine template still sees every fine sample, in two launches
            assert res[True][2] == {"hn_mlp_forward[SE3Field]": 2, "hn_mlp_forward[template_coarse]": 1,
                                    "hn_mlp_forward[template_fine]": 2}, res[True][2]
            assert res[False][2] == {"hn_mlp_forward[SE3Field]": 2, "hn_mlp_forward[template_coarse]": 1,
                                     "hn_mlp_forward[template_fine]": 1}, res[False][2]
            assert {n for name, _, n in res[True][4] if name == "warp_field"} == {b * (nc + nf)}
            assert {n for name, _, n in res[False][4] if name == "warp_field"} == {b * (2 * nc + nf)}
        else:
            assert sorted(res[True][2]) == ["hn_mlp_forward[level_coarse]", "hn_mlp_forward[level_fine]",
                                            "hn_mlp_forward[template_fine_reuse]"], res[True][2]
            assert sorted(res[False][2]) == ["hn_mlp_forward[level_coarse]", "hn_mlp_forward[level_fine]"], res[False][2]
            pts = {name: n for name, _, n in res[True][4]}
            assert pts == {"level_coarse": b * nc, "level_fine": b * nf, "level_fine_reuse": b * nc}, pts
            assert {name: n for name, _, n in res[False][4]} == {"level_coarse": b * nc, "level_fine": b * (nc + nf)}
        assert torch.equal(res[True][3], res[False][3]), "fine sample indices"
        for lvl in ("coarse", "fine"):
            for k in ("points", "warped_points", "rgb", "depth", "med_depth", "acc", "weights", "med_points"):
                assert torch.equal(res[True][0][lvl][k], res[False][0][lvl][k]), f"reuse {case} {lvl}/{k}"
        assert res[False][1].keys() == res[True][1].keys()
        for k, g in res[False][1].items():
            assert_grad_close(res[True][1][k], g, 1e-4, f"reuse {case} {sizes} d {k}")
    finally:
        HN.set_precision("bf16")


def test_empty_ray_batch():
    """Zero rays: the reference's ATen ops return empty tensors of the usual trailing shapes; here no kernel is launched
    and the same keys / shapes come back (NerfModel.forward and the legacy render_rays)."""
    m = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=16, **CASES["bendy_cond"]).to(DEV)
    z = torch.zeros(0, 3, device=DEV)
    idx = torch.zeros(0, dtype=torch.int64, device=DEV)
    out = m({"origins": z, "directions": z, "viewdirs": None,
             "metadata": {k: idx for k in ("warp", "camera", "appearance", "time")}}, {})
    assert set(out) == {"coarse", "fine"}
    assert out["coarse"]["rgb"].shape == (0, 3) and out["fine"]["weights"].shape == (0, 24)
    assert out["fine"]["warped_points"].shape == (0, 24, 7) and out["coarse"]["med_points"].shape == (0, 1, 1)
    nets = [legacy_nerf.NeRF().to(DEV), legacy_nerf.NeRF().to(DEV)]
    emb = [legacy_nerf.Embedding(3, 10), legacy_nerf.Embedding(3, 4)]
    res = legacy_rendering.render_rays(nets, emb, torch.zeros(0, 8, device=DEV), N_samples=8, N_importance=8)
    assert sorted(res) == ["depth_coarse", "depth_fine", "opacity_coarse", "opacity_fine", "rgb_coarse", "rgb_fine"]
    assert res["rgb_fine"].shape == (0, 3) and res["depth_coarse"].shape == (0,)


def test_config2_full_size_bf16_vs_fp32_mode():
    """BASELINE config 2 at full size, the throughput mode against the parity mode on the same weights and draws
    (fp32 mode itself is held to the oracle at this size by test_config2_full_size_fp32_vs_oracle): forward within
    1e-2 of the tensor scale, the WHOLE gradient (1.5 M entries) within a relative L2 of 0.2 and a cosine of >= 0.98 —
    the small-batch bf16 bounds must also hold where every kernel runs its persistent multi-tile loops."""
    b, nc, nf, seed = 1024, 64, 64, 85
    o, d, idx = rays_for(seed, b)
    rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1).to(DEV), "u": H.uniform(seed, "u", (b, nf), 0, 1).to(DEV),
           "noise_coarse": (H.normal(seed, "n1", (b, nc, 1)) * 0.5).to(DEV),
           "noise_fine": (H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5).to(DEV)}
    gt = H.uniform(seed, "gt", (b, 3), 0, 1).to(DEV)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    res = {}
    try:
        for prec in ("fp32", "bf16"):
            HN.set_precision(prec)
            m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6,
                                 **CASES["bendy_cond"])
            load_hash(m, seed)
            m = m.to(DEV)
            out = m(rays, {}, rng=rng)
            loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
            loss.backward()
            g = torch.cat([p.grad.reshape(-1).double() for k, p in m.named_parameters() if p.grad is not None])
            res[prec] = ({k: out["coarse"][k].detach() for k in ("rgb", "depth", "acc", "weights")}, g, float(loss.detach()))
    finally:
        HN.set_precision("bf16")
    for k, v in res["bf16"][0].items():
        assert_close(v, res["fp32"][0][k].cpu(), 1e-2, f"config2 full size bf16 vs fp32 mode coarse/{k}", elementwise=False)
    assert abs(res["bf16"][2] - res["fp32"][2]) <= 2e-3 * res["fp32"][2]
    gb, gf = res["bf16"][1], res["fp32"][1]
    rel = float((gb - gf).norm() / gf.norm())
    cos = float((gb * gf).sum() / (gb.norm() * gf.norm()))
    assert rel <= 0.2 and cos >= 0.98, f"whole gradient bf16 vs fp32 mode: rel L2 {rel:.3f}, cosine {cos:.4f}"


def test_replacing_a_submodule_after_a_forward_pass_rebuilds_the_programs():
    """`model.warp_field = ...` after the level programs were compiled (they hold the old module's parameters)."""
    HN.set_precision("fp32")
    try:
        m = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, noise_std=None, **CASES["bendy_cond"]).to(DEV)
        m.use_stratified_sampling = False
        o, d, idx = rays_for(97, 16)
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        with torch.no_grad():
            a = m(rays, {})["fine"]["rgb"].clone()
            new = warping.TranslationField(in_ch=3, in_ch_embed=8).to(DEV)
            with torch.no_grad():
                for p_ in new.parameters():
                    p_.mul_(3.0)
            m.warp_field = new
            b = m(rays, {})["fine"]["rgb"].clone()
            fresh = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, noise_std=None, **CASES["bendy_cond"]).to(DEV)
            fresh.use_stratified_sampling = False
            fresh.load_state_dict(m.state_dict())
            c = fresh(rays, {})["fine"]["rgb"]
        assert not torch.equal(a, b), "the new warp field must be used"
        assert torch.equal(b, c), "and give what a freshly built model with the same weights gives"
    finally:
        HN.set_precision("bf16")


def test_structural_attribute_change_and_nested_swap_rebuild_the_programs():
    """The compiled-program cache must not outlive what shaped it: (a) a structural attribute flipped after the first
    forward (`use_viewdirs`), (b) a NESTED module replaced from outside (`model.warp_field.mlp = ...`, which the
    top-level __setattr__ never sees) — both must render what a freshly built model with the same weights renders;
    (c) a gather index of the wrong length is refused instead of indexing out of bounds."""
    HN.set_precision("fp32")
    try:
        def build():
            mm = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, noise_std=None, **CASES["bendy_cond"]).to(DEV)
            mm.use_stratified_sampling = False
            return mm
        m = build()
        o, d, idx = rays_for(98, 16)
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        with torch.no_grad():
            a = m(rays, {})["fine"]["rgb"].clone()
            # (b) nested swap
            new_mlp = modules.MLP(in_ch=m.warp_field.mlp.in_ch, out_ch=3, depth=6, width=128).to(DEV)
            for p_ in new_mlp.parameters():
                p_.mul_(2.0)
            m.warp_field.mlp = new_mlp
            b = m(rays, {})["fine"]["rgb"].clone()
            fresh = build()
            fresh.load_state_dict(m.state_dict())
            c = fresh(rays, {})["fine"]["rgb"]
            assert not torch.equal(a, b) and torch.equal(b, c), "nested module swap must rebuild the level programs"
            # (a) structural flag
            assert m.use_viewdirs
            m.use_viewdirs = False
            fresh2 = build()
            fresh2.use_viewdirs = False
            fresh2.load_state_dict(m.state_dict())
            try:
                e = m(rays, {})["fine"]["rgb"]
                f = fresh2(rays, {})["fine"]["rgb"]
                assert torch.equal(e, f), "flag flipped after the first forward must not reuse the stale program"
            except (RuntimeError, ValueError) as exc:      # a flag the constructor sized layers for: both must refuse alike
                with pytest.raises(type(exc)):
                    fresh2(rays, {})
            # (c)
            m2 = build()
            bad = dict(rays, metadata={k: idx[:5].to(DEV) for k in ("warp", "camera", "appearance", "time")})
            with pytest.raises(L.HnError):
                m2(bad, {})
    finally:
        HN.set_precision("bf16")


def test_deepcopy_and_pickle_of_a_model_with_compiled_programs():
    """copy.deepcopy (EMA copies, Lightning) and torch.save(model) after a forward pass: the copy runs on ITS weights,
    the original is untouched, the pickle round trip renders the same image."""
    import copy
    import io
    HN.set_precision("fp32")
    try:
        m = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, noise_std=None, **CASES["bendy_cond"]).to(DEV)
        m.use_stratified_sampling = False
        o, d, idx = rays_for(97, 16)
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        with torch.no_grad():
            a = m(rays, {})["fine"]["rgb"].clone()
            m2 = copy.deepcopy(m)
            for p_ in m2.parameters():
                p_.mul_(1.5)
            b = m2(rays, {})["fine"]["rgb"].clone()
            a2 = m(rays, {})["fine"]["rgb"].clone()
        assert not torch.equal(a, b) and torch.equal(a, a2)
        buf = io.BytesIO()
        torch.save(m, buf)
        buf.seek(0)
        m3 = torch.load(buf, weights_only=False)
        with torch.no_grad():
            c = m3(rays, {})["fine"]["rgb"]
        assert torch.equal(a, c)
    finally:
        HN.set_precision("bf16")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_model_random_sizes_fuzz(prec):
    """The full render path on 16 seeded random (configuration, rays, coarse, fine) combinations — 1..65 rays, 3..70
    coarse and 1..70 fine samples, i.e. ragged last blocks, samples-per-ray that are and are not multiples of 32 (the
    in-kernel and the fall-back embedding gradient), all four warp / slice structures — in fp32 mode against the oracle:
    coarse tensors 1e-4 element-wise, fine-index agreement, whole-gradient relative L2 <= 1e-2; and in bf16 mode against
    the oracle under the same arithmetic contract (O.bf16_operands): coarse tensors 2e-3 of their scale, whole gradient
    <= 0.2 (tiny batches: a single ReLU decision on a rounding boundary is a visible share of the gradient)."""
    import contextlib
    HN.set_precision(prec)
    rs = np.random.RandomState(2468)
    cases = {"bendy_cond": (CASES["bendy_cond"], "translation"), "axis": (CASES["axis"], "translation"),
             "nowarp_cond": (CASES["nowarp_cond"], "translation"),
             "se3_axis": (dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=True,
                               use_alpha_cond=True), "se3")}
    try:
        for it in range(16):
            name = list(cases)[it % 4]
            kw, warp_kind = cases[name]
            b = int(rs.choice([1, 2, 7, 33, 65]))
            nc = int(rs.choice([3, 4, 8, 31, 32, 33, 64, 70]))      # 2 coarse samples leave no pdf bin: the reference errors
            nf = int(rs.choice([1, 2, 8, 32, 33, 64, 70]))
            seed = 700 + it
            what = f"model fuzz {it}: {name} rays {b} coarse {nc} fine {nf}"
            m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
            if warp_kind == "se3":
                m.warp_field = warping.SE3Field(in_ch=3)
            sd = H.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
            for k in sd:
                if k.startswith(("warp_field.w_net.logit_layer", "warp_field.v_net.logit_layer")):
                    sd[k] = sd[k] * 0.02
            m.load_state_dict(sd)
            m = m.to(DEV)
            o, d, idx = rays_for(seed, b)
            if b == 1:
                idx = idx[:, None]      # (1,) indices lose their batch axis in the reference's GLOEmbed (modules.py:164-165)
            rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
                   "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5,
                   "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
            cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6,
                             warp_kind=warp_kind, **kw)
            p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
            gt = H.uniform(seed, "gt", (b, 3), 0, 1)
            with (O.bf16_operands() if prec == "bf16" else contextlib.nullcontext()):
                ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
                O.mse_loss(ref, gt).backward()
            rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                    "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
            out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
            for k in ("rgb", "depth", "acc", "weights", "warped_points"):
                if prec == "fp32":
                    assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"{what} coarse/{k}")
                else:
                    assert_close(out["coarse"][k], ref["coarse"][k], 2e-3, f"bf16 {what} coarse/{k}", elementwise=False)
            same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
            assert same >= (0.99 if prec == "fp32" else 0.9), f"{what}: only {same:.4f} of the fine-sample indices agree"
            if same == 1.0 and prec == "fp32":
                for k in ("rgb", "depth", "acc", "weights"):
                    assert_close(out["fine"][k], ref["fine"][k], 1e-4, f"{what} fine/{k}")
            loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
            loss.backward()
            named = dict(m.named_parameters())
            ks = [k for k in named if p[k].grad is not None and named[k].grad is not None]
            ga = torch.cat([named[k].grad.detach().cpu().double().reshape(-1) for k in ks])
            ra = torch.cat([p[k].grad.double().reshape(-1) for k in ks])
            rel = float((ga - ra).norm() / ra.norm())
            bound = (1e-2 if same == 1.0 else 5e-2) if prec == "fp32" else 0.2
            assert rel <= bound, f"{prec} {what}: whole-gradient rel L2 {rel:.2e}"
    finally:
        HN.set_precision("bf16")


LEGACY = {
    "c_only": dict(N_samples=16, N_importance=0, perturb=0, noise_std=0),
    "c_only_pert_noise": dict(N_samples=16, N_importance=0, perturb=1, noise_std=1),
    "cf_det": dict(N_samples=16, N_importance=16, perturb=0, noise_std=0),
    "cf_pert_noise": dict(N_samples=16, N_importance=16, perturb=1, noise_std=1),
    "cf_white": dict(N_samples=16, N_importance=16, perturb=1, noise_std=0, white_back=True),
    "cf_test_time": dict(N_samples=16, N_importance=16, perturb=0, noise_std=0, test_time=True),
    "cf_disp": dict(N_samples=16, N_importance=8, perturb=1, noise_std=1, use_disp=True),
    "c64": dict(N_samples=64, N_importance=0, perturb=1, noise_std=1),
}


def legacy_rng(g, kw):
    kinds = g["draw_kinds"].tolist()
    draws = [torch.from_numpy(g[f"draw{i}"]) for i in range(len(kinds))]
    rng, i = {}, 0
    if kw["perturb"] > 0:
        rng["perturb_rand"] = draws[i]; i += 1
    rng["noise_coarse"] = draws[i]; i += 1
    if kw["N_importance"] > 0:
        if kw["perturb"] > 0:
            rng["u"] = draws[i]; i += 1
        rng["noise_fine"] = draws[i]; i += 1
    return rng


@pytest.mark.parametrize("name", sorted(LEGACY))
def test_golden_legacy_render_rays(golden_dir, name):
    """nerf_pl render_rays (BASELINE config 1 family) in fp32 mode vs the reference's outputs."""
    HN.set_precision("fp32")
    g = np.load(os.path.join(golden_dir, "g12_legacy_" + name + ".npz"))
    kw = LEGACY[name]
    seed = int(g["seed"])
    coarse, fine = legacy_nerf.NeRF(), legacy_nerf.NeRF()
    assert sorted(coarse.state_dict().keys()) == g["keys"].tolist()
    load_hash(coarse, seed); load_hash(fine, seed + 1)
    coarse, fine = coarse.to(DEV), fine.to(DEV)
    emb = [legacy_nerf.Embedding(3, 10), legacy_nerf.Embedding(3, 4)]
    rays = torch.from_numpy(g["rays"]).to(DEV)
    rng = {k: v.to(DEV) for k, v in legacy_rng(g, kw).items()}
    res = legacy_rendering.render_rays([coarse, fine], emb, rays, rng=rng, **kw)
    for k in [k for k in g.files if k.startswith("out/")]:
        assert_close(res[k[4:]], torch.from_numpy(g[k]), 1e-4, f"{name} {k}")
    if "loss" in g.files:
        b = rays.shape[0]
        gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0).to(DEV)
        loss = ((res["rgb_coarse"] - gt) ** 2).mean()
        if "rgb_fine" in res:
            loss = loss + ((res["rgb_fine"] - gt) ** 2).mean()
        assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4
        loss.backward()
        grad_stats_close({k: v.grad for k, v in coarse.named_parameters()}, g, "gradc/", 5e-3)
        if "rgb_fine" in res:
            grad_stats_close({k: v.grad for k, v in fine.named_parameters()}, g, "gradf/", 5e-3)


@pytest.mark.parametrize("b,nc,nf", [(1024, 64, 64), (16384, 64, 128)], ids=["config2", "config3"])
def test_full_size_properties(b, nc, nf):
    """BASELINE config 2 (1024 rays x (64+64)) and config 3 (16,384 rays x (64+128) = 4.2 M evaluated points, a 60 GB
    activation stash), bendy sheet, bf16, forward + backward at FULL size: size-independent properties of the result
    (ranges, weights sum to <= 1, opacity = sum of weights, merged depths sorted, every gradient finite; linearity
    of the loss head: d loss / d rgb of the mean-square loss = 2 rgb / numel)."""
    HN.set_precision("bf16")
    torch.manual_seed(0)
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0,
                         hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True,
                         view_fourier_dim=6).to(DEV)
    o, d, idx = rays_for(11, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    out = m(rays, {})
    for lvl, s in (("coarse", nc), ("fine", nc + nf)):
        r = out[lvl]
        assert r["rgb"].shape == (b, 3) and r["weights"].shape == (b, s)
        assert r["warped_points"].shape == (b, s, 7) and r["med_points"].shape == (b, 1, 1)
        assert torch.isfinite(r["rgb"]).all() and (r["rgb"] >= 0).all() and (r["rgb"] <= 1.0 + 1e-3).all()
        assert (r["weights"] >= 0).all() and (r["weights"].sum(-1) <= 1.0 + 1e-2).all()
        assert torch.allclose(r["acc"], r["weights"][:, :-1].sum(-1), atol=1e-5)
    z = m.last_sampling["z_fine"]
    assert (z[:, 1:] >= z[:, :-1]).all(), "merged fine depths must be sorted"
    out["fine"]["rgb"].retain_grad()
    loss = (out["coarse"]["rgb"] ** 2).mean() + (out["fine"]["rgb"] ** 2).mean()
    loss.backward()
    assert torch.allclose(out["fine"]["rgb"].grad, 2.0 * out["fine"]["rgb"].detach() / (3 * b), rtol=1e-5, atol=1e-12)
    for k, prm in m.named_parameters():
        if k.startswith("nerf_embed"):
            continue    # unused when GLO tables are shared
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), k
    used = torch.unique(idx)
    assert bool((m.warp_embed.embed.weight.grad[used.to(DEV)].abs().sum(-1) > 0).all()), "every GLO row in use gets a gradient"


def test_config2_full_size_fp32_vs_oracle():
    """BASELINE config 2 at its FULL size (1024 rays x (64+64) = 196,608 evaluated points, the fused level programs,
    the in-kernel embedding gradient path with 32-point blocks inside one ray) in fp32 mode against the CPU oracle:
    forward tensors element-wise to 1e-4, loss, the gradient of the GLO table (every point of the batch contributes to
    it through all three networks) and every weight gradient (relative L2)."""
    HN.set_precision("fp32")
    try:
        kw = CASES["bendy_cond"]
        b, nc, nf, seed = 1024, 64, 64, 83
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0, view_fourier_dim=6, **kw)
        sd = load_hash(m, seed)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)), "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1))}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0, view_fourier_dim=6, **kw)
        torch.set_num_threads(oracle_threads(64))
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        ref_loss = O.mse_loss(ref, gt)
        ref_loss.backward()
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
        for k in ("rgb", "depth", "acc", "weights", "warped_points"):
            assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"config2 full size coarse/{k}")
        same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.9995, f"only {same:.5f} of the 65,536 fine-sample indices agree"
        # the isolating statement behind "bit-exact fine-sample indices": end to end the indices depend on the coarse
        # weights, which two fp32 implementations agree on to ~1e-6 — a draw u that sits that close to a cdf step lands
        # in the neighbouring bin (the <= 0.05 % above).  Fed the ORACLE's coarse weights and depths, the HIP inverse-CDF
        # kernel reproduces every one of the 65,536 indices, the samples and the merged sort exactly.
        z_c = m.last_sampling["z_coarse"]
        assert torch.equal(z_c.cpu(), O.sample_along_rays(o, d, nc, 0.0, 1.0, rng["t_rand"])[0]), "coarse depths bit-exact"
        z_all, _, inds_iso, _ = F.sample_pdf(ref["coarse"]["weights"].detach().to(DEV), z_c, rng["u"].to(DEV),
                                             o.to(DEV), d.to(DEV))
        flips = int((inds_iso.cpu() != ref["fine"]["_inds"]).sum())
        assert flips == 0, f"{flips} index flips with identical coarse weights"
        mid = 0.5 * (z_c[:, 1:] + z_c[:, :-1]).cpu()
        z_ref2, _, _ = O.sample_pdf(mid, ref["coarse"]["weights"].detach()[:, 1:-1], o, d, z_c.cpu(), rng["u"])
        assert torch.equal(z_all.cpu(), z_ref2), "merged sorted fine depths bit-exact on identical coarse weights"
        # a fine sample that lands in the neighbouring pdf bin changes that ray's fine render: compare the rays whose
        # indices all agree (> 97 % of them)
        ok = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).all(dim=1)
        assert float(ok.float().mean()) > 0.97
        for k in ("rgb", "depth", "acc"):
            assert_close(out["fine"][k][ok.to(DEV)], ref["fine"][k][ok], 1e-4, f"config2 full size fine/{k}")
        from hypernerf_torch_amd import losses
        loss = losses.MSELoss()(out, gt.to(DEV))
        assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 2e-5 * max(1.0, float(ref_loss.detach()))
        loss.backward()
        # one fine sample that lands in the neighbouring pdf bin (<= 0.05 % of them do) moves its ray's share of a
        # table row by ~1/128, so the max-norm bound is 2e-2 here and the tight statement is the relative L2
        g, gr = m.warp_embed.embed.weight.grad, p["warp_embed.embed.weight"].grad
        assert_grad_close(g, gr, 2e-2, "config2 d GLO table (max)")
        assert_grad_close(g, gr, 5e-3, "config2 d GLO table (rel L2)", frobenius=True)
        # EVERY weight gradient at full size (the weight-gradient kernel's jobs run hundreds of LDS stages here, the
        # small-batch tests only two or three): whole gradient and every tensor that carries >= 0.1 % of it, relative L2
        named = dict(m.named_parameters())
        ks = [k for k in named if p[k].grad is not None and named[k].grad is not None]
        assert len(ks) >= 60
        ga = torch.cat([named[k].grad.detach().cpu().double().reshape(-1) for k in ks])
        ra = torch.cat([p[k].grad.double().reshape(-1) for k in ks])
        tot = float(ra.norm())
        rel = float((ga - ra).norm()) / tot
        assert rel <= 3e-3, f"config 2 full size: whole-gradient rel L2 {rel:.2e} against the oracle"
        for k in ks:
            if float(p[k].grad.norm()) >= 1e-3 * tot:
                assert_grad_close(named[k].grad, p[k].grad, 1e-2, f"config2 full size d {k}", frobenius=True)
    finally:
        HN.set_precision("bf16")


def test_config3_full_size_subset_vs_oracle():
    """BASELINE config 3 at its FULL size — ONE launch of 16,384 rays x (64 + 128) samples = 4.2 M evaluated points,
    the persistent tile loops, weight-gradient jobs of hundreds of LDS stages, a > 100 GB fp32 activation stash — pinned
    to the CPU oracle through a seeded subset: rays are independent (models.py:673-780), so the oracle run on 256 of
    the launch's rays (same rows of the draws) must reproduce those rows of the full launch (forward 1e-4), and with the
    loss masked to those rays the WHOLE weight gradient and the GLO-table gradient of the full-size backward (every
    other ray contributes an exact zero through every kernel) must be the oracle's (rel L2 <= 3e-3)."""
    HN.set_precision("fp32")
    try:
        kw = CASES["bendy_cond"]
        b, nc, nf, nsel, seed = 16384, 64, 128, 256, 93
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0, view_fourier_dim=6, **kw)
        sd = load_hash(m, seed)
        m = m.to(DEV)
        free, _ = torch.cuda.mem_get_info()
        prog = m._level_call("fine").program
        need = sum(prog.layout(L.HN_MODE_F32, b * s)[1] + prog.layout(L.HN_MODE_F32, b * s)[2] for s in (nc, nc + nf))
        if need * 1.15 > free:
            pytest.skip(f"fp32 stash of the full launch needs {need / 2**30:.0f} GiB, {free / 2**30:.0f} GiB free")
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)), "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1))}
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        sel = torch.from_numpy(np.sort(np.random.RandomState(seed).choice(b, nsel, replace=False)))
        # the oracle on the subset only
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0, view_fourier_dim=6, **kw)
        torch.set_num_threads(oracle_threads(64))
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o[sel], d[sel], idx[sel], {k: v[sel] for k, v in rng.items()})
        ref_loss = O.mse_loss(ref, gt[sel])
        ref_loss.backward()
        # the full launch
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
        assert out["fine"]["weights"].shape == (b, nc + nf)
        sd_ = sel.to(DEV)
        for k in ("rgb", "depth", "acc", "weights", "warped_points"):
            assert_close(out["coarse"][k][sd_], ref["coarse"][k], 1e-4, f"config3 full size coarse/{k} (256-ray subset)")
        inds = m.last_sampling["inds"][sd_].cpu()
        same = (inds == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.999, f"only {same:.5f} of the subset's fine-sample indices agree"
        ok = (inds == ref["fine"]["_inds"]).all(dim=1)
        assert float(ok.float().mean()) > 0.9
        for k in ("rgb", "depth", "acc"):
            assert_close(out["fine"][k][sd_][ok.to(DEV)], ref["fine"][k][ok], 1e-4, f"config3 full size fine/{k} (subset)")
        # loss masked to the subset (losses.py:10-14 on those rays), backward through the FULL launch
        loss = ((out["coarse"]["rgb"][sd_] - gt[sel].to(DEV)) ** 2).mean() + ((out["fine"]["rgb"][sd_] - gt[sel].to(DEV)) ** 2).mean()
        assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 2e-5 * max(1.0, float(ref_loss.detach()))
        loss.backward()
        g, gr = m.warp_embed.embed.weight.grad, p["warp_embed.embed.weight"].grad
        assert_grad_close(g, gr, 5e-3, "config3 full size d GLO table (rel L2)", frobenius=True)
        rows_off = torch.ones(g.shape[0], dtype=torch.bool)
        rows_off[torch.unique(idx[sel])] = False
        assert float(g[rows_off.to(DEV)].abs().max()) == 0.0, "rays outside the subset must contribute exact zeros"
        named = dict(m.named_parameters())
        ks = [k for k in named if p[k].grad is not None and named[k].grad is not None]
        assert len(ks) >= 60
        ga = torch.cat([named[k].grad.detach().cpu().double().reshape(-1) for k in ks])
        ra = torch.cat([p[k].grad.double().reshape(-1) for k in ks])
        tot = float(ra.norm())
        rel = float((ga - ra).norm()) / tot
        assert rel <= 3e-3, f"config 3 full size: whole-gradient rel L2 {rel:.2e} against the oracle on the subset"
        for k in ks:
            if float(p[k].grad.norm()) >= 1e-3 * tot:
                assert_grad_close(named[k].grad, p[k].grad, 1e-2, f"config3 full size d {k}", frobenius=True)
    finally:
        HN.set_precision("bf16")


def test_config5_full_size_fp32_vs_oracle():
    """BASELINE config 5 (SE3Field warp + axis-aligned slice, GLO conditions) at its FULL size, 1024 rays x (64+64), in
    fp32 mode against the CPU oracle: coarse tensors element-wise to 1e-4, fine-index agreement, loss, and the whole
    weight gradient (SE3 trunk and heads through `hn_se3_apply`, template with the table gathered in-kernel)."""
    HN.set_precision("fp32")
    try:
        kw = dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=True, use_alpha_cond=True)
        b, nc, nf, seed = 1024, 64, 64, 87
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0, view_fourier_dim=6, **kw)
        m.warp_field = warping.SE3Field(in_ch=3)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = H.fill_state_dict(shapes, seed)
        for k in sd:        # small rigid motions: the template re-encodes warped points with sin(2^9 x)
            if k.startswith(("warp_field.w_net.logit_layer", "warp_field.v_net.logit_layer")):
                sd[k] = sd[k] * 0.02
        m.load_state_dict(sd)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)), "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1))}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=1.0, view_fourier_dim=6, warp_kind="se3", **kw)
        torch.set_num_threads(oracle_threads(64))
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        ref_loss = O.mse_loss(ref, gt)
        ref_loss.backward()
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
        for k in ("rgb", "depth", "acc", "weights", "warped_points"):
            assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"config5 full size coarse/{k}")
        same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.999, f"only {same:.5f} of the fine-sample indices agree"
        loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
        assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 5e-5 * max(1.0, float(ref_loss.detach()))
        loss.backward()
        named = dict(m.named_parameters())
        ks = [k for k in named if p[k].grad is not None and named[k].grad is not None]
        ga = torch.cat([named[k].grad.detach().cpu().double().reshape(-1) for k in ks])
        ra = torch.cat([p[k].grad.double().reshape(-1) for k in ks])
        tot = float(ra.norm())
        rel = float((ga - ra).norm()) / tot
        assert rel <= 5e-3, f"config 5 full size: whole-gradient rel L2 {rel:.2e} against the oracle"
        for k in ks:
            if float(p[k].grad.norm()) >= 1e-3 * tot:
                assert_grad_close(named[k].grad, p[k].grad, 2e-2, f"config5 full size d {k}", frobenius=True)
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
def test_param_arena_gradients_match_autograd_path():
    """The same step with parameters attached to a ParamArena (dW accumulated straight into the flat gradient
    buffer, embedding scatter-add into its view) must give the gradients the autograd-returned path gives, and
    a second backward must ACCUMULATE like torch does.  fp32 mode; the only difference allowed is the order of
    the fp32 atomic adds."""
    import hypernerf_torch_amd as HN
    HN.set_precision("fp32")
    try:
        kw = dict(n_samples_coarse=16, n_samples_fine=16, noise_std=1.0, hyper_slice_method="bendy_sheet",
                  use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
        m1 = models.NerfModel(EMB, **kw).to(DEV)
        load_hash(m1, 5)
        m2 = models.NerfModel(EMB, **kw).to(DEV)
        m2.load_state_dict(m1.state_dict())
        arena = HN.ParamArena(m2.parameters())
        o, d, idx = rays_for(3, 48)
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        b = 48
        rng = {"t_rand": torch.rand(b, 16, device=DEV), "noise_coarse": torch.randn(b, 16, 1, device=DEV),
               "u": torch.rand(b, 16, device=DEV), "noise_fine": torch.randn(b, 32, 1, device=DEV)}

        def loss_of(m):
            out = m(rays, {}, rng=rng)
            return (out["coarse"]["rgb"] ** 2).mean() + (out["fine"]["rgb"] ** 2).mean() + out["fine"]["depth"].mean()

        l1 = loss_of(m1)
        l1.backward()
        arena.zero_grad()
        l2 = loss_of(m2)
        l2.backward()
        assert float((l1 - l2).detach().abs()) <= 1e-6 * max(1.0, float(l1.detach().abs()))
        n1 = dict(m1.named_parameters())
        for name, p in m2.named_parameters():
            assert arena.attached(p) is not None, name
            g1 = n1[name].grad
            if g1 is None:
                assert float(p.grad.abs().max()) == 0.0, name
                continue
            assert_grad_close(p.grad, g1, 1e-5, name)
        first = arena.grad.clone()
        loss_of(m2).backward()              # accumulates
        assert_close(arena.grad, 2 * first, 1e-5, "accumulated gradients")
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("use_arena", [False, True])
def test_weights_are_repacked_after_fused_optimizer_step(use_arena):
    """A fused optimizer updates parameters without bumping Tensor._version; the packed weight streams must still
    follow.  After one Adam step the model has to render what a freshly built model with the updated state dict
    renders (inference mode, i.e. the change-detection path, and training mode)."""
    import hypernerf_torch_amd as HN
    HN.set_precision("fp32")
    try:
        kw = dict(n_samples_coarse=8, n_samples_fine=8, noise_std=0.0, hyper_slice_method="bendy_sheet",
                  use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
        m = models.NerfModel(EMB, **kw).to(DEV)
        load_hash(m, 9)
        o, d, idx = rays_for(4, 32)
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        rng = {"t_rand": torch.rand(32, 8, device=DEV), "u": torch.rand(32, 8, device=DEV)}
        if use_arena:
            arena = HN.ParamArena(m.parameters())
            opt = torch.optim.Adam([arena.flat_param], lr=1e-2, fused=True)
        else:
            opt = torch.optim.Adam(m.parameters(), lr=1e-2, fused=True)
        out0 = m(rays, {}, rng=rng)
        loss = (out0["fine"]["rgb"] ** 2).mean() + (out0["coarse"]["rgb"] ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            out1 = m(rays, {}, rng=rng)["fine"]["rgb"]
        out1_train = m(rays, {}, rng=rng)["fine"]["rgb"]
        fresh = models.NerfModel(EMB, **kw).to(DEV)
        fresh.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
        with torch.no_grad():
            ref = fresh(rays, {}, rng=rng)["fine"]["rgb"]
        assert float((ref - out0["fine"]["rgb"].detach()).abs().max()) > 1e-4      # the step did move the output
        assert_close(out1, ref, 1e-6, "inference after optimizer step")
        assert_close(out1_train, ref, 1e-6, "training forward after optimizer step")
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
def test_g13_se3_transform_through_the_kernel(golden_dir):
    """The one reference pin of row a19 — `rigid_body.exp_se3(S=(0,0,1,1,0,0), theta=0.5)` (tests/golden/g13_misc.npz
    `se3_T`, produced by the reference itself) — THROUGH hn_se3_apply: the kernel maps the origin and the three basis
    points with w = S_w * theta, v = S_v * theta; t = f(0), column i of R = f(e_i) - f(0); compared with the
    reference's 4x4 at 1e-4 (measured ~1e-7)."""
    g = np.load(os.path.join(golden_dir, "g13_misc.npz"))
    T_ref = torch.from_numpy(g["se3_T"]).reshape(4, 4)
    theta = 0.5
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    w = torch.tensor([0.0, 0.0, 1.0]).expand(4, 3) * theta
    v = torch.tensor([1.0, 0.0, 0.0]).expand(4, 3) * theta
    y = F.se3_apply(w.contiguous().to(DEV), v.contiguous().to(DEV), pts.to(DEV)).cpu()
    t = y[0]
    R = (y[1:] - t).T
    assert_close(R, T_ref[:3, :3], 1e-4, "g13 se3_T rotation through hn_se3_apply")
    assert_close(t, T_ref[:3, 3], 1e-4, "g13 se3_T translation through hn_se3_apply")
    assert torch.equal(T_ref[3], torch.tensor([0.0, 0.0, 0.0, 1.0]))


def test_rigid_body_module_surface(golden_dir):
    """`hypernerf.rigid_body` (round 5): the importable names of the reference's module (rigid_body.py:21-93) over the
    SE(3) kernel.  The reference's own call — exp_se3(S (1,1,6), theta (1,1)) — against its recorded 4x4 (G13, the one
    valid result upstream can produce), then batches against the oracle's restatement of the cited formulas: skew
    (exact), exp_so3 / exp_se3 (1e-4), the homogeneous helpers (exact), the single-point layout upstream returns."""
    from hypernerf_torch_amd.hypernerf import rigid_body as RB
    g = np.load(os.path.join(golden_dir, "g13_misc.npz"))
    T_ref = torch.from_numpy(g["se3_T"]).reshape(4, 4)
    S = torch.tensor([[[0.0, 0.0, 1.0, 1.0, 0.0, 0.0]]], device=DEV)
    T = RB.exp_se3(S, torch.full((1, 1), 0.5, device=DEV))
    assert T.shape == (4, 4)
    assert_close(T, T_ref, 1e-4, "rigid_body.exp_se3 vs the reference's own 4x4 (G13)")
    n, seed = 257, 47
    w = H.normal(seed, "rbw", (n, 3))
    w = w / w.norm(dim=-1, keepdim=True)
    v = H.normal(seed, "rbv", (n, 3))
    th = H.uniform(seed, "rbt", (n,), 1e-3, 3.0)
    assert torch.equal(RB.skew(w.to(DEV)).cpu(), O.skew(w))
    x = H.normal(seed, "rbx", (n, 3))
    assert_close((RB.skew(w.to(DEV)) @ x.to(DEV)[..., None])[..., 0], torch.cross(w, x, dim=-1), 1e-6, "skew(w) v == w x v")
    R_ref, p_ref = O.exp_se3(torch.cat([w, v], -1), th)
    assert_close(RB.exp_so3(w.to(DEV), th.to(DEV)), R_ref, 1e-4, "rigid_body.exp_so3 (batched)")
    Tb = RB.exp_se3(torch.cat([w, v], -1).to(DEV), th.to(DEV))
    assert Tb.shape == (n, 4, 4)
    assert_close(Tb[:, :3, :3], R_ref, 1e-4, "rigid_body.exp_se3 rotation (batched)")
    assert_close(Tb[:, :3, 3], p_ref, 1e-4, "rigid_body.exp_se3 translation (batched)")
    assert torch.equal(Tb[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(n, 4))
    assert_close(RB.exp_so3(w[:1].reshape(3).to(DEV), th[:1].to(DEV)), R_ref[0], 1e-4, "exp_so3, the reference's (3,) call")
    # inputs upstream accepts beyond unit axes (advisor, round 5): a non-unit axis is the exponential of the twist itself
    # (rotation about w/|w| by |w| theta), w = 0 the pure translation R = I, p = theta v (upstream's own result), the
    # reference's __main__ example ones(1,1,6) runs; the strict refusal is opt-in
    R2 = RB.exp_so3((2.0 * w).to(DEV), th.to(DEV))
    R2_ref, _ = O.exp_se3(torch.cat([w, v], -1), 2.0 * th)
    assert_close(R2, R2_ref, 1e-4, "rigid_body.exp_so3 with a non-unit axis == rotation by |w| theta")
    S0 = torch.cat([torch.zeros(n, 3), v], -1)
    S0[::2, :3] = w[::2]                                                  # every second screw rotates, the others do not
    T0 = RB.exp_se3(S0.to(DEV), th.to(DEV))
    assert torch.isfinite(T0).all()
    assert torch.equal(T0[1::2, :3, :3].cpu(), torch.eye(3).expand(len(T0[1::2]), 3, 3))
    assert_close(T0[1::2, :3, 3], (th[:, None] * v)[1::2], 1e-6, "exp_se3 with w = 0: p = theta v")
    assert_close(T0[::2, :3, 3], p_ref[::2], 1e-4, "exp_se3: rotating screws next to still ones")
    Tm = RB.exp_se3(torch.ones(1, 1, 6, device=DEV), torch.full((1, 1), 0.25, device=DEV))       # rigid_body.py __main__
    assert Tm.shape == (4, 4) and torch.isfinite(Tm).all()
    far = RB.exp_se3(torch.cat([w, 1e6 * v], -1).to(DEV), th.to(DEV))    # R is read with v = 0: no (R e + t) - t cancellation
    assert_close(far[:, :3, :3], R_ref, 1e-4, "exp_se3 rotation next to a translation of 1e6")
    RB.STRICT_UNIT_AXIS = True
    try:
        with pytest.raises(ValueError):
            RB.exp_so3((2.0 * w).to(DEV), th.to(DEV))                     # opt-in: not a unit axis
    finally:
        RB.STRICT_UNIT_AXIS = False
    hom = RB.to_homogenous(x[:, None, :].to(DEV))                        # (N,1,3) -> (4,N)
    assert hom.shape == (4, n) and torch.equal(hom[:3].T.cpu(), x) and bool((hom[3] == 1).all())
    one = RB.to_homogenous(x[:1, None, :].to(DEV))                       # the only shape upstream handles: identical
    assert torch.equal(one.cpu(), torch.cat([x[:1], torch.ones(1, 1)], -1).reshape(4, 1))
    back = RB.from_homogenous((Tb @ hom.T[..., None])[..., 0])           # rigid transform of each point by its own T
    assert_close(back, (R_ref @ x[..., None])[..., 0] + p_ref, 1e-4, "exp_se3 . to_homogenous . from_homogenous")
    assert torch.equal(RB.rp_to_se3(Tb[:, :3, :3], Tb[:, :3, 3]), Tb)
    with pytest.raises(L.HnError):
        RB.skew(w)                                                       # CPU tensor: no fallback


def test_translation_field_gradient_wrt_points():
    """TranslationField.warp under autograd w.r.t. its INPUT points (reference: warping.py:90-96, p + mlp(posenc(p))):
    the residual passes the output gradient through, the encoder adds its share through the MLP — against the oracle
    (fp32: output 1e-4, d points and every parameter gradient 1e-3 of the tensor's largest entry), per-point and per-ray
    embeddings."""
    HN.set_precision("fp32")
    try:
        for per_ray in (False, True):
            tf = warping.TranslationField(in_ch=3, in_ch_embed=8)
            sd = load_hash(tf, 43)
            tf = tf.to(DEV)
            b, s_ = 7, 32
            pts = H.uniform(43, "tfp", (b, s_, 3), -1.0, 1.0)
            emb = H.normal(43, "tfe", (b, 8)) * 0.1
            g = H.normal(43, "tfg", (b, s_, 3))
            p = {"wf." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
            pr, er = pts.clone().requires_grad_(True), emb.clone().requires_grad_(True)
            ref = O.translation_field(p, "wf", pr, er[:, None, :].expand(b, s_, 8))
            (ref * g).sum().backward()
            pd, ed = pts.clone().to(DEV).requires_grad_(True), emb.clone().to(DEV).requires_grad_(True)
            out = tf.warp(pd, ed if per_ray else ed[:, None, :].expand(b, s_, 8), None)
            (out * g.to(DEV)).sum().backward()
            assert_close(out, ref, 1e-4, f"TranslationField.warp (per_ray={per_ray})")
            assert_grad_close(pd.grad, pr.grad, 1e-3, "TranslationField d points")
            assert_grad_close(ed.grad, er.grad, 1e-3, "TranslationField d embedding")
            for k, prm in tf.named_parameters():
                assert_grad_close(prm.grad, p["wf." + k].grad, 1e-3, f"TranslationField d {k}")
    finally:
        HN.set_precision("bf16")


# ------------------------------------------------------------------------------------------------------------
# BASELINE config 5: SE3Field warp + axis-aligned slice ("parity unpinned" upstream: checked against the oracle's
# restatement of the formulas the reference's code states)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.7, 1e-2])
def test_se3_apply_matches_oracle_exp_map(scale):
    """hn_se3_apply_forward/backward against torch autograd through oracle.exp_se3 (rigid_body.py:55-83), fp32.
    Tolerance 1e-4 of the tensor scale (forward) / 1e-3 of the largest gradient entry."""
    from hypernerf_torch_amd import functional as F
    n, seed = 777, 31
    w = H.normal(seed, "se3w", (n, 3)) * scale
    v = H.normal(seed, "se3v", (n, 3)) * scale
    pts = H.uniform(seed, "se3p", (n, 3), -1.0, 1.0)
    g = H.normal(seed, "se3g", (n, 3))
    wr, vr, pr = (t.clone().requires_grad_(True) for t in (w, v, pts))
    theta = torch.norm(wr, dim=-1)
    R, pvec = O.exp_se3(torch.cat([wr / theta[:, None], vr / theta[:, None]], dim=-1), theta)
    ref = (R @ pr[..., None])[..., 0] + pvec
    (ref * g).sum().backward()
    wd, vd, pd = (t.clone().to(DEV).requires_grad_(True) for t in (w, v, pts))
    out = F.se3_apply(wd, vd, pd)
    (out * g.to(DEV)).sum().backward()
    assert_close(out, ref, 1e-4, "se3 warped points")
    assert_grad_close(wd.grad, wr.grad, 1e-3, "d w")
    assert_grad_close(vd.grad, vr.grad, 1e-3, "d v")
    assert_grad_close(pd.grad, pr.grad, 1e-3, "d points")


@pytest.mark.gpu
def test_se3_field_warp_vs_oracle():
    """SE3Field.warp (trunk on the HIP machine, heads, exp-map kernel) against oracle.se3_field; fp32 <= 1e-4,
    parameter gradients <= 1e-3 of each tensor's largest entry."""
    HN.set_precision("fp32")
    try:
        f = warping.SE3Field(in_ch=3)
        sd = load_hash(f, 41)
        f = f.to(DEV)
        pts = H.uniform(41, "se3pts", (6, 50, 3), -1.0, 1.0)
        g = H.normal(41, "se3go", (6, 50, 3))
        p = {"wf." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
        pr = pts.clone().requires_grad_(True)
        ref = O.se3_field(p, "wf", pr)
        (ref * g).sum().backward()
        pg = pts.to(DEV).requires_grad_(True)
        out = f.warp(pg, None, {"warp_alpha": None})
        assert out.shape == (6, 50, 3)
        (out * g.to(DEV)).sum().backward()
        assert_close(out, ref, 1e-4, "SE3Field.warp")
        for k, prm in f.named_parameters():
            assert_grad_close(prm.grad, p["wf." + k].grad, 1e-3, f"SE3Field d {k}")
        # gradient w.r.t. the points: through R p + t (hn_se3_apply_backward) and through encoder + trunk + heads
        assert_grad_close(pg.grad, pr.grad, 1e-3, "SE3Field d points")
        # no library GEMM: the only launches of a forward are the machine and the exp-map kernel
        from hypernerf_torch_amd import _lib as L
        L.KERNEL_TIMES = {}
        with torch.no_grad():
            f.warp(pts.to(DEV), None, {"warp_alpha": None})
        names = set(k.split("[")[0] for k in L.collect_kernel_times())
        L.KERNEL_TIMES = None
        assert names <= {"hn_mlp_forward", "hn_se3_warp_forward", "hn_pack_units"}, names
        assert set(f(pts.to(DEV), None, {"warp_alpha": None}).keys()) == {"warped_points"}
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
def test_se3_warped_rows_carry_gradients_to_field_and_table():
    """A loss on `warped_points` of a config-5 level (= [xyz | GLO row], written by the exp-map launch) reaches the
    field through its xyz columns and the embedding table through its row columns, like the reference's differentiable
    cat([xyz, rows]) (models.py:578-581): compared with the same loss on torch.cat of the plain se3_warp output and
    an index_select of the table."""
    from hypernerf_torch_amd import functional as F
    b, s, hdim, rows, seed = 5, 32, 8, 11, 77
    n = b * s
    wv = (H.normal(seed, "wv", (n, 6)) * 0.3).to(DEV)
    pts = H.uniform(seed, "p", (n, 3), -1.0, 1.0).to(DEV)
    table = H.normal(seed, "tab", (rows, hdim)).to(DEV)
    idx = torch.tensor([3, 0, 10, 3, 7], device=DEV)
    gx = H.normal(seed, "gx", (n, 3)).to(DEV)
    gw = H.normal(seed, "gw", (n, 3 + hdim)).to(DEV)
    a_wv, a_p, a_t = (t.clone().requires_grad_(True) for t in (wv, pts, table))
    xyz, warped = F.se3_warp(a_wv, a_p, a_t, idx, s)
    assert warped.requires_grad and warped.shape == (n, 3 + hdim)
    ((xyz * gx).sum() + (warped * gw).sum()).backward()
    r_wv, r_p, r_t = (t.clone().requires_grad_(True) for t in (wv, pts, table))
    xyz_r = F.se3_warp(r_wv, r_p)
    warped_r = torch.cat([xyz_r, r_t.index_select(0, idx).repeat_interleave(s, dim=0)], dim=1)
    ((xyz_r * gx).sum() + (warped_r * gw).sum()).backward()
    assert_close(warped, warped_r, 1e-6, "warped rows")
    assert_grad_close(a_wv.grad, r_wv.grad, 1e-5, "d wv through warped")
    assert_grad_close(a_p.grad, r_p.grad, 1e-5, "d points through warped")
    assert_grad_close(a_t.grad, r_t.grad, 1e-5, "d table through warped")
    # the training step's own use (gradient through xyz only) is unchanged
    b_wv = wv.clone().requires_grad_(True)
    xyz2, warped2 = F.se3_warp(b_wv, pts, table, idx, s)
    (xyz2 * gx).sum().backward()
    c_wv = wv.clone().requires_grad_(True)
    (F.se3_warp(c_wv, pts) * gx).sum().backward()
    assert torch.equal(b_wv.grad, c_wv.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("cond", [False, True])
def test_config5_se3_warp_axis_aligned_model_vs_oracle(cond):
    """Config 5 end to end: NerfModel with `warp_field = SE3Field(3)` and hyper_slice_method='axis_aligned_plane'
    against the oracle (fp32, same draws): outputs <= 1e-4, gradients <= 1e-2 of each tensor's largest entry.
    With the template GLO condition on, the template differentiates into 3 + 8 + 8 = 19 source components
    (more than one half of the source-gradient accumulator tile)."""
    HN.set_precision("fp32")
    try:
        kw = dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=cond,
                  use_alpha_cond=cond)
        nc = nf = 16
        b, seed = 40, 53
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
        m.warp_field = warping.SE3Field(in_ch=3)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = H.fill_state_dict(shapes, seed)
        for k in sd:        # small rigid motions: the template re-encodes warped points with sin(2^9 x)
            if k.startswith(("warp_field.w_net.logit_layer", "warp_field.v_net.logit_layer")):
                sd[k] = sd[k] * 0.02
        m.load_state_dict(sd)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5,
               "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6,
                         warp_kind="se3", **kw)
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        O.mse_loss(ref, gt).backward()
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
        for k in ("rgb", "depth", "acc", "weights", "warped_points"):
            assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"config5 coarse/{k}")
        loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
        loss.backward()
        for k, prm in m.named_parameters():
            assert_grad_close(prm.grad, p[k].grad, 5e-3, f"config5 d {k}")
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
def test_batched_inference_and_render_image_match_one_shot():
    """eval.py's chunk loop: chunked rendering == one forward over all rays (deterministic sampling), reference
    result layout for batched_inference, requested keys only for render_image."""
    from hypernerf_torch_amd.inference import batched_inference, render_image
    HN.set_precision("fp32")
    try:
        m = models.NerfModel(EMB, n_samples_coarse=16, n_samples_fine=16, noise_std=None, view_fourier_dim=6,
                             **CASES["bendy_cond"])
        load_hash(m, 17)
        m = m.to(DEV).eval()
        m.use_stratified_sampling = False
        o, d, idx = rays_for(17, 100)
        rays = torch.cat([o, d, torch.zeros(100, 1), torch.ones(100, 1), idx.float()[:, None]], dim=1).to(DEV)
        from hypernerf_torch_amd.hypernerf import model_utils as MU
        with torch.no_grad():
            ref = m(MU.prepare_ray_dict(rays), {})
        res = batched_inference(m, MU.prepare_ray_dict(rays), 16, 16, False, 32, False)
        assert set(res) == {"coarse", "fine"} and set(res["fine"]) == set(ref["fine"])
        for lvl in ("coarse", "fine"):
            for k in ("rgb", "depth", "acc", "weights", "points", "warped_points"):
                assert res[lvl][k].shape == ref[lvl][k].shape, (lvl, k)
                assert_close(res[lvl][k], ref[lvl][k], 1e-6, f"chunked {lvl}/{k}")
        img = render_image(m, rays, chunk=48, keys=("rgb", "depth"))
        assert set(img) == {"rgb", "depth"} and img["rgb"].shape == (100, 3)
        assert_close(img["rgb"], ref["fine"]["rgb"], 1e-6, "render_image rgb")
        assert_close(img["depth"], ref["fine"]["depth"], 1e-6, "render_image depth")
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_train_step_harness(use_graph):
    """training.TrainStep (reference: train.py training_step): loss falls on a fixed batch, the log has the
    reference's keys, graph replay and eager stepping agree on the first logged loss."""
    from hypernerf_torch_amd.training import TrainStep
    HN.set_precision("bf16")
    torch.manual_seed(3)
    m = models.NerfModel(EMB, n_samples_coarse=32, n_samples_fine=32, noise_std=1.0, view_fourier_dim=6,
                         **CASES["bendy_cond"]).to(DEV)
    o, d, idx = rays_for(23, 256)
    rays = torch.cat([o, d, torch.zeros(256, 1), torch.ones(256, 1), idx.float()[:, None]], dim=1).to(DEV)
    rgbs = H.uniform(23, "rgbs", (256, 3), 0.2, 0.8).to(DEV)
    ts = TrainStep(m, lr=2e-3, use_graph=use_graph)
    logs = [ts.step(rays, rgbs) for _ in range(40)]
    assert set(logs[0]) == {"train/loss", "train/psnr", "lr"}
    first, last = float(logs[0]["train/loss"]), float(logs[-1]["train/loss"])
    assert math.isfinite(first) and math.isfinite(last)
    assert last < 0.6 * first, (first, last)
    assert float(logs[-1]["train/psnr"]) > float(logs[0]["train/psnr"])
    assert ts.arena.attached(m.warp_field.mlp.linears[0].weight) is not None


@pytest.mark.gpu
def test_config3_sample_counts_vs_oracle_and_edge_batches():
    """BASELINE config 3's sample counts (64 coarse + 128 fine = 192-sample fine level: the widest compositing scan
    and inverse-CDF merge) against the oracle in fp32, and ragged / minimal batches (2 rays, 33 rays: partial
    workgroups; a single ray hits the reference's own GLOEmbed squeeze quirk, modules.py:162-163) through forward +
    backward."""
    HN.set_precision("fp32")
    try:
        kw = CASES["bendy_cond"]
        nc, nf, b, seed = 64, 128, 12, 61
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
        sd = load_hash(m, seed)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
               "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5,
               "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
        ref = O.nerf_model_forward({k: v.clone() for k, v in sd.items()}, cfg, o, d, idx, rng)
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
        assert out["fine"]["weights"].shape == (b, nc + nf)
        for k in ("rgb", "depth", "acc", "weights"):
            assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"config3 coarse/{k}")
        same = (m.last_sampling["inds"].cpu() == ref["fine"]["_inds"]).float().mean().item()
        assert same > 0.999, f"only {same:.4f} of fine-sample indices agree"
        for k in ("rgb", "depth", "acc"):
            assert_close(out["fine"][k], ref["fine"][k], 1e-4, f"config3 fine/{k}")
        for nb in (2, 33):
            o2, d2, idx2 = rays_for(seed + nb, nb)
            r2 = {"origins": o2.to(DEV), "directions": d2.to(DEV), "viewdirs": None,
                  "metadata": {k: idx2.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
            m.zero_grad(set_to_none=True)
            out2 = m(r2, {})
            assert out2["fine"]["rgb"].shape == (nb, 3) and torch.isfinite(out2["fine"]["rgb"]).all()
            ((out2["fine"]["rgb"] ** 2).mean() + (out2["coarse"]["rgb"] ** 2).mean()).backward()
            assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())
    finally:
        HN.set_precision("bf16")


@pytest.mark.gpu
def test_render_opts_filter_sigma_vs_oracle():
    """render_opts (reference models.py:35-63, applied to the fine level only, :768): dust threshold + bounding box
    inside the compositing kernel against the oracle, forward and gradients, fp32."""
    HN.set_precision("fp32")
    try:
        kw = CASES["bendy_cond"]
        nc = nf = 24
        b, seed = 40, 71
        m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=None, view_fourier_dim=6, **kw)
        sd = load_hash(m, seed)
        m = m.to(DEV)
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1)}
        ro = {"dust_threshold": 0.55, "bounding_box": (-0.6, 0.7, -0.8, 0.5, -0.7, 0.9)}
        cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=None, view_fourier_dim=6, **kw)
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng, render_opts=ro)
        plain = O.nerf_model_forward({k: v.clone() for k, v in sd.items()}, cfg, o, d, idx, rng)
        assert float((ref["fine"]["rgb"].detach() - plain["fine"]["rgb"]).abs().max()) > 1e-3      # the filter does something
        gt = H.uniform(seed, "gt", (b, 3), 0, 1)
        O.mse_loss(ref, gt).backward()
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        out = m(rays, {}, render_opts=ro, rng={k: v.to(DEV) for k, v in rng.items()})
        for k in ("rgb", "depth", "acc", "weights"):
            assert_close(out["coarse"][k], ref["coarse"][k], 1e-4, f"render_opts coarse/{k}")
            assert_close(out["fine"][k], ref["fine"][k], 1e-4, f"render_opts fine/{k}")
        loss = ((out["coarse"]["rgb"] - gt.to(DEV)) ** 2).mean() + ((out["fine"]["rgb"] - gt.to(DEV)) ** 2).mean()
        loss.backward()
        for k, prm in m.named_parameters():
            assert_grad_close(prm.grad, p[k].grad, 5e-3, f"render_opts d {k}")
    finally:
        HN.set_precision("bf16")
