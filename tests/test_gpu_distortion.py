"""GPU tests (MI355X) of the distortion loss: hn_distortion_* against the float64 restatement
(tests/distortion_restated.py), losses.DistortionLoss on a model against the CPU oracle in fp32 mode, and
TrainStep(distortion_loss=...) eagerly, in chunks and as a replayed graph."""
import json
import os

import numpy as np
import pytest
import torch

import distortion_restated as R
import hashprng as H
import hypernerf_torch_amd as HN
from gpu_common import DEV, EMB, assert_grad_close, load_hash, rays_for
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.losses import DistortionLoss
from hypernerf_torch_amd.training import TrainStep
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu
NEAR, FAR = 2.0, 6.0
EPS = 2.0 ** -24
# (S, B): every segment count boundary of the wave-per-ray kernel (64, 128, 192, 512), odd sizes, blocks of four rays
# that are full, partial and many (4099 rays: 1025 blocks, the last-block reduction over partials from every XCD)
SHAPES = [(1, 1), (2, 3), (3, 4), (63, 5), (64, 19), (65, 4), (128, 3), (192, 257), (257, 5), (512, 5), (64, 4099)]


class _Spy:
    """Names of the launches made through _lib.launch while active (eager code only: a replay launches nothing here)."""

    def __enter__(self):
        self.names, self._orig = [], L.launch

        def spy(name, *a, **k):
            self.names.append(name)
            return self._orig(name, *a, **k)
        L.launch = spy
        return self

    def __exit__(self, *exc):
        L.launch = self._orig
        return False


# ----------------------------------------------------------------------------------------------------------------------
# kernels against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _kernel_case(s, b):
    """fp32 (weights, z): z sorted in [NEAR, FAR], weights a softmax-like draw scaled so that sum w <= 1; from ray 1 on,
    as far as the batch reaches: all zeros, one-hot at a middle, the last and the first sample, repeated depths."""
    seed = 1000 * s + b
    z = torch.sort(H.uniform(seed, "dist_z", (b, s), NEAR, FAR), dim=1).values
    w = torch.softmax(3.0 * H.normal(seed, "dist_w", (b, s)), dim=1) * H.uniform(seed, "dist_a", (b, 1), 0.3, 0.999)
    w = w.float()
    special = ["zeros", "mid", "last", "first", "repeat"]
    for ray, kind in zip(range(1, b), special):
        if kind == "repeat":
            z[ray, 1::2] = z[ray, 0::2][:z[ray, 1::2].numel()]
            continue
        w[ray] = 0.0
        if kind != "zeros":
            w[ray, {"mid": s // 2, "last": s - 1, "first": 0}[kind]] = 1.0
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and float(w.double().sum(1).max()) <= 1.0 + 1e-6
    return w.contiguous(), z.contiguous()


@pytest.mark.parametrize("spacing", ["linear", "disparity"])
@pytest.mark.parametrize("s,b", SHAPES)
def test_kernels_match_the_restatement(s, b, spacing):
    """Per-ray loss and per-sample gradient (before the 1/B of the mean) within 16 S 2^-24 absolute of the float64
    restatement on the same fp32 inputs, the scalar within a further B 2^-24 (4/3): with s in [0, 1] and sum w <= 1 every
    partial sum is at most 1, a sum of n fp32 terms in any order is off by at most n 2^-24 sum |terms|, the gradient is two
    differences of two such sums plus a handful of roundings (8 S 2^-24 worst case), doubled for margin.  Through the
    unit-root fast path (hn_distortion_forward_grad alone), through hn_distortion_backward with an incoming gradient of
    0.37, per ray (reduction='none'), and through the fast path for an announced root of 0.25; the fast path's gradient is
    the backward kernel's for the same root bit for bit, and two runs give the same bits."""
    w, z = _kernel_case(s, b)
    ref_rays = R.per_ray(w.numpy(), z.numpy(), NEAR, FAR, spacing)
    ref_loss = float(ref_rays.mean())
    ref_grad = R.grad_rays(w.numpy(), z.numpy(), NEAR, FAR, spacing)          # (B, S), before the 1/B
    bound = 16 * s * EPS
    zd = z.to(DEV)

    def run(g, root=1.0, cached=False):
        wd = w.to(DEV).requires_grad_(True)
        with _Spy() as spy:
            loss = F.distortion_loss(wd, zd, NEAR, FAR, spacing, root=root)
            if cached:
                F.backward(loss, g)                  # the cached root gradient
            else:
                loss.backward(gradient=torch.tensor(g, device=DEV))
        return loss.detach().cpu(), wd.grad.detach().cpu(), spy.names

    def check(loss, grad, g, what):
        err = abs(float(loss) - ref_loss)
        gerr = float(np.abs(grad.double().numpy() * b / g - ref_grad).max())
        print(f"distortion S={s} B={b} {spacing} {what}: loss err {err:.2e} (bound {bound + b * EPS * 4 / 3:.2e}), "
              f"grad err {gerr:.2e} (bound {bound:.2e})")
        assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
        assert err <= bound + b * EPS * 4 / 3, (what, float(loss), ref_loss)
        assert gerr <= bound, (what, gerr)

    loss1, grad1, names1 = run(1.0, cached=True)
    assert names1 == ["hn_distortion_forward_grad"], names1
    check(loss1, grad1, 1.0, "unit root")
    loss2, grad2, names2 = run(0.37)
    assert names2 == ["hn_distortion_forward_grad", "hn_distortion_backward"], names2
    check(loss2, grad2, 0.37, "g = 0.37")
    assert torch.equal(loss1, loss2)
    loss3, grad3, names3 = run(1.0)                  # a root gradient of 1 that is not the cached one: the backward kernel
    assert names3[-1] == "hn_distortion_backward" and torch.equal(grad3, grad1)
    loss4, grad4, _ = run(1.0, cached=True)          # a second run: the same bits
    assert torch.equal(loss4, loss1) and torch.equal(grad4, grad1)
    # an announced root of 0.25: the forward launch alone, the backward kernel's bits for g = 0.25
    loss5, grad5, names5 = run(0.25, root=0.25, cached=True)
    assert names5 == ["hn_distortion_forward_grad"] and torch.equal(loss5, loss1)
    _, grad6, names6 = run(0.25)
    assert names6[-1] == "hn_distortion_backward" and torch.equal(grad5, grad6)
    check(loss5, grad5, 0.25, "root 0.25")
    # the forward-only launch, and the per-ray values with a per-ray incoming gradient
    with torch.no_grad(), _Spy() as spy:
        loss7 = F.distortion_loss(w.to(DEV), zd, NEAR, FAR, spacing).cpu()
    assert spy.names == ["hn_distortion_forward"] and torch.equal(loss7, loss1)
    wd = w.to(DEV).requires_grad_(True)
    rays = F.distortion_loss(wd, zd, NEAR, FAR, spacing, reduction="none")
    assert tuple(rays.shape) == (b,)
    rays.backward(gradient=torch.full((b,), 0.37, device=DEV))
    rerr = float(np.abs(rays.detach().cpu().double().numpy() - ref_rays).max())
    gerr = float(np.abs(wd.grad.cpu().double().numpy() / 0.37 - ref_grad).max())
    print(f"distortion S={s} B={b} {spacing} per ray: loss err {rerr:.2e}, grad err {gerr:.2e} (bound {bound:.2e})")
    assert rerr <= bound and gerr <= bound
    # all-zero rays, a one-hot ray at the last sample and S = 1: exactly zero loss; the zero ray's gradient exactly zero
    got = rays.detach().cpu()
    if b > 1:
        assert float(got[1]) == 0.0 and not bool(grad1[1].any())
    if b > 3:
        assert float(got[3]) == 0.0 and float(grad1[3, s - 1]) == 0.0
    if s == 1:
        assert not bool(got.any()) and not bool(grad1.any())


# ----------------------------------------------------------------------------------------------------------------------
# a model against the CPU oracle, fp32
# ----------------------------------------------------------------------------------------------------------------------
CASES = {
    "bendy_cond": dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True),
    "nowarp": dict(use_warp=False, hyper_slice_method=None, use_nerf_embed=False, use_alpha_cond=False),
}
# chosen on the oracle's numbers alone: at 0.1 every trunk tensor's gradient moves by more than 0.3 of its largest entry
# (the paper's 0.01 moves the coarse trunk by 0.03 .. 0.07 only: too close to the 5e-3 bound to show a wrong term)
ORACLE_WEIGHT = 0.1
GRAD_BOUND = 5e-3          # test_model_vs_oracle_larger's: of the tensor's largest entry


def _oracle_depths(points, o, d):
    """z of the oracle's sample points o + z d (its result carries no depths)."""
    o, d = o.double()[:, None], d.double()[:, None]
    return ((points.detach().double() - o) * d).sum(-1) / (d * d).sum(-1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_model_vs_oracle(case):
    """96 rays x (32 + 32), injected draws: MSE + weight x the restated term (torch, float64 on the oracle's weights) for
    levels ('coarse', 'fine').  Loss within 1e-4 relative, every gradient tensor within 5e-3 of its largest entry.  The
    fine level comes in two parts through the merge permutation (bendy_cond): weights and depths must be in one order."""
    HN.set_precision("fp32")
    kw = CASES[case]
    nc = nf = 32
    b, seed = 96, 77
    m = models.NerfModel(EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
    sd = load_hash(m, seed)
    near, far = m.near, m.far
    m = m.to(DEV)
    o, d, idx = rays_for(seed, b)
    rng = {"t_rand": H.uniform(seed, "t", (b, nc), 0, 1), "u": H.uniform(seed, "u", (b, nf), 0, 1),
           "noise_coarse": H.normal(seed, "n1", (b, nc, 1)) * 0.5, "noise_fine": H.normal(seed, "n2", (b, nc + nf, 1)) * 0.5}
    cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=0.5, view_fourier_dim=6, **kw)
    gt = H.uniform(seed, "gt", (b, 3), 0, 1)
    ref_grads, ref_loss = {}, {}
    for weight in (0.0, ORACLE_WEIGHT):
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = O.nerf_model_forward(p, cfg, o, d, idx, rng)
        loss = O.mse_loss(ref, gt)
        for lvl in ("coarse", "fine"):
            z = _oracle_depths(ref[lvl]["points"], o, d)
            assert bool((z[:, 1:] >= z[:, :-1]).all())
            loss = loss + weight * R.loss_torch(ref[lvl]["weights"].double(), z, near, far).float()
        loss.backward()
        ref_grads[weight], ref_loss[weight] = {k: v.grad for k, v in p.items()}, float(loss.detach())
    # the term is visible: on the oracle's numbers alone, every trunk gradient moves by more than ten times the bound
    trunk = [k for k in sd if ".trunk_mlp." in k]
    assert len(trunk) >= 16
    for k in trunk:
        with_, without = ref_grads[ORACLE_WEIGHT][k], ref_grads[0.0][k]
        assert float((with_ - without).abs().max()) > 10 * GRAD_BOUND * float(with_.abs().max()), k
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    out = m(rays, {}, rng={k: v.to(DEV) for k, v in rng.items()})
    term = DistortionLoss(weight=ORACLE_WEIGHT, levels=("coarse", "fine"))
    dist = term(m, out)
    loss = F.mse_loss(out["coarse"]["rgb"], out["fine"]["rgb"], gt.to(DEV)) + term.weight * dist
    loss.backward()
    got = float(loss.detach())
    print(f"distortion model {case}: loss {got:.7g} ref {ref_loss[ORACLE_WEIGHT]:.7g} (term {float(dist.detach()):.6g})")
    assert abs(got - ref_loss[ORACLE_WEIGHT]) <= 1e-4 * abs(ref_loss[ORACLE_WEIGHT])
    for k, prm in m.named_parameters():
        assert_grad_close(prm.grad, ref_grads[ORACLE_WEIGHT][k], GRAD_BOUND, f"distortion {case} d {k}")


# ----------------------------------------------------------------------------------------------------------------------
# TrainStep(distortion_loss=...)
# ----------------------------------------------------------------------------------------------------------------------
B, NC, NF = 64, 8, 8
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
TS_WEIGHT = 0.1


def _ts_model(seed, precision="fp32"):
    HN.set_precision(precision)
    m = models.NerfModel(EMB, n_samples_coarse=NC, n_samples_fine=NF, noise_std=None, **KW)
    load_hash(m, seed)
    return m.to(DEV)


def _ts_inputs(seed):
    o, d, idx = rays_for(seed, B)
    rays = torch.cat([o, d, torch.zeros(B, 1), torch.ones(B, 1), idx.float()[:, None]], dim=1).to(DEV)
    rgbs = H.uniform(seed, "rgbs", (B, 3), 0.1, 0.9).to(DEV)
    return rays, rgbs


def _ts_rng(seed, step):
    return {"t_rand": H.uniform(seed + step, "t", (B, NC), 0, 1).to(DEV), "u": H.uniform(seed + step, "u", (B, NF), 0, 1).to(DEV)}


def _term(**kw):
    return DistortionLoss(weight=TS_WEIGHT, levels=("coarse", "fine"), **kw)


class _TorchHead:
    """The same term in torch ops, with DistortionLoss's interface towards TrainStep."""
    weight = TS_WEIGHT

    def per_level(self, model, results, root=1.0):
        zs = model.last_sampling
        return [R.loss_torch(results[lv]["weights"], zs["z_" + lv], model.near, model.far) for lv in ("coarse", "fine")]


def _first_gradient(seed, term, chunk=None):
    """arena.grad and the log of one eager fp32 forward + backward from the hashed parameters and injected draws."""
    rays, rgbs = _ts_inputs(seed)
    kw = {} if chunk is None else dict(chunk=chunk)
    ts = TrainStep(_ts_model(seed), lr=1e-3, use_graph=False, distortion_loss=term, **kw)
    ts._rays, ts._rgbs, ts._rng = rays.clone(), rgbs.clone(), _ts_rng(seed, 0)
    ts._forward_backward()
    ts.optimizer.finish_gradients()
    torch.cuda.synchronize()
    return ts.arena.grad.clone(), {k: float(v) for k, v in ts._log.items()}


def _same_up_to_atomics(a, b, what):
    """The bound of the existing eager-versus-graph tests (test_first_graphed_step_applies_exactly_one_update): the same
    numbers up to the summation order of float atomics, |difference| > 1e-5 for fewer than 1e-3 of the entries."""
    diff = (a - b).abs()
    frac = float((diff > 1e-5).float().mean())
    print(f"{what}: max |diff| {float(diff.max()):.3e} (max |value| {float(b.abs().max()):.3e}), fraction > 1e-5: {frac:.2e}")
    assert bool(torch.isfinite(a).all()) and frac < 1e-3, (what, frac)


def test_hip_head_equals_a_torch_ops_head():
    seed = 51
    hip, log_hip = _first_gradient(seed, _term())
    ref, log_ref = _first_gradient(seed, _TorchHead())
    none, log_none = _first_gradient(seed, None)
    _same_up_to_atomics(hip, ref, "HIP head vs torch-ops head")
    assert abs(log_hip["train/distortion_loss"] - log_ref["train/distortion_loss"]) <= 1e-5 * log_ref["train/distortion_loss"]
    assert "train/distortion_loss" not in log_none and log_hip["train/loss"] == log_none["train/loss"]
    moved = float((hip - none).norm() / none.norm())
    print(f"the term moves the gradient by {moved:.3e} of its norm")
    assert moved > 1e-2 and 0.0 < log_hip["train/distortion_loss"] < 4.0 / 3.0 * 2


def test_graph_replays_equal_eager_steps():
    """Three replayed steps against three eager ones, every random tensor injected; the bound of the existing
    test_graph_replays_equal_eager_steps."""
    seed = 53
    rays, rgbs = _ts_inputs(seed)
    res, logs = {}, {}
    for use_graph in (False, True):
        ts = TrainStep(_ts_model(seed), lr=1e-3, use_graph=use_graph, distortion_loss=_term())
        before = ts.arena.data.clone()
        snaps = []
        for step in range(3):
            log = ts.step(rays, rgbs, rng=_ts_rng(seed, step))
            snaps.append((ts.arena.data - before).clone())
            assert set(log) == {"train/loss", "train/psnr", "train/distortion_loss", "lr"}
            logs.setdefault(use_graph, []).append({k: float(v) for k, v in log.items()})
        assert float(ts.optimizer.step_count) == 3.0
        assert (ts._graph is not None) == use_graph
        res[use_graph] = snaps
    for step in range(3):
        _same_up_to_atomics(res[True][step], res[False][step], f"graph vs eager, step {step}")
        for k in ("train/loss", "train/distortion_loss"):
            a, b = logs[True][step][k], logs[False][step][k]
            assert abs(a - b) <= 1e-4 * abs(b), (step, k, a, b)
    assert len({lg["train/distortion_loss"] for lg in logs[True]}) == 3        # fresh draws, a moving model: a live output


def test_a_step_in_chunks_equals_the_step_in_one_chunk():
    seed = 55
    whole, log_whole = _first_gradient(seed, _term())
    parts, log_parts = _first_gradient(seed, _term(), chunk=24)          # 24 + 24 + 16 rays
    _same_up_to_atomics(parts, whole, "chunks of 24 vs one chunk")
    for k in ("train/loss", "train/distortion_loss"):
        assert abs(log_parts[k] - log_whole[k]) <= 1e-6 * abs(log_whole[k]), (k, log_parts[k], log_whole[k])


def test_bf16_step_with_the_term_is_finite_and_replays():
    seed = 57
    rays, rgbs = _ts_inputs(seed)
    ts = TrainStep(_ts_model(seed, "bf16"), lr=1e-3, use_graph=True, distortion_loss=DistortionLoss())
    before = ts.arena.data.clone()
    for step in range(3):
        log = ts.step(rays, rgbs, rng=_ts_rng(seed, step))
        assert all(np.isfinite(float(log[k])) for k in ("train/loss", "train/psnr", "train/distortion_loss"))
        assert 0.0 < float(log["train/distortion_loss"]) < 4.0 / 3.0
    assert ts._graph is not None and float(ts.optimizer.step_count) == 3.0
    assert bool(torch.isfinite(ts.arena.data).all()) and not torch.equal(ts.arena.data, before)
    HN.set_precision("fp32")


def test_the_term_beside_the_background_loss_and_gradient_clipping():
    """Two steps with background_loss=, clip_grad_norm= and distortion_loss= together, every draw injected: the log carries
    all three entries, the replayed graph takes the eager steps (the atomics bound), and the clip sees a gradient the
    term has already added to: its norm differs from the one of the step without the term by more than summation order
    can (1e-5 relative; the background term's gradient dominates the norm, so the difference is small)."""
    from hypernerf_torch_amd.losses import BackgroundLoss
    seed, bg_n = 59, 257
    rays, rgbs = _ts_inputs(seed)
    pts = H.uniform(seed, "bg_table", (50, 3), -1.0, 1.0).to(DEV)

    def rng(step):
        u = torch.from_numpy(H.uniform01(seed + step, "bg_u", 2 * bg_n).reshape(bg_n, 2).copy())
        return dict(_ts_rng(seed, step), bg_u=u.to(DEV), bg_n=H.normal(seed + step, "bg_n", (bg_n, 3)).to(DEV))

    def steps(use_graph, term):
        ts = TrainStep(_ts_model(seed), lr=1e-3, use_graph=use_graph, distortion_loss=term, clip_grad_norm=1e-3,
                       background_loss=BackgroundLoss(pts, [3, 17, 42, 5, 99, 0, 64], batch_size=bg_n))
        before = ts.arena.data.clone()
        logs = [{k: float(v) for k, v in ts.step(rays, rgbs, rng=rng(i)).items()} for i in range(2)]
        return (ts.arena.data - before).clone(), logs

    eager, log_e = steps(False, _term())
    graph, log_g = steps(True, _term())
    _, log_none = steps(False, None)
    assert set(log_e[0]) == {"train/loss", "train/psnr", "train/background_loss", "train/distortion_loss",
                             "train/grad_norm", "lr"}
    _same_up_to_atomics(graph, eager, "background + clip + distortion, graph vs eager")
    for a, b in zip(log_g, log_e):
        for k in ("train/loss", "train/background_loss", "train/distortion_loss", "train/grad_norm"):
            assert abs(a[k] - b[k]) <= 1e-4 * abs(b[k]), (k, a[k], b[k])
    assert log_e[0]["train/background_loss"] == log_none[0]["train/background_loss"]
    print(f"grad norm with the term {log_e[0]['train/grad_norm']:.6f}, without {log_none[0]['train/grad_norm']:.6f}")
    assert abs(log_e[0]["train/grad_norm"] - log_none[0]["train/grad_norm"]) > 1e-5 * log_none[0]["train/grad_norm"]


def _eager_launches(ts, rays, rgbs, steps=2):
    with _Spy() as spy:
        for _ in range(steps):
            ts.step(rays, rgbs)
    torch.cuda.synchronize()
    return spy.names


@pytest.mark.parametrize("levels", [("fine",), ("coarse", "fine")])
def test_the_term_adds_one_launch_per_level_behind_the_compositing_launches(golden_dir, levels):
    """Built without the term, two eager steps make the launches of tests/golden/g26_trainstep_launches.json; built with
    it, the same list with ONE hn_distortion_forward_grad per level right behind the step's last compositing launch
    (the forward writes the already scaled gradient: no backward launch), nothing else changed or reordered."""
    with open(os.path.join(golden_dir, "g26_trainstep_launches.json")) as f:
        want = json.load(f)["launches"]
    seed = 45
    rays, rgbs = _ts_inputs(seed)
    F.seed_draws(5)
    got = _eager_launches(TrainStep(_ts_model(seed), lr=1e-3, use_graph=False), rays, rgbs)
    assert got == want, (got, want)
    assert not any(n.startswith("hn_distortion_") for n in got)
    term = DistortionLoss(levels=levels)
    with_term = _eager_launches(TrainStep(_ts_model(seed), lr=1e-3, use_graph=False, distortion_loss=term), rays, rgbs)
    expect = []
    for name in want:
        expect.append(name)
        if name == "hn_composite_forward":          # the fine level's, the last compositing launch of a step's forward
            expect += ["hn_distortion_forward_grad"] * len(levels)
    assert want.count("hn_composite_forward") == 2 and with_term == expect, (with_term, expect)
