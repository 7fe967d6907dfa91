"""GPU tests (MI355X) of the background regularization: hn_bg_loss_* and hn_bg_sample against their restatements
(tests/background_restated.py), losses.BackgroundLoss end to end against the CPU oracle's warp fields in fp32 and bf16
mode, and TrainStep(background_loss=...) eagerly and as a replayed graph."""
import json
import os

import numpy as np
import pytest
import torch

import background_restated as R
import hashprng as H
import hypernerf_torch_amd as HN
from gpu_common import DEV, EMB, load_hash, rays_for
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import models, warping
from hypernerf_torch_amd.losses import BackgroundLoss
from hypernerf_torch_amd.training import TrainStep
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
SCALES = [0.001, 0.05]
LAST = float(np.float32(1.0 - 2.0 ** -24))         # the largest 24-bit uniform


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
# loss kernels
# ----------------------------------------------------------------------------------------------------------------------
def _loss_case(n, scale):
    """fp32 (warped, points) whose x = |w - p|^2 / scale^2 is spread log-uniformly over 1e-4 .. 1e4, every eleventh row
    (from row 5) with a residual of exactly zero."""
    seed = 100 + n
    p = H.uniform(seed, "bg_p", (n, 3), -1.0, 1.0).double()
    d = H.normal(seed, "bg_d", (n, 3)).double()
    d = d / d.norm(dim=-1, keepdim=True)
    x = 10.0 ** (8.0 * H.uniform(seed, "bg_x", (n,), 0.0, 1.0).double() - 4.0)
    w = (p + d * (scale * x.sqrt())[:, None]).float()
    p = p.float()
    w[5::11] = p[5::11]
    return w, p


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_loss_kernels_match_the_restatement(n, scale):
    """Loss within 5e-6 relative, every gradient element within 5e-6 relative + 1e-12 absolute of the float64 restatement
    on the same fp32 inputs (at most ten fp32 roundings of 6e-8 per element and a log-depth sum), through the unit-root
    fast path (hn_bg_loss_forward_grad alone) and through hn_bg_loss_backward with an incoming gradient of 0.37; the
    fast path's gradient is the backward kernel's for g = 1 bit for bit, and two runs give the same bits."""
    w, p = _loss_case(n, scale)
    ref_loss = R.loss(w.numpy(), p.numpy(), scale)
    ref_grad = R.grad(w.numpy(), p.numpy(), scale)
    if n > 1:
        xs = ((w.double() - p.double()) ** 2).sum(-1) / scale ** 2
        assert float(xs[xs > 0].min()) < 1e-2 and float(xs.max()) > 1e2 and (n < 6 or bool((xs == 0).any()))

    def run(g):
        wd = w.to(DEV).requires_grad_(True)
        with _Spy() as spy:
            loss = F.bg_loss(wd, p.to(DEV), scale)
            if g is None:
                F.backward(loss)                     # the cached root gradient 1.0
            else:
                loss.backward(gradient=torch.tensor(g, device=DEV))
        return loss.detach().cpu(), wd.grad.detach().cpu(), spy.names

    def check(loss, grad, g, what):
        err = abs(float(loss) - ref_loss)
        gerr = (grad.double().numpy() - g * ref_grad)
        worst = float(np.max(np.abs(gerr) / (np.abs(g * ref_grad) + 1e-300) * (ref_grad != 0)))
        print(f"bg_loss n={n} scale={scale} {what}: loss rel err {err / max(ref_loss, 1e-300):.2e}, grad rel err {worst:.2e}")
        assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
        assert err <= 5e-6 * abs(ref_loss), (what, float(loss), ref_loss)
        assert np.all(np.abs(gerr) <= 5e-6 * np.abs(g * ref_grad) + 1e-12), (what, float(np.abs(gerr).max()))

    loss1, grad1, names1 = run(None)
    assert names1 == ["hn_bg_loss_forward_grad"], names1
    check(loss1, grad1, 1.0, "unit root")
    loss2, grad2, names2 = run(0.37)
    assert names2 == ["hn_bg_loss_forward_grad", "hn_bg_loss_backward"], names2
    check(loss2, grad2, 0.37, "g = 0.37")
    assert torch.equal(loss1, loss2)
    # zero residual rows: loss term and gradient exactly zero
    assert not bool(grad1[5::11].any()) and not bool(grad2[5::11].any())
    # the forward-only launch and a second full run: the same bits
    with torch.no_grad(), _Spy() as spy:
        loss3 = F.bg_loss(w.to(DEV), p.to(DEV), scale).cpu()
    assert spy.names == ["hn_bg_loss_forward"] and torch.equal(loss3, loss1)
    loss4, grad4, _ = run(None)
    assert torch.equal(loss4, loss1) and torch.equal(grad4, grad1)
    loss5, grad5, names5 = run(1.0)                  # a root gradient of 1 that is not the cached one: the backward kernel
    assert names5[-1] == "hn_bg_loss_backward" and torch.equal(grad5, grad1)


@pytest.mark.parametrize("n", [1, 65])
def test_zero_residual_gives_zero_loss_and_zero_gradient(n):
    p = H.uniform(7, "bg_zero", (n, 3), -1.0, 1.0).to(DEV)
    w = p.clone().requires_grad_(True)
    loss = F.bg_loss(w, p, 0.001)
    loss.backward(gradient=torch.tensor(0.37, device=DEV))
    assert float(loss) == 0.0 and not bool(w.grad.any()) and bool(torch.isfinite(w.grad).all())


# ----------------------------------------------------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("m", [1, 3, 1000])
def test_sampler_is_bit_exact(m, k, n):
    seed = 1000 * m + 10 * k + n
    pts = H.uniform(seed, "bg_pts", (m, 3), -2.0, 2.0)
    ids = torch.from_numpy(np.random.RandomState(seed).permutation(40)[:k].astype(np.int64))
    nrm = H.normal(seed, "bg_nrm", (n, 3))
    u = torch.from_numpy(H.uniform01(seed, "bg_u", 2 * n).reshape(n, 2).copy())
    if n >= 2:
        u[0], u[-1] = 0.0, LAST
        u[1, 0], u[1, 1] = LAST, 0.0
        variants = [u]
    else:
        variants = [torch.zeros(1, 2), torch.full((1, 2), LAST), u]
    for uv in variants:
        assert float(uv.min()) >= 0.0 and float(uv.max()) < 1.0
        for std in (0.25, 0.001, 0.0):
            want_p, want_i, i, j = R.sample(pts.numpy(), ids.numpy(), uv.numpy(), nrm.numpy(), std)
            assert 0 <= i.min() and i.max() < m and 0 <= j.min() and j.max() < k
            got_p, got_i = F.bg_sample(pts.to(DEV), ids.to(DEV), uv.to(DEV), nrm.to(DEV), std)
            assert got_p.dtype == torch.float32 and got_i.dtype == torch.int64
            assert np.array_equal(got_i.cpu().numpy(), want_i), (m, k, n, std)
            assert np.array_equal(got_p.cpu().numpy().view(np.uint32), want_p.view(np.uint32)), (m, k, n, std)
            if std == 0.0:          # table rows unchanged
                assert torch.equal(got_p.cpu(), pts[torch.from_numpy(i)])
    if n >= 2:
        assert i[0] == 0 and i[-1] == m - 1 and j[-1] == k - 1 and i[1] == m - 1 and j[1] == 0


def test_sampler_clamps_whatever_the_uniforms_hold():
    """An injected buffer may hold anything: NaN, negatives and values past 1 still read inside the tables."""
    pts = H.uniform(3, "bg_pts", (7, 3), -2.0, 2.0)
    ids = torch.tensor([4, 9, 2], dtype=torch.int64)
    u = torch.tensor([[float("nan"), -1.0], [1.0, 2.5], [-0.0, float("inf")], [1e30, float("-inf")]])
    got_p, got_i = F.bg_sample(pts.to(DEV), ids.to(DEV), u.to(DEV), torch.zeros(4, 3, device=DEV), 0.0)
    assert torch.equal(got_p.cpu(), pts[[0, 6, 0, 6]]) and got_i.tolist() == [4, 2, 2, 4]


# ----------------------------------------------------------------------------------------------------------------------
# losses.BackgroundLoss end to end against the oracle's warp fields
# ----------------------------------------------------------------------------------------------------------------------
E2E_N, E2E_M = 257, 50
E2E_IDS = [3, 17, 42, 5, 99, 0, 64]
E2E_SEED = 91
# bf16 mode against the oracle under O.bf16_operands(): MEASURED on the MI355X (error of the loss relative to the loss;
# per-tensor gradient error relative to the tensor's largest entry, worst tensor), the bound four times that — bf16
# operand rounding varies with the weights, and at scale = 0.001 the loss amplifies a warp error by 1e6, so no bound can
# be derived.  {(field, scale): (measured loss, measured gradient)}
BF16_MEASURED = {("translation", 0.001): (2.477e-07, 9.772e-04), ("translation", 0.05): (3.505e-06, 3.828e-04),
                 ("se3", 0.001): (5.787e-06, 1.534e-02), ("se3", 0.05): (2.053e-06, 3.918e-03)}


def _e2e_model(field):
    m = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, noise_std=None, **KW)
    if field == "se3":
        m.warp_field = warping.SE3Field(in_ch=3)
    sd = H.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, E2E_SEED)
    for k in sd:            # small rigid motions, as the config-5 model tests scale them
        if k.startswith(("warp_field.w_net.logit_layer", "warp_field.v_net.logit_layer")):
            sd[k] = sd[k] * 0.02
    m.load_state_dict(sd)
    return m.to(DEV), sd


def _e2e_inputs():
    pts = H.uniform(E2E_SEED, "bg_table", (E2E_M, 3), -1.0, 1.0)
    u = torch.from_numpy(H.uniform01(E2E_SEED, "bg_u", 2 * E2E_N).reshape(E2E_N, 2).copy())
    u[0], u[-1] = 0.0, LAST
    return pts, u, H.normal(E2E_SEED, "bg_n", (E2E_N, 3))


_ORACLE = {}


def _e2e_oracle(field, scale, sd, bf16, dtype=torch.float64):
    """(loss, {name: gradient}) of glo_embed + translation_field / se3_field + the restated loss, CPU autograd; computed
    once per case and shared."""
    key = (field, scale, bf16, dtype)
    if key not in _ORACLE:
        import contextlib
        pts, u, nrm = _e2e_inputs()
        p_np, ids_np, _, _ = R.sample(pts.numpy(), np.asarray(E2E_IDS), u.numpy(), nrm.numpy(), 0.001)
        p = torch.from_numpy(p_np).to(dtype)
        prm = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items()
               if k.startswith(("warp_field.", "warp_embed."))}
        with (O.bf16_operands() if bf16 else contextlib.nullcontext()):
            emb = O.glo_embed(prm["warp_embed.embed.weight"], torch.from_numpy(ids_np))
            w = O.translation_field(prm, "warp_field", p, emb) if field == "translation" else O.se3_field(prm, "warp_field", p)
            loss = R.loss_torch(w, p, scale)
            loss.backward()
        _ORACLE[key] = (float(loss.detach()), {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in prm.items()})
    return _ORACLE[key]


def _e2e_run(field, scale, use_arena):
    m, sd = _e2e_model(field)
    arena = HN.ParamArena(m.parameters()) if use_arena else None
    if arena is not None:
        arena.zero_grad()
    pts, u, nrm = _e2e_inputs()
    bg = BackgroundLoss(pts.to(DEV), E2E_IDS, batch_size=E2E_N, scale=scale)
    loss = bg(m, rng={"bg_u": u.to(DEV), "bg_n": nrm.to(DEV)})
    F.backward(loss)
    torch.cuda.synchronize()
    return m, sd, float(loss.detach()), {k: (None if v.grad is None else v.grad.detach().cpu().clone())
                                         for k, v in m.named_parameters()}


def _e2e_errors(grads, ref_grads):
    """Worst per-tensor gradient error relative to the tensor's largest reference entry, over the tensors the oracle
    differentiates; every other parameter's gradient must be exactly zero (SE3Field ignores the embedding: its table
    included)."""
    worst = (0.0, None)
    for k, g in grads.items():
        ref = ref_grads.get(k)
        if ref is None or not bool(ref.any()):
            assert g is None or not bool(g.any()), f"{k}: a parameter outside the term has a gradient"
            continue
        assert g is not None and bool(torch.isfinite(g).all()), k
        err = float((g.double() - ref.double()).abs().max() / ref.double().abs().max())
        if err > worst[0]:
            worst = (err, k)
    return worst


@pytest.mark.parametrize("use_arena", [True, False], ids=["arena", "autograd"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("field", ["translation", "se3"])
def test_background_loss_fp32_vs_oracle(field, scale, use_arena):
    """fp32 mode: loss, and the gradients of the warp-field weights and of the warp GLO table, within the project's fp32
    parity bound of 1e-4 relative to each tensor's largest magnitude; the gradient of every other parameter exactly
    zero.  With the parameters in a ParamArena (the training configuration) and through plain autograd."""
    HN.set_precision("fp32")
    m, sd, loss, grads = _e2e_run(field, scale, use_arena)
    ref_loss, ref_grads = _e2e_oracle(field, scale, sd, bf16=False)
    if field == "translation":
        assert bool(ref_grads["warp_embed.embed.weight"].any())
    werr, wname = _e2e_errors(grads, ref_grads)
    print(f"bg e2e fp32 {field} scale={scale} arena={use_arena}: loss {loss:.6g} ref {ref_loss:.6g} "
          f"rel err {abs(loss - ref_loss) / abs(ref_loss):.2e}; worst gradient {werr:.2e} ({wname})")
    assert 0.0 < ref_loss < 2.0
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss), (loss, ref_loss)
    assert werr <= 1e-4, (wname, werr)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("field", ["translation", "se3"])
def test_background_loss_bf16_vs_bf16_operand_oracle(field, scale):
    """bf16 mode against the oracle under O.bf16_operands() (the arithmetic contract of the MFMA path): bounds four times
    the errors measured on the MI355X, BF16_MEASURED."""
    HN.set_precision("bf16")
    m, sd, loss, grads = _e2e_run(field, scale, True)
    ref_loss, ref_grads = _e2e_oracle(field, scale, sd, bf16=True, dtype=torch.float32)
    werr, wname = _e2e_errors(grads, ref_grads)
    lerr = abs(loss - ref_loss) / abs(ref_loss)
    print(f"bg e2e bf16 {field} scale={scale}: loss {loss:.6g} ref {ref_loss:.6g} rel err {lerr:.3e}; "
          f"worst gradient {werr:.3e} ({wname})")
    m_loss, m_grad = BF16_MEASURED[(field, scale)]
    assert lerr <= 4 * m_loss, (lerr, m_loss)
    assert werr <= 4 * m_grad, (wname, werr, m_grad)


# ----------------------------------------------------------------------------------------------------------------------
# TrainStep(background_loss=...)
# ----------------------------------------------------------------------------------------------------------------------
B, NC, NF, BG_N = 64, 8, 8, 257


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
    u = torch.from_numpy(H.uniform01(seed + step, "bg_u", 2 * BG_N).reshape(BG_N, 2).copy())
    return {"t_rand": H.uniform(seed + step, "t", (B, NC), 0, 1).to(DEV), "u": H.uniform(seed + step, "u", (B, NF), 0, 1).to(DEV),
            "bg_u": u.to(DEV), "bg_n": H.normal(seed + step, "bg_n", (BG_N, 3)).to(DEV)}


def _bg(seed, **kw):
    pts = H.uniform(seed, "bg_table", (E2E_M, 3), -1.0, 1.0).to(DEV)
    return BackgroundLoss(pts, E2E_IDS, batch_size=BG_N, **kw)


def test_graph_replays_equal_eager_steps():
    """Three replayed steps against three eager ones, every random tensor injected.  The bound is the one of the existing
    graph-versus-eager test (test_first_graphed_step_applies_exactly_one_update): the same update up to the summation
    order of float atomics (the embedding tables' scatter-add), |difference| > 1e-5 for fewer than 1e-3 of the
    parameters."""
    seed = 41
    rays, rgbs = _ts_inputs(seed)
    res, logs = {}, {}
    for use_graph in (False, True):
        m = _ts_model(seed)
        ts = TrainStep(m, lr=1e-3, use_graph=use_graph, background_loss=_bg(seed))
        before = ts.arena.data.clone()
        snaps = []
        for step in range(3):
            log = ts.step(rays, rgbs, rng=_ts_rng(seed, step))
            snaps.append((ts.arena.data - before).clone())
            assert set(log) == {"train/loss", "train/psnr", "train/background_loss", "lr"}
            logs.setdefault(use_graph, []).append({k: float(v) for k, v in log.items()})
        assert float(ts.optimizer.step_count) == 3.0
        res[use_graph] = snaps
    for step in range(3):
        diff = (res[True][step] - res[False][step]).abs()
        frac = float((diff > 1e-5).float().mean())
        print(f"graph vs eager, step {step}: max |diff| {float(diff.max()):.3e}, fraction > 1e-5: {frac:.2e}, "
              f"bit-identical: {torch.equal(res[True][step], res[False][step])}")
        assert frac < 1e-3, (step, frac)
        for k in ("train/loss", "train/background_loss"):
            a, b = logs[True][step][k], logs[False][step][k]
            assert abs(a - b) <= 1e-4 * abs(b), (step, k, a, b)
    assert all(0.0 < lg["train/background_loss"] < 2.0 for lg in logs[True])


def test_replays_without_injected_draws_sample_fresh_points():
    seed = 43
    rays, rgbs = _ts_inputs(seed)
    m = _ts_model(seed)
    bg = _bg(seed)
    ts = TrainStep(m, lr=1e-3, use_graph=True, background_loss=bg)
    F.seed_draws(5)
    seen = []
    for _ in range(3):
        log = ts.step(rays, rgbs)
        pts, ids = bg.last_sample
        seen.append((pts.clone(), ids.clone()))
        assert set(ids.tolist()) <= set(E2E_IDS) and ids.shape == (BG_N,)
        assert 0.0 < float(log["train/background_loss"]) < 2.0
    assert ts._graph is not None
    for a, b in ((0, 1), (1, 2)):
        assert not torch.equal(seen[a][1], seen[b][1]) and not torch.equal(seen[a][0], seen[b][0])


def _eager_launches(ts, rays, rgbs, steps=2):
    with _Spy() as spy:
        for _ in range(steps):
            ts.step(rays, rgbs)
    torch.cuda.synchronize()
    return spy.names


def test_step_without_the_term_launches_what_it_always_did(golden_dir):
    """Built without background_loss, two eager steps make the launches recorded from the tree before the term existed
    (tests/golden/g26_trainstep_launches.json: the same model, rays and seed, entry-point names in launch order); with it,
    the four launches of the term come first and the rest of the list is unchanged."""
    with open(os.path.join(golden_dir, "g26_trainstep_launches.json")) as f:
        want = json.load(f)["launches"]
    seed = 45
    rays, rgbs = _ts_inputs(seed)
    F.seed_draws(5)
    got = _eager_launches(TrainStep(_ts_model(seed), lr=1e-3, use_graph=False), rays, rgbs)
    assert got == want, (got, want)
    assert not any(n.startswith("hn_bg_") for n in got)
    with_bg = _eager_launches(TrainStep(_ts_model(seed), lr=1e-3, use_graph=False, background_loss=_bg(seed)), rays, rgbs)
    mine = [n for n in with_bg if n.startswith("hn_bg_")]
    assert mine == ["hn_bg_sample", "hn_bg_loss_forward_grad"] * 2, mine          # weight 1.0: no backward launch
    half = _eager_launches(TrainStep(_ts_model(seed), lr=1e-3, use_graph=False, background_loss=_bg(seed, weight=0.5)),
                           rays, rgbs)
    assert [n for n in half if n.startswith("hn_bg_")] == ["hn_bg_sample", "hn_bg_loss_forward_grad",
                                                           "hn_bg_loss_backward"] * 2
    # the term sits in front of the ray chunks, and behind it the step is the default one
    assert want[0] == "hn_render_prologue"
    assert with_bg.index("hn_render_prologue") > with_bg.index("hn_bg_loss_forward_grad")
    assert with_bg[0] == "hn_random_fill" and with_bg.count("hn_random_fill") == 2      # the term's draws, once per step
    second, half_len = with_bg.index("hn_random_fill", 1), len(want) // 2
    assert with_bg[:second][-half_len:] == want[:half_len] and with_bg[second:][-half_len:] == want[half_len:]


def test_the_term_moves_only_the_warp_field_and_the_warp_embedding():
    """One eager fp32 step from the same parameters with the same draws, with the term (weight 1.0) and without it: the
    term's gradient is exactly zero outside the warp field and the warp GLO table, so every other parameter takes the
    same step, and those two take another one.  (A step whose photometric gradient vanishes altogether does not exist
    for a model that renders two levels against one target, so the comparison is against the step without the term;
    the tolerance for 'the same step' is the existing graph-versus-eager one, float atomics in the embedding
    scatter-add.)"""
    seed = 47
    rays, rgbs = _ts_inputs(seed)
    rng = _ts_rng(seed, 0)
    with torch.no_grad():      # rgb targets = the model's own fine prediction: the photometric residual is small
        from hypernerf_torch_amd.hypernerf import model_utils
        m0 = _ts_model(seed)
        out = m0(model_utils.prepare_ray_dict(rays), {}, rng={k: rng[k] for k in ("t_rand", "u")})
        rgbs = out["fine"]["rgb"].detach().clone()
    after = {}
    for with_bg in (False, True):
        m = _ts_model(seed)
        ts = TrainStep(m, lr=1e-3, use_graph=False, background_loss=_bg(seed) if with_bg else None)
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        ts.step(rays, rgbs, rng=rng if with_bg else {k: rng[k] for k in ("t_rand", "u")})
        after[with_bg] = {k: (v.detach() - before[k]).clone() for k, v in m.named_parameters()}
    moved, total, bad = [], 0, 0
    for k in after[True]:
        diff = (after[True][k] - after[False][k]).abs()
        if k.startswith(("warp_field.", "warp_embed.")):
            if float(diff.max()) > 1e-5:
                moved.append(k)
        else:
            total += diff.numel()
            bad += int((diff > 1e-5).sum())
    print(f"parameters outside the term: {bad} of {total} differ by more than 1e-5; moved by the term: {len(moved)} tensors")
    assert bad < 1e-3 * total, (bad, total)
    assert any(k.startswith("warp_embed.") for k in moved) and any(k.startswith("warp_field.mlp.") for k in moved), moved


def test_draws_for_the_term_never_reach_the_model():
    """'bg_u' / 'bg_n' carry batch_size rows, not one per ray: a step in ray chunks slices the per-ray keys only."""
    seed = 49
    rays, rgbs = _ts_inputs(seed)
    ts = TrainStep(_ts_model(seed), lr=1e-3, use_graph=False, chunk=24, background_loss=_bg(seed))
    log = ts.step(rays, rgbs, rng=_ts_rng(seed, 0))
    whole = TrainStep(_ts_model(seed), lr=1e-3, use_graph=False, background_loss=_bg(seed))
    log2 = whole.step(rays, rgbs, rng=_ts_rng(seed, 0))
    assert float(log["train/background_loss"]) == float(log2["train/background_loss"])
    assert abs(float(log["train/loss"]) - float(log2["train/loss"])) <= 1e-5 * float(log2["train/loss"])
