"""GPU tests of the arena optimizers SGD / RAdam / Ranger (optim.ArenaSGD / ArenaRAdam / ArenaRanger on hn_sgd_step /
hn_radam_step, csrc/hn_optim.hip): the reference's own trajectories (tests/golden/g20_optimizers.npz), torch.optim.SGD
live, ragged buffer lengths, graph replay, TrainStep's optimizer selection and capture warm-ups, state_dict resume,
grad_scale, and a short training run against the CPU oracle with the restated RAdam (tests/optim_restated.py)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
import oracle_train as OT
from gpu_common import DEV, oracle_threads
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import optim
from hypernerf_torch_amd.hypernerf import models
from hypernerf_torch_amd.training import TrainStep
from oracle import hypernerf_oracle as O
from optim_restated import Restated, g20_inputs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_optimizers.npz")
STATE_NAMES = ("exp_avg", "exp_avg_sq", "slow_buffer", "momentum_buffer")


@pytest.fixture(scope="module")
def g20():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def arena_of(tensors):
    params = [torch.nn.Parameter(t.clone().to(DEV)) for t in tensors]
    return HN.ParamArena(params)


def set_grads(arena, grads):
    for p, g in zip(arena.params, grads):
        p.grad.copy_(g.to(DEV))


def flat_params(arena):
    return torch.cat([p.detach().reshape(-1) for p in arena.params])


def flat_unpadded(arena, t):
    return torch.cat([t[o:o + p.numel()] for p, o in zip(arena.params, arena.offsets)])


def scaled_err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def make_opt(cls, arena, kw):
    kw = {k: tuple(v) if k == "betas" else v for k, v in kw.items()}
    return getattr(HN, cls)(arena, **kw)


@pytest.mark.parametrize("case", ["sgd_m09", "sgd_m09_wd", "sgd_m0", "adam", "radam", "radam_wd", "radam_nodegen",
                                  "radam_b099", "ranger", "ranger_wd", "ranger_k3"])
def test_arena_optimizers_follow_the_reference_trajectories(g20, case):
    """Every update against the reference's recorded trajectory: parameters within 5e-6 of their scale (the tolerance
    of test_arena_adam_matches_torch_adam), the final state likewise; the gradient buffer reads zero after each step
    and the device step counter counts."""
    z, meta = g20
    c = meta["cases"][case]
    init, grads = g20_inputs(meta["shapes"], meta["seed"], meta["steps"])
    arena = arena_of(init)
    opt = make_opt(c["cls"], arena, c["kw"])
    ref = torch.from_numpy(z[f"{case}/params"])
    for t in range(meta["steps"]):
        set_grads(arena, grads[t])
        opt.step()
        assert float(arena.grad.abs().max()) == 0.0
        assert float(opt.step_count) == t + 1
        err = scaled_err(flat_params(arena), ref[t])
        assert err <= 5e-6, (case, t, err)
    for s in STATE_NAMES:
        key = f"{case}/{s}"
        mine = getattr(opt, s, None)
        assert (mine is None) == (key not in z.files), (case, s)
        if mine is not None:
            err = scaled_err(flat_unpadded(arena, mine), torch.from_numpy(z[key]))
            assert err <= 5e-6, (case, s, err)


def _launch_n(opt, n):
    """The optimizer's launch over the first n elements of its arena only (a length that is not a multiple of 4)."""
    a = opt.arena
    zg = C.c_int(1)
    if isinstance(opt, HN.ArenaSGD):
        L.launch("hn_sgd_step", L.ptr(a.data), L.ptr(a.grad), L.ptr(opt.momentum_buffer), C.c_longlong(n),
                 L.ptr(opt.hyper), L.ptr(opt._step_words), zg, L.stream_handle())
    else:
        L.launch("hn_radam_step", L.ptr(a.data), L.ptr(a.grad), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq),
                 L.ptr(opt._slow()), C.c_longlong(n), C.c_int(opt._k()), L.ptr(opt.hyper), L.ptr(opt._step_words),
                 zg, L.stream_handle())


@pytest.mark.parametrize("kind,kw", [
    ("sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-2)),
    ("radam", dict(lr=1e-2, weight_decay=1e-2)),
    ("ranger", dict(lr=1e-2, k=3, alpha=0.8)),
])
@pytest.mark.parametrize("n", [1, 3, 1001, 4 * 256 * 256 + 7])
def test_ragged_lengths_update_exactly_n_elements(kind, kw, n):
    """The scalar tail: launches over n elements of a longer buffer follow the restated rule on those n and leave the
    rest of every buffer alone (also past one full grid-stride sweep of 256 x 256 x 4)."""
    pad = 9
    x0 = H.uniform(61, "p", (n + pad,), -1, 1)
    arena = arena_of([x0])
    cls = {"sgd": HN.ArenaSGD, "radam": HN.ArenaRAdam, "ranger": HN.ArenaRanger}[kind]
    opt = cls(arena, **kw)
    total = arena.numel
    ref_p = [x0[:n].clone()]
    r = Restated(kind, **kw)
    for t in range(7):
        g = H.normal(61, f"g{t}", (total,))
        arena.grad.copy_(g.to(DEV))
        before = arena.data.clone()
        _launch_n(opt, n)
        r.step(ref_p, [g[:n]])
        got = arena.data.cpu()
        assert torch.equal(got[n:], before[n:].cpu()), "elements past n were written"
        assert torch.equal(arena.grad[n:].cpu(), g[n:]), "gradients past n were cleared"
        assert float(arena.grad[:n].abs().max()) == 0.0
        err = scaled_err(got[:n], ref_p[0])
        assert err <= 5e-6, (kind, n, t, err)
    assert float(opt.step_count) == 7.0
    for s in STATE_NAMES:
        mine = getattr(opt, s, None)
        if mine is not None:
            assert float(mine[n:].abs().max()) == 0.0, s
            assert scaled_err(mine[:n], r.flat_state(s)) <= 5e-6, s


@pytest.mark.parametrize("kw", [dict(momentum=0.0), dict(momentum=0.9), dict(momentum=0.9, nesterov=True),
                                dict(momentum=0.9, dampening=0.3), dict(momentum=0.0, weight_decay=1e-2),
                                dict(momentum=0.8, nesterov=True, weight_decay=1e-2)])
def test_arena_sgd_matches_torch_sgd(kw):
    torch.manual_seed(7)
    shapes = [(37, 19), (19,), (5, 3, 2), (1,), (130, 64)]
    p1 = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    p2 = [torch.nn.Parameter(p.detach().clone()) for p in p1]
    ref = torch.optim.SGD(p1, lr=3e-2, **kw)
    arena = HN.ParamArena(p2)
    opt = HN.ArenaSGD(arena, lr=3e-2, **kw)
    for it in range(6):
        for a, b in zip(p1, p2):
            g = torch.randn_like(a) * (0.1 + it)
            a.grad = g.clone()
            b.grad.copy_(g)
        ref.step()
        opt.step()
        assert float(arena.grad.abs().max()) == 0.0
        for a, b in zip(p1, p2):
            assert scaled_err(b, a) <= 5e-6, (kw, it)
    assert float(opt.step_count) == 6.0
    if kw["momentum"] != 0:
        o0, n0 = arena.offsets[4], p1[4].numel()
        assert scaled_err(opt.momentum_buffer[o0:o0 + n0], ref.state[p1[4]]["momentum_buffer"].reshape(-1)) <= 5e-6
    else:
        assert opt.momentum_buffer is None


CASES3 = [("ArenaSGD", dict(lr=0.05, momentum=0.9, weight_decay=1e-2)), ("ArenaRAdam", dict(lr=1e-2)),
          ("ArenaRanger", dict(lr=1e-2, k=6))]


@pytest.mark.parametrize("cls,kw", CASES3)
def test_graph_replay_matches_eager_steps_bit_for_bit(g20, cls, kw):
    """One captured step replayed 14 times = 14 eager steps, bit for bit: the first-update momentum / slow-buffer
    initialisation and the lookahead at k all come from the device step counter.  An lr change made with
    sync_hyper() reaches the replay."""
    _, meta = g20
    init, grads = g20_inputs(meta["shapes"], meta["seed"], 14)
    ea, ga = arena_of(init), arena_of(init)
    eo, go = make_opt(cls, ea, kw), make_opt(cls, ga, kw)
    flat = []
    for t in range(14):
        set_grads(ga, grads[t])
        flat.append(ga.grad.clone())
    ga.grad.zero_()
    L.load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        go.step()
    torch.cuda.synchronize()
    assert float(go.step_count) == 0.0 and torch.equal(ga.data, ea.data), "capturing must not run the step"
    for t in range(14):
        if t == 7:
            for o in (eo, go):
                o.param_groups[0]["lr"] *= 0.5
            assert go.sync_hyper()
        ea.grad.copy_(flat[t])
        eo.step()
        ga.grad.copy_(flat[t])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ga.data, ea.data), (cls, t)
        assert float(ga.grad.abs().max()) == 0.0
    assert float(go.step_count) == 14.0
    for s, e in zip(go.state_tensors(), eo.state_tensors()):
        assert torch.equal(s, e)


@pytest.mark.parametrize("cls,kw", CASES3)
def test_state_dict_resume_is_bit_exact(g20, cls, kw):
    """8 steps = 4 steps, state_dict, load into a fresh optimizer on a fresh arena, 4 more steps (Ranger k = 6: the
    resumed run crosses a lookahead sync)."""
    _, meta = g20
    init, grads = g20_inputs(meta["shapes"], meta["seed"], 8)
    a1, a2 = arena_of(init), arena_of(init)
    o1, o2 = make_opt(cls, a1, kw), make_opt(cls, a2, kw)
    for t in range(8):
        set_grads(a1, grads[t])
        o1.step()
    for t in range(4):
        set_grads(a2, grads[t])
        o2.step()
    sd = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in o2.state_dict().items()}
    a3 = arena_of([p.detach().cpu() for p in a2.params])
    o3 = make_opt(cls, a3, dict(kw, lr=kw["lr"] * 3))            # the loaded param_groups win
    o3.load_state_dict(sd)
    assert o3.param_groups[0]["lr"] == kw["lr"]
    for t in range(4, 8):
        set_grads(a3, grads[t])
        o3.step()
    assert torch.equal(a3.data, a1.data)
    for s, e in zip(o3.state_tensors(), o1.state_tensors()):
        assert torch.equal(s, e)


@pytest.mark.parametrize("cls,kw", CASES3)
def test_grad_scale_is_applied_to_the_gradient_first(g20, cls, kw):
    """grad_scale = 0.5 on a doubled gradient (the mean of a 2-rank SUM all-reduce) = grad_scale 1 on the plain one."""
    _, meta = g20
    init, grads = g20_inputs(meta["shapes"], meta["seed"], 8)
    a1, a2 = arena_of(init), arena_of(init)
    o1, o2 = make_opt(cls, a1, kw), make_opt(cls, a2, dict(kw, grad_scale=0.5))
    for t in range(8):
        set_grads(a1, grads[t])
        set_grads(a2, [2.0 * g for g in grads[t]])
        o1.step()
        o2.step()
        assert torch.equal(a1.data, a2.data), (cls, t)


# ---- TrainStep ------------------------------------------------------------------------------------------------------
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)


def small_model(seed):
    from gpu_common import EMB, load_hash
    HN.set_precision("fp32")
    m = models.NerfModel(EMB, n_samples_coarse=16, n_samples_fine=16, noise_std=None, **KW)
    load_hash(m, seed)
    return m.to(DEV)


def ray_rows(seed, b):
    from gpu_common import rays_for
    o, d, idx = rays_for(seed, b)
    return torch.cat([o, d, torch.zeros(b, 1), torch.ones(b, 1), idx.float()[:, None]], dim=1)


@pytest.mark.parametrize("name,cls", [("sgd", HN.ArenaSGD), ("radam", HN.ArenaRAdam), ("ranger", HN.ArenaRanger)])
def test_train_step_first_graphed_step_applies_exactly_one_update(name, cls):
    """TrainStep(optimizer=...): the capture warm-ups restore every piece of the optimizer's state, so the first graphed
    step applies ONE update (step counter 1; Ranger's slow buffer = the parameters before the step) and equals an eager
    first step up to the summation order of the weight-gradient atomics."""
    rays = ray_rows(32, 64).to(DEV)
    rgbs = H.uniform(32, "rgbs", (64, 3), 0.1, 0.9).to(DEV)
    res = {}
    for use_graph in (False, True):
        m = small_model(32)
        m.use_stratified_sampling = False
        ts = TrainStep(m, lr=1e-3, use_graph=use_graph, optimizer=name)
        assert type(ts.optimizer) is cls
        before = ts.arena.data.clone()
        ts.step(rays, rgbs)
        assert float(ts.optimizer.step_count) == 1.0
        if name == "ranger":
            assert torch.equal(ts.optimizer.slow_buffer, before)
        if name == "sgd":
            assert ts.optimizer.param_groups[0]["momentum"] == 0.9
            assert float(ts.optimizer.momentum_buffer.abs().max()) > 0.0
        delta = ts.arena.data - before
        assert float(delta.abs().max()) > 0.0
        res[use_graph] = delta
        ts.step(rays, rgbs)
        assert float(ts.optimizer.step_count) == 2.0
    diff = (res[True] - res[False]).abs()
    assert float((diff > 1e-5).float().mean()) < 1e-3, float((diff > 1e-5).float().mean())


def test_train_step_takes_the_optimizer_and_warm_up_rule_from_hparams():
    m = small_model(33)
    hp = dict(lr_scheduler="steplr", decay_step=[2], decay_gamma=0.5, warmup_epochs=2, warmup_multiplier=2.0,
              weight_decay=0.0)
    ts = TrainStep(m, lr=1e-3, hparams=types.SimpleNamespace(optimizer="ranger", **hp))
    assert type(ts.optimizer) is HN.ArenaRanger
    assert ts.optimizer.param_groups[0]["betas"] == (.95, 0.999)          # not the betas keyword's Adam default
    assert ts.optimizer.param_groups[0]["eps"] == 1e-8
    assert type(ts.scheduler) is optim.MultiStepLR                         # no warm-up for radam / ranger
    ts = TrainStep(m, lr=1e-3, hparams=types.SimpleNamespace(optimizer="radam", **hp))
    assert type(ts.optimizer) is HN.ArenaRAdam and type(ts.scheduler) is optim.MultiStepLR
    ts = TrainStep(m, lr=1e-3, hparams=types.SimpleNamespace(optimizer="sgd", momentum=0.5, **hp))
    assert type(ts.optimizer) is HN.ArenaSGD and ts.optimizer.param_groups[0]["momentum"] == 0.5
    assert type(ts.scheduler) is optim.GradualWarmup
    ts = TrainStep(m, lr=1e-3, hparams=types.SimpleNamespace(optimizer="adam", **hp))
    assert type(ts.optimizer) is HN.ArenaAdam and type(ts.scheduler) is optim.GradualWarmup
    ts = TrainStep(m, lr=1e-3)
    assert type(ts.optimizer) is HN.ArenaAdam
    # get_optimizer on an arena: the reference's arguments
    h = types.SimpleNamespace(optimizer="sgd", lr=0.1, momentum=0.7, weight_decay=1e-3)
    o = optim.get_optimizer(h, ts.arena)
    assert type(o) is HN.ArenaSGD and o.param_groups[0]["momentum"] == 0.7 and o.param_groups[0]["weight_decay"] == 1e-3
    o = optim.get_optimizer(types.SimpleNamespace(optimizer="ranger", lr=0.1, weight_decay=0.0), ts.arena)
    assert o.param_groups[0]["k"] == 6 and o.param_groups[0]["alpha"] == 0.5 and o.param_groups[0]["eps"] == 1e-8


def test_radam_training_tracks_the_cpu_oracle():
    """TrainStep(optimizer='radam') in fp32 (graph replay) and the CPU oracle with the restated RAdam train 16 steps
    from the same weights on the same batches and draws (tests/oracle_train.py); loss curves agree to 2e-3 relative,
    as test_training_tracks_the_cpu_oracle asks of Adam.  16 steps cross RAdam's rectification threshold (t = 6)."""
    nc = nf = 16
    b, steps, seed, lr, noise = 96, 16, 43, 5e-4, 0.5
    HN.set_precision("fp32")
    data, _ = OT.batches(seed, steps, b, nc, nf, noise)
    sd = OT.initial_state(seed, nc, nf)
    m = models.NerfModel(OT.EMB, n_samples_coarse=nc, n_samples_fine=nf, noise_std=noise, **OT.KW)
    m.load_state_dict(sd)
    m = m.to(DEV)
    ts = TrainStep(m, lr=lr, use_graph=True, chunk=40, optimizer="radam")
    cfg = O.ModelCfg(n_samples_coarse=nc, n_samples_fine=nf, noise_std=noise, **OT.KW)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ropt = Restated("radam", lr=lr, eps=1e-8)
    torch.set_num_threads(oracle_threads(32))
    cpu_loss, hip_loss = [], []
    for o, d, idx, gt, rng in data:
        for v in p.values():
            v.grad = None
        loss = O.mse_loss(O.nerf_model_forward(p, cfg, o, d, idx, rng), gt)
        loss.backward()
        live = [v for v in p.values() if v.grad is not None]
        ropt.step(live, [v.grad for v in live])
        cpu_loss.append(float(loss.detach()))
        rays = torch.cat([o, d, torch.zeros(b, 1), torch.ones(b, 1), idx.float()[:, None]], dim=1).to(DEV)
        log = ts.step(rays, gt.to(DEV), rng={k: v.to(DEV) for k, v in rng.items()})
        hip_loss.append(float(log["train/loss"]))
    cl, hl = np.array(cpu_loss), np.array(hip_loss)
    rel = np.abs(hl - cl) / cl
    print("radam loss rel err per step:", np.array2string(rel, precision=2))
    assert float(ts.optimizer.step_count) == steps
    assert rel.max() <= 2e-3, (rel.max(), cl, hl)
