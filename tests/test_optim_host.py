"""CPU tests of the arena optimizers SGD / RAdam / Ranger (optim.ArenaSGD / ArenaRAdam / ArenaRanger, csrc/hn_optim.hip):
the restated update rules (tests/optim_restated.py) reproduce the reference's own trajectories
(tests/golden/g20_optimizers.npz), get_optimizer and the constructors refuse what the reference refuses before any device
work, and the C-ABI entry points refuse bad arguments with a negative status without launching anything."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import optim
from optim_restated import Restated, g20_inputs

RESTATED = {"ArenaSGD": "sgd", "ArenaRAdam": "radam", "ArenaRanger": "ranger"}


def load_g20(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_optimizers.npz"))
    return z, json.loads(str(z["meta"]))


def test_g20_covers_the_cases_the_issue_names(golden_dir):
    z, meta = load_g20(golden_dir)
    assert meta["steps"] >= 14
    n = sum(int(np.prod(s)) for s in meta["shapes"])
    assert any(int(np.prod(s)) % 4 for s in meta["shapes"])
    kinds = [c["cls"] for c in meta["cases"].values()]
    assert {k: kinds.count(k) for k in set(kinds)} == {"ArenaSGD": 3, "ArenaAdam": 1, "ArenaRAdam": 4, "ArenaRanger": 3}
    for name in meta["cases"]:
        assert z[f"{name}/params"].shape == (meta["steps"], n)
    assert os.path.getsize(os.path.join(golden_dir, "g20_optimizers.npz")) < 512 * 1024


@pytest.mark.parametrize("case", ["sgd_m09", "sgd_m09_wd", "sgd_m0", "radam", "radam_wd", "radam_nodegen",
                                  "radam_b099", "ranger", "ranger_wd", "ranger_k3", "adam"])
def test_restated_rules_reproduce_the_reference(golden_dir, case):
    """The restatement, step by step, against the reference's trajectory: parameters to 1e-6 of their scale after every
    update, final state likewise (Adam: torch.optim.Adam itself, which the reference builds)."""
    z, meta = load_g20(golden_dir)
    c = meta["cases"][case]
    init, grads = g20_inputs(meta["shapes"], meta["seed"], meta["steps"])
    params = [p.clone() for p in init]
    if c["cls"] == "ArenaAdam":
        tp = [torch.nn.Parameter(p) for p in params]
        opt = torch.optim.Adam(tp, **c["kw"])
    else:
        opt = Restated(RESTATED[c["cls"]], **{k: tuple(v) if k == "betas" else v for k, v in c["kw"].items()})
    ref = torch.from_numpy(z[f"{case}/params"])
    scale = max(1.0, float(ref.abs().max()))
    for t in range(meta["steps"]):
        if c["cls"] == "ArenaAdam":
            for p, g in zip(tp, grads[t]):
                p.grad = g.clone()
            opt.step()
            params = [p.detach() for p in tp]
        else:
            opt.step(params, grads[t])
        got = torch.cat([p.reshape(-1) for p in params])
        err = float((got - ref[t]).abs().max())
        assert err <= 1e-6 * scale, (case, t, err)
    for s in ("exp_avg", "exp_avg_sq", "slow_buffer", "momentum_buffer"):
        key = f"{case}/{s}"
        if c["cls"] == "ArenaAdam":
            mine = torch.cat([opt.state[p][s].reshape(-1) for p in tp]) if key in z.files else None
        else:
            mine = opt.flat_state(s)
        assert (mine is None) == (key not in z.files), (case, s)
        if mine is not None:
            r = torch.from_numpy(z[key])
            assert float((mine - r).abs().max()) <= 1e-6 * max(1.0, float(r.abs().max())), (case, s)


def test_the_rectified_branch_starts_where_the_reference_says():
    """fp64 schedule scalars: at beta2 = 0.999, N_sma(5) < 5 <= N_sma(6) (fp32 would give 6.0005 at t = 6)."""
    r = Restated("radam")
    for t, rect in ((5, False), (6, True)):
        r.t = t
        assert r._schedule(lambda n: n >= 5)[0] == rect


def test_get_optimizer_refuses_unknown_names_before_device_work():
    for name in ("adamw", "plainradam", "lbfgs", ""):
        with pytest.raises(ValueError, match="optimizer not recognized!"):
            optim.get_optimizer(types.SimpleNamespace(optimizer=name, lr=1e-3, momentum=0.9, weight_decay=0.0), None)
    from hypernerf_torch_amd.training import TrainStep
    with pytest.raises(ValueError, match="optimizer not recognized!"):
        TrainStep(torch.nn.Linear(2, 2), optimizer="adamw")
    with pytest.raises(ValueError, match="optimizer not recognized!"):
        TrainStep(torch.nn.Linear(2, 2), hparams=types.SimpleNamespace(optimizer="lamb"))


def _cpu_arena():
    return HN.ParamArena([torch.nn.Parameter(torch.zeros(5))])


@pytest.mark.parametrize("cls,kw,msg", [
    ("ArenaRAdam", dict(lr=-1.0), "Invalid learning rate: -1.0"),
    ("ArenaRAdam", dict(eps=-1e-8), "Invalid epsilon value: -1e-08"),
    ("ArenaRAdam", dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0: 1.0"),
    ("ArenaRAdam", dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1"),
    ("ArenaRanger", dict(alpha=1.5), "Invalid slow update rate: 1.5"),
    ("ArenaRanger", dict(k=0), "Invalid lookahead steps: 0"),
    ("ArenaRanger", dict(lr=0.0), "Invalid Learning Rate: 0.0"),
    ("ArenaRanger", dict(eps=0.0), "Invalid eps: 0.0"),
    ("ArenaSGD", dict(lr=-0.1), "Invalid learning rate: -0.1"),
    ("ArenaSGD", dict(momentum=-0.5), "Invalid momentum value: -0.5"),
    ("ArenaSGD", dict(weight_decay=-1.0), "Invalid weight_decay value: -1.0"),
    ("ArenaSGD", dict(momentum=0.0, nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
    ("ArenaSGD", dict(momentum=0.9, dampening=0.1, nesterov=True), "Nesterov momentum requires"),
])
def test_constructors_raise_the_reference_errors_without_a_gpu(cls, kw, msg):
    with pytest.raises(ValueError) as e:
        getattr(HN, cls)(_cpu_arena(), **kw)
    assert str(e.value).startswith(msg), str(e.value)


def test_valid_constructors_refuse_cpu_arenas():
    """Past the argument checks the arena must live on the GPU: there is no CPU fallback."""
    for cls in (HN.ArenaSGD, HN.ArenaRAdam, HN.ArenaRanger):
        with pytest.raises(L.HnError):
            cls(_cpu_arena())


def test_entry_points_refuse_bad_arguments_without_launching():
    HN.build()
    lib = L.load()
    assert {"hn_sgd_step", "hn_radam_step"} <= set(L.EXPORTS)
    buf = (ctypes.c_double * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c, d, s = (ctypes.c_void_p(base + 16 * i) for i in range(5))
    hyp, step = ctypes.c_void_p(base + 160), ctypes.c_void_p(base + 240)
    mis = ctypes.c_void_p(base + 4)
    sgd, radam = lib.hn_sgd_step, lib.hn_radam_step
    # n <= 0
    assert sgd(a, b, c, ctypes.c_longlong(0), hyp, step, 1, None) == -2
    assert radam(a, b, c, d, s, ctypes.c_longlong(-4), 1, hyp, step, 1, None) == -2
    # k < 1 (checked whether or not there is a slow buffer)
    assert radam(a, b, c, d, s, ctypes.c_longlong(8), 0, hyp, step, 1, None) == -2
    assert radam(a, b, c, d, None, ctypes.c_longlong(8), -1, hyp, step, 1, None) == -2
    # null pointers (the momentum / slow buffers may be NULL: no momentum, RAdam)
    assert sgd(None, b, c, ctypes.c_longlong(8), hyp, step, 1, None) == -3
    assert sgd(a, None, c, ctypes.c_longlong(8), hyp, step, 1, None) == -3
    assert sgd(a, b, c, ctypes.c_longlong(8), None, step, 1, None) == -3
    assert sgd(a, b, None, ctypes.c_longlong(8), hyp, None, 1, None) == -3
    for i in range(4):
        args = [a, b, c, d]
        args[i] = None
        assert radam(*args, s, ctypes.c_longlong(8), 1, hyp, step, 1, None) == -3
    assert radam(a, b, c, d, None, ctypes.c_longlong(8), 1, None, step, 1, None) == -3
    assert radam(a, b, c, d, None, ctypes.c_longlong(8), 1, hyp, None, 1, None) == -3
    # misaligned buffers
    assert sgd(mis, b, c, ctypes.c_longlong(8), hyp, step, 1, None) == -4
    assert sgd(a, b, mis, ctypes.c_longlong(8), hyp, step, 1, None) == -4
    assert sgd(a, b, c, ctypes.c_longlong(8), ctypes.c_void_p(base + 164), step, 1, None) == -4
    for i in range(5):
        args = [a, b, c, d, s]
        args[i] = mis
        assert radam(*args, ctypes.c_longlong(8), 1, hyp, step, 1, None) == -4
