"""Fused Adam on a ParamArena: one HIP kernel updates every parameter of the model and clears the
gradient buffer for the next step (`hn_adam_step`).  Same update rule and defaults as torch.optim.Adam, which is what
the reference's `get_optimizer` builds (utils/__init__.py:23-41), and `MultiStepLR` — its 'steplr' scheduler
(utils/__init__.py:43-46).  The other optimizers `get_optimizer` can build — SGD, RAdam, Ranger — follow below
(`ArenaSGD`, `ArenaRAdam`, `ArenaRanger`, `get_optimizer`), with the rest of its schedulers.

Everything a captured launch depends on lives ON THE DEVICE: the step counter and the hyper-parameters
[lr, beta1, beta2, eps, weight_decay, grad_scale].  `param_groups[0]` stays the user-facing source of truth (torch
schedulers write `lr` there); `sync_hyper()` uploads it when it changed — `step()` does that itself when it runs
eagerly, and whoever replays a graph that contains the step calls it before the replay (TrainStep does).
"""
from __future__ import annotations

from bisect import bisect_right
from typing import Sequence

import torch

from . import _lib as L
from .arena import ParamArena


# The fused reduce + Adam launch is opt-in, off by default: HN_FUSE_REDUCE=1 turns it on for the callers that pass this on
# as `fuse_reduce` (TrainStep, bench.py); measured slower than reduce, then Adam (NOTES.md, profiles/r06_reduce_adam_ab.log)
FUSE_REDUCE = __import__("os").environ.get("HN_FUSE_REDUCE", "0") != "0"


class ArenaAdam:
    def __init__(self, arena: ParamArena, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, zero_grad: bool = True, grad_scale: float = 1.0, fuse_reduce: bool = False):
        L.require_gpu(arena.data)
        self.arena = arena
        # fuse_reduce: consume the reduce launch of the batched weight gradient (machine.PendingReduce) — `step()` then
        # completes the gradient and applies the update in ONE launch (hn_mlp_wgrad_reduce_adam).  Between backward() and
        # step() the gradient buffer is then INCOMPLETE; `finish_gradients()` (or any ParamArena collective / zero_grad)
        # completes it with the plain reduce.  Single-GPU training steps only: training.TrainStep and bench.py switch it on under HN_FUSE_REDUCE=1.
        self.fuse_reduce = bool(fuse_reduce)
        if self.fuse_reduce:
            import weakref
            from . import machine
            machine.REDUCE_CONSUMERS[machine._uid(arena.grad)] = weakref.ref(self)
        self.param_groups = [{"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay}]
        self.grad_scale = float(grad_scale)        # 1 / world size when the gradients arrive SUM-all-reduced
        self.zero_grad_in_step = zero_grad
        dev = arena.data.device
        self.exp_avg = torch.zeros_like(arena.data)
        self.exp_avg_sq = torch.zeros_like(arena.data)
        self._step_words = torch.zeros(2, dtype=torch.float32, device=dev)      # [updates done, ticket counter]
        self.step_count = self._step_words[:1]
        self.hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        self._uploaded = None
        self.sync_hyper()

    def _hyper_values(self):
        g = self.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), float(self.grad_scale), 0.0, 0.0)

    def sync_hyper(self) -> bool:
        """Upload the hyper-parameters if they changed since the last upload (one 32-byte copy; never while a
        stream capture is in progress: a captured copy would freeze the values into the graph)."""
        vals = self._hyper_values()
        if vals == self._uploaded:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise L.HnError("ArenaAdam: hyper-parameters changed inside a stream capture; call sync_hyper() before")
        self.hyper.copy_(torch.tensor(vals, dtype=torch.float32))
        self._uploaded = vals
        return True

    @torch.no_grad()
    def step(self):
        L.load()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        a = self.arena
        from . import machine
        pend = machine.take_pending_reduce(a.grad)
        if pend is not None:
            rest = pend.rest_table(a.grad) if self.fuse_reduce else None
            if rest is None:            # not a partition of this arena (or fusion off): the two-launch form
                pend.plain()
                pend = None
        if pend is not None:
            f = L.HnAdamFuse()
            f.params, f.grads, f.exp_avg, f.exp_avg_sq = a.data.data_ptr(), a.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
            f.n, f.hyper, f.step = a.numel, self.hyper.data_ptr(), self.step_count.data_ptr()
            f.rest, f.n_rest, f.zero_grad = rest[0].data_ptr(), rest[1], int(self.zero_grad_in_step)
            pend.fused(f)
        else:
            L.launch("hn_adam_step", L.ptr(a.data), L.ptr(a.grad), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                     a.numel, L.ptr(self.hyper), L.ptr(self.step_count),
                     int(self.zero_grad_in_step), L.stream_handle())
        a.bump()

    def finish_gradients(self):
        """Complete the gradient buffer before step() (fuse_reduce holds the reduce launch back until then)."""
        from . import machine
        machine.flush_pending_reduce(self.arena.grad)

    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

    def state_dict(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count,
                "param_groups": self.param_groups}

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"]); self.step_count.copy_(sd["step"])
        self.param_groups = sd["param_groups"]
        self.sync_hyper()


class MultiStepLR:
    """torch.optim.lr_scheduler.MultiStepLR for ArenaAdam (the reference's 'steplr', utils/__init__.py:43-46):
    lr = base_lr * gamma ** (number of milestones <= epoch).  `step()` is called once per epoch, as Lightning does
    with the scheduler `configure_optimizers` returns (train.py:128-131); it only writes `param_groups[0]['lr']`,
    the device copy follows at the next `sync_hyper()`."""

    def __init__(self, optimizer: ArenaAdam, milestones: Sequence[int], gamma: float = 0.1, last_epoch: int = 0):
        self.optimizer = optimizer
        self.milestones = sorted(int(m) for m in milestones)
        self.gamma = float(gamma)
        self.base_lr = float(optimizer.param_groups[0]["lr"])
        self.last_epoch = int(last_epoch)
        self._apply()

    def _apply(self):
        self.optimizer.param_groups[0]["lr"] = self.base_lr * self.gamma ** bisect_right(self.milestones, self.last_epoch)

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [self.optimizer.param_groups[0]["lr"]]

    def state_dict(self):
        return {"milestones": self.milestones, "gamma": self.gamma, "base_lr": self.base_lr,
                "last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.milestones, self.gamma = list(sd["milestones"]), float(sd["gamma"])
        self.base_lr, self.last_epoch = float(sd["base_lr"]), int(sd["last_epoch"])
        self._apply()


# ------------------------------------------------------------------------------------------------------------------
# the rest of the reference's `get_scheduler` (utils/__init__.py:43-59): 'cosine', 'poly', and the GradualWarmup wrapper
# (utils/warmup_scheduler.py) it puts around any of them when warmup_epochs > 0.  Pure host arithmetic on
# `optimizer.param_groups[0]['lr']` (any object with that attribute: ArenaAdam or a torch optimizer), stepped once per
# epoch; the device copy follows at the next `sync_hyper()`.  Pinned by tests/golden/g17_lr_schedules.npz, recorded
# from the reference's own get_scheduler (incl. what torch's chainable schedulers make of the warm-up hand-over).
# ------------------------------------------------------------------------------------------------------------------
class _EpochScheduler:
    def __init__(self, optimizer):
        self.optimizer = optimizer
        self.base_lr = float(optimizer.param_groups[0]["lr"])
        self.last_epoch = 0

    @property
    def lr(self) -> float:
        return float(self.optimizer.param_groups[0]["lr"])

    def _set(self, lr: float):
        self.optimizer.param_groups[0]["lr"] = float(lr)

    def get_lr(self) -> float:          # the chainable form: next lr from last_epoch and the CURRENT lr
        raise NotImplementedError

    def step(self):
        self.last_epoch += 1
        self._set(self.get_lr())

    def get_last_lr(self):
        return [self.lr]

    def state_dict(self):
        """Everything needed to resume mid-schedule: the scheduler's own fields, the learning rate the optimizer holds
        right now (the chainable forms compute the next rate FROM it) and — GradualWarmup — the wrapped scheduler's
        state (the reference's _LRScheduler.state_dict keeps `after_scheduler` inside its __dict__ the same way)."""
        sd = {k: v for k, v in self.__dict__.items() if k not in ("optimizer", "after")}
        sd["lr"] = self.lr
        after = getattr(self, "after", None)
        if after is not None:
            sd["after"] = after.state_dict()
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        lr, after = sd.pop("lr", None), sd.pop("after", None)
        self.__dict__.update(sd)
        if after is not None and getattr(self, "after", None) is not None:
            self.after.load_state_dict(after)
        if lr is not None:
            self._set(lr)           # the optimizer holds the restored rate, not the one it was constructed with


class StepLR(_EpochScheduler):
    """'steplr' in torch's chainable form (lr *= gamma at every milestone): what MultiStepLR above computes in closed
    form; this one can follow a warm-up that has changed the optimizer's lr."""

    def __init__(self, optimizer, milestones: Sequence[int], gamma: float = 0.1):
        super().__init__(optimizer)
        self.milestones = sorted(int(m) for m in milestones)
        self.gamma = float(gamma)

    def get_lr(self):
        return self.lr * self.gamma ** self.milestones.count(self.last_epoch)


class CosineAnnealingLR(_EpochScheduler):
    """'cosine' (utils/__init__.py:47-48: T_max = num_epochs, eta_min = 1e-8), torch's recursion."""

    def __init__(self, optimizer, T_max: int, eta_min: float = 1e-8):
        super().__init__(optimizer)
        self.T_max, self.eta_min = int(T_max), float(eta_min)

    def get_lr(self):
        import math
        e, T = self.last_epoch, self.T_max
        if (e - 1 - T) % (2 * T) == 0:
            return self.lr + (self.base_lr - self.eta_min) * (1 - math.cos(math.pi / T)) / 2
        return ((1 + math.cos(math.pi * e / T)) / (1 + math.cos(math.pi * (e - 1) / T)) * (self.lr - self.eta_min)
                + self.eta_min)


class PolyLR(_EpochScheduler):
    """'poly' as the reference states it (utils/__init__.py:49-52): lr = base_lr * (1 - epoch / num_epochs) ** poly_exp.
    Upstream raises NameError here (`LambdaLR` is never imported), so there is nothing to pin it to."""

    def __init__(self, optimizer, num_epochs: int, poly_exp: float = 0.9):
        super().__init__(optimizer)
        self.num_epochs, self.poly_exp = int(num_epochs), float(poly_exp)

    def get_lr(self):
        return self.base_lr * max(0.0, 1.0 - self.last_epoch / self.num_epochs) ** self.poly_exp


class GradualWarmup(_EpochScheduler):
    """GradualWarmupScheduler (utils/warmup_scheduler.py:4-66): lr ramps linearly from base_lr to base_lr * multiplier
    over `total_epoch` epochs, then `after` takes over with its base_lr scaled by the multiplier — including the
    hand-over epoch, where the reference asks the wrapped scheduler for a learning rate before ever stepping it."""

    def __init__(self, optimizer, multiplier: float, total_epoch: int, after: _EpochScheduler = None):
        if multiplier < 1.0:
            raise ValueError('multiplier should be greater thant or equal to 1.')
        super().__init__(optimizer)
        self.multiplier, self.total_epoch, self.after, self.finished = float(multiplier), int(total_epoch), after, False

    def get_lr(self):
        if self.last_epoch > self.total_epoch:
            if self.after is not None:
                if not self.finished:
                    self.after.base_lr = self.base_lr * self.multiplier
                    self.finished = True
                return self.after.get_lr()
            return self.base_lr * self.multiplier
        return self.base_lr * ((self.multiplier - 1.0) * self.last_epoch / self.total_epoch + 1.0)

    def step(self):
        if self.finished and self.after is not None:
            self.after.step()
        else:
            super().step()


def get_scheduler(hparams, optimizer):
    """The reference's get_scheduler (utils/__init__.py:43-59) for ArenaAdam: hparams needs `lr_scheduler` and, per
    kind, decay_step / decay_gamma | num_epochs | num_epochs / poly_exp, plus warmup_epochs / warmup_multiplier."""
    kind = hparams.lr_scheduler
    warm = getattr(hparams, "warmup_epochs", 0) > 0 and getattr(hparams, "optimizer", "adam") not in ("radam", "ranger")
    if kind == 'steplr':
        sch = (StepLR if warm else MultiStepLR)(optimizer, hparams.decay_step, hparams.decay_gamma)
    elif kind == 'cosine':
        sch = CosineAnnealingLR(optimizer, hparams.num_epochs, 1e-8)
    elif kind == 'poly':
        sch = PolyLR(optimizer, hparams.num_epochs, hparams.poly_exp)
    else:
        raise ValueError('scheduler not recognized!')
    if warm:
        sch = GradualWarmup(optimizer, hparams.warmup_multiplier, hparams.warmup_epochs, sch)
    return sch


# ------------------------------------------------------------------------------------------------------------------
# the other optimizers of the reference's get_optimizer (utils/__init__.py:23-41): torch.optim.SGD, RAdam and Ranger
# (utils/optimizers.py:6-95, 266-405), each one HIP launch over the arena (hn_sgd_step / hn_radam_step,
# csrc/hn_optim.hip).  Same protocol as ArenaAdam: `param_groups[0]` is the source of truth, `sync_hyper()` uploads it
# (as doubles: the kernels compute the schedule scalars in fp64, as the reference does in Python), the step counter
# lives on the device.  A pending reduce of the arena's gradient is completed first (no fused form for these).
# ------------------------------------------------------------------------------------------------------------------
class _ArenaOptimizer:
    _N_HYPER = 8
    _STATE = ()                 # names of the flat state tensors, in state_dict order

    def _setup(self, arena: ParamArena, group: dict, zero_grad: bool, grad_scale: float):
        L.require_gpu(arena.data)
        self.arena = arena
        self.param_groups = [group]
        self.grad_scale = float(grad_scale)        # 1 / world size when the gradients arrive SUM-all-reduced
        self.zero_grad_in_step = zero_grad
        dev = arena.data.device
        self._step_words = torch.zeros(2, dtype=torch.float32, device=dev)      # [updates done, ticket counter]
        self.step_count = self._step_words[:1]
        self.hyper = torch.zeros(self._N_HYPER, dtype=torch.float64, device=dev)
        self._uploaded = None

    def _hyper_values(self):
        raise NotImplementedError

    def sync_hyper(self) -> bool:
        """Upload the hyper-parameters if they changed since the last upload (never while a stream capture is in
        progress: a captured copy would freeze the values into the graph)."""
        vals = self._hyper_values()
        if vals == self._uploaded:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise L.HnError(f"{type(self).__name__}: hyper-parameters changed inside a stream capture; "
                            "call sync_hyper() before")
        self.hyper.copy_(torch.tensor(vals, dtype=torch.float64))
        self._uploaded = vals
        return True

    def _launch(self):
        raise NotImplementedError

    @torch.no_grad()
    def step(self):
        L.load()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        from . import machine
        machine.flush_pending_reduce(self.arena.grad)
        self._launch()
        self.arena.bump()

    def finish_gradients(self):
        from . import machine
        machine.flush_pending_reduce(self.arena.grad)

    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

    def state_tensors(self):
        """Every device tensor the optimizer's state lives in (the step counter included): what a caller saves and
        restores around warm-up runs of a graph capture (training.TrainStep)."""
        return [t for t in (getattr(self, n) for n in self._STATE) if t is not None] + [self._step_words]

    def state_dict(self):
        sd = {n: getattr(self, n) for n in self._STATE}
        sd["step"] = self.step_count
        sd["param_groups"] = self.param_groups
        return sd

    def load_state_dict(self, sd):
        for n in self._STATE:
            dst = getattr(self, n)
            if (dst is None) != (sd.get(n) is None):
                raise ValueError(f"{type(self).__name__}.load_state_dict: '{n}' present in one state but not the other")
            if dst is not None:
                dst.copy_(sd[n])
        self.step_count.copy_(sd["step"])
        self.param_groups = [dict(g) for g in sd["param_groups"]]
        self.sync_hyper()


class ArenaSGD(_ArenaOptimizer):
    """torch.optim.SGD (get_optimizer's 'sgd': momentum and weight_decay from hparams) over a ParamArena."""
    _STATE = ("momentum_buffer",)

    def __init__(self, arena: ParamArena, lr: float = 1e-3, momentum: float = 0, dampening: float = 0,
                 weight_decay: float = 0, nesterov: bool = False, zero_grad: bool = True, grad_scale: float = 1.0):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._setup(arena, {"lr": lr, "momentum": momentum, "dampening": dampening, "weight_decay": weight_decay,
                            "nesterov": bool(nesterov)}, zero_grad, grad_scale)
        # torch keeps no momentum buffer when momentum is 0: neither does this (16 B per parameter instead of 24)
        self.momentum_buffer = torch.zeros_like(arena.data) if momentum != 0 else None
        self.sync_hyper()

    def _hyper_values(self):
        g = self.param_groups[0]
        if g["momentum"] != 0 and self.momentum_buffer is None:
            raise ValueError("ArenaSGD: momentum switched on after construction with momentum 0 (no momentum buffer)")
        return (float(g["lr"]), float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"]),
                1.0 if g["nesterov"] else 0.0, float(self.grad_scale), 0.0, 0.0)

    def _launch(self):
        a = self.arena
        L.launch("hn_sgd_step", L.ptr(a.data), L.ptr(a.grad), L.ptr(self.momentum_buffer), a.numel,
                 L.ptr(self.hyper), L.ptr(self._step_words), int(self.zero_grad_in_step), L.stream_handle())


def _check_radam_args(lr, betas, eps):
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {}".format(eps))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))


class ArenaRAdam(_ArenaOptimizer):
    """The reference's RAdam (utils/optimizers.py:6-95) over a ParamArena, operation for operation: rectified update
    when N_sma >= 5, otherwise the degenerated-to-SGD update (or none at all with degenerated_to_sgd=False); decoupled
    weight decay p += (-wd*lr)*p, applied only when an update happens."""
    _N_HYPER = 12
    _STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, arena: ParamArena, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, degenerated_to_sgd: bool = True, zero_grad: bool = True,
                 grad_scale: float = 1.0):
        _check_radam_args(lr, betas, eps)
        self.degenerated_to_sgd = bool(degenerated_to_sgd)
        self._setup(arena, {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay},
                    zero_grad, grad_scale)
        self._init_state()

    def _init_state(self):
        self.exp_avg = torch.zeros_like(self.arena.data)
        self.exp_avg_sq = torch.zeros_like(self.arena.data)
        self.sync_hyper()

    def _hyper_values(self):
        g = self.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), float(self.grad_scale), 5.0, 1.0 if self.degenerated_to_sgd else 0.0,
                0.0, 0.0, 0.0, 0.0)

    def _slow(self):
        return None

    def _k(self) -> int:
        return 1

    def _launch(self):
        a = self.arena
        L.launch("hn_radam_step", L.ptr(a.data), L.ptr(a.grad), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                 L.ptr(self._slow()), a.numel, self._k(), L.ptr(self.hyper),
                 L.ptr(self._step_words), int(self.zero_grad_in_step), L.stream_handle())


class ArenaRanger(ArenaRAdam):
    """The reference's Ranger (utils/optimizers.py:266-405): RAdam with the threshold N_sma > N_sma_threshhold, weight
    decay on every step, and lookahead — the slow buffer takes the parameters before update 1, and after every update
    t with t % k == 0 moves alpha of the way to them and is copied back.  (`N_sma_threshhold`: the reference's
    spelling.)  `k` is a launch argument: a captured step keeps the k it was captured with."""
    _STATE = ("exp_avg", "exp_avg_sq", "slow_buffer")

    def __init__(self, arena: ParamArena, lr: float = 1e-3, alpha: float = 0.5, k: int = 6, N_sma_threshhold=5,
                 betas=(.95, 0.999), eps: float = 1e-5, weight_decay: float = 0, zero_grad: bool = True,
                 grad_scale: float = 1.0):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        if not lr > 0:
            raise ValueError(f'Invalid Learning Rate: {lr}')
        if not eps > 0:
            raise ValueError(f'Invalid eps: {eps}')
        self.N_sma_threshhold = N_sma_threshhold
        self._setup(arena, {"lr": lr, "alpha": alpha, "k": int(k), "step_counter": 0, "betas": tuple(betas),
                            "N_sma_threshhold": N_sma_threshhold, "eps": eps, "weight_decay": weight_decay},
                    zero_grad, grad_scale)
        self.slow_buffer = torch.zeros_like(arena.data)      # set to the parameters by update 1 (in the kernel)
        self._init_state()

    def _hyper_values(self):
        g = self.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), float(self.grad_scale), float(g["N_sma_threshhold"]), 1.0,
                float(g["alpha"]), 0.0, 0.0, 0.0)

    def _slow(self):
        return self.slow_buffer

    def _k(self) -> int:
        return int(self.param_groups[0]["k"])


# ------------------------------------------------------------------------------------------------------------------
# gradient clipping on the arena (hn_grad_norm / hn_grad_scale, csrc/hn_optim.hip): what Lightning's Trainer does with
# gradient_clip_val / gradient_clip_algorithm and the Nerfies / HyperNeRF trainers do by hand (value, then global norm),
# as two launches over `arena.grad` between backward and the optimizer's launch.
# ------------------------------------------------------------------------------------------------------------------
def check_clip_args(max_norm, clip_value, who: str = "GradClip"):
    """The host-side refusals of GradClip (and of TrainStep's clip_grad_norm / clip_grad_value), before any device work:
    returns (max_norm, clip_value) as floats or None."""
    if max_norm is None and clip_value is None:
        raise ValueError(f"{who}: give max_norm, clip_value or both")
    out = []
    for name, v in (("max_norm", max_norm), ("clip_value", clip_value)):
        if v is not None:
            v = float(v)
            if not v > 0.0:                 # NaN included
                raise ValueError(f"{who}: {name} must be positive, got {v}")
        out.append(v)
    return tuple(out)


class GradClip:
    """torch.nn.utils.clip_grad_value_(clip_value) and then torch.nn.utils.clip_grad_norm_(max_norm) (2-norm,
    error_if_nonfinite=False) over a ParamArena's gradient buffer, of the gradient that counts: grad_scale * arena.grad
    (grad_scale = 1 / world when the buffer arrives SUM-all-reduced; the optimizer's launch applies it afterwards).
    `max_norm=float('inf')` measures only.  `apply()` goes between backward and `optimizer.step()`: at most two launches,
    capturable, never a host sync; `total_norm` (before the norm clip, what clip_grad_norm_ returns) and `coef` (the
    factor applied, at most 1) are 0-dim device views the launches overwrite.  The thresholds are launch arguments,
    frozen into a captured graph: fixed at construction."""

    _WORK_FLOATS = 256 + 4          # one partial per block of the largest grid, the ticket word, padding to 16 bytes

    def __init__(self, arena: ParamArena, max_norm=None, clip_value=None, grad_scale: float = 1.0):
        self._max_norm, self._clip_value = check_clip_args(max_norm, clip_value)
        self._grad_scale = float(grad_scale)
        if not self._grad_scale > 0.0:
            raise ValueError(f"GradClip: grad_scale must be positive, got {grad_scale}")
        L.require_gpu(arena.data)
        self.arena = arena
        dev = arena.data.device
        self._work = torch.zeros(self._WORK_FLOATS, dtype=torch.float32, device=dev)    # zeroed once: the ticket re-arms itself
        self._out = torch.zeros(2, dtype=torch.float32, device=dev)
        self._out[1] = 1.0
        self.total_norm, self.coef = self._out[0], self._out[1]

    max_norm = property(lambda self: self._max_norm)
    clip_value = property(lambda self: self._clip_value)
    grad_scale = property(lambda self: self._grad_scale)

    @torch.no_grad()
    def apply(self):
        L.load()
        from . import machine
        machine.flush_pending_reduce(self.arena.grad)       # a held-back reduce launch: the buffer must be complete
        a, inf = self.arena, float("inf")
        value = inf if self._clip_value is None else self._clip_value
        if self._max_norm is not None:
            L.launch("hn_grad_norm", L.ptr(a.grad), a.numel, self._grad_scale, value,
                     self._max_norm, L.ptr(self._work), L.ptr(self._out), L.stream_handle())
        if (self._clip_value is not None and self._clip_value != inf) or (self._max_norm is not None and self._max_norm != inf):
            L.launch("hn_grad_scale", L.ptr(a.grad), a.numel, self._grad_scale, value,
                     L.ptr(self._out if self._max_norm is not None else None), L.stream_handle())


OPTIMIZERS = ("sgd", "adam", "radam", "ranger")


def make_optimizer(name: str, arena: ParamArena, lr: float, eps: float = 1e-8, weight_decay: float = 0.0,
                   momentum: float = 0.9, **kw):
    """The optimizer `name` of the reference's get_optimizer with its arguments: 'sgd' takes lr, momentum and
    weight_decay, 'adam' / 'radam' / 'ranger' lr, eps and weight_decay (everything else at the class defaults).
    `kw` (zero_grad, grad_scale) goes to the constructor."""
    if name not in OPTIMIZERS:
        raise ValueError('optimizer not recognized!')
    if name == 'sgd':
        return ArenaSGD(arena, lr=lr, momentum=momentum, weight_decay=weight_decay, **kw)
    if name == 'adam':
        return ArenaAdam(arena, lr=lr, eps=eps, weight_decay=weight_decay, **kw)
    if name == 'radam':
        return ArenaRAdam(arena, lr=lr, eps=eps, weight_decay=weight_decay, **kw)
    return ArenaRanger(arena, lr=lr, eps=eps, weight_decay=weight_decay, **kw)


def get_optimizer(hparams, arena: ParamArena, **kw):
    """The reference's get_optimizer (utils/__init__.py:23-41) on a ParamArena: hparams needs `optimizer`, `lr`,
    `weight_decay` and, for 'sgd', `momentum`.  An unknown name raises before any device work."""
    if hparams.optimizer not in OPTIMIZERS:
        raise ValueError('optimizer not recognized!')
    return make_optimizer(hparams.optimizer, arena, lr=hparams.lr, eps=1e-8, weight_decay=hparams.weight_decay,
                          momentum=getattr(hparams, "momentum", 0.9) if hparams.optimizer == 'sgd' else 0.9, **kw)
