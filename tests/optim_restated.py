"""Test infrastructure: the update rules of the reference's SGD (torch.optim.SGD), RAdam and Ranger
(utils/optimizers.py:29-95, 322-405) restated in a few lines of torch on the CPU.  Schedule scalars (beta^t, N_sma, the
step size and its products with lr) are Python doubles, as in the reference; tensor arithmetic is fp32, in the
reference's order.  tests/test_optim_host.py pins this restatement to the reference's own trajectories
(tests/golden/g20_optimizers.npz); the GPU tests use it where a live reference is needed (ragged buffers, a training run).
"""
import math

import torch


class Restated:
    """One optimizer over a list of fp32 tensors: `step(params, grads)` updates `params` in place.
    kind: 'sgd' (lr, momentum, dampening, weight_decay, nesterov), 'radam' (lr, betas, eps, weight_decay,
    degenerated_to_sgd) or 'ranger' (lr, alpha, k, N_sma_threshhold, betas, eps, weight_decay), the classes' defaults."""

    DEFAULTS = {
        "sgd": dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
        "radam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, degenerated_to_sgd=True),
        "ranger": dict(lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0.0),
    }

    def __init__(self, kind, **kw):
        self.kind = kind
        self.h = dict(self.DEFAULTS[kind], **kw)
        self.t = 0
        self.state = None

    @torch.no_grad()
    def step(self, params, grads):
        if self.state is None:
            self.state = [{} for _ in params]
        self.t += 1
        for p, g, st in zip(params, grads, self.state):
            getattr(self, "_" + self.kind)(p, g.float(), st)

    def _sgd(self, p, g, st):
        h = self.h
        d = g.clone()
        if h["weight_decay"] != 0:
            d = d.add(p, alpha=h["weight_decay"])
        if h["momentum"] != 0:
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = d.clone()
            else:
                st["momentum_buffer"].mul_(h["momentum"]).add_(d, alpha=1 - h["dampening"])
            d = d.add(st["momentum_buffer"], alpha=h["momentum"]) if h["nesterov"] else st["momentum_buffer"]
        p.add_(d, alpha=-h["lr"])

    def _schedule(self, rectified):
        h, t = self.h, self.t
        beta1, beta2 = h["betas"]
        beta2_t = beta2 ** t
        n_sma_max = 2 / (1 - beta2) - 1
        n_sma = n_sma_max - 2 * t * beta2_t / (1 - beta2_t)
        if rectified(n_sma):
            return True, math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max
                                   / (n_sma_max - 2)) / (1 - beta1 ** t)
        if self.kind == "ranger" or h["degenerated_to_sgd"]:
            return False, 1.0 / (1 - beta1 ** t)
        return False, -1.0

    def _moments(self, p, g, st):
        beta1, beta2 = self.h["betas"]
        if "exp_avg" not in st:
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
        st["exp_avg_sq"].mul_(beta2).addcmul_(g, g, value=1 - beta2)
        st["exp_avg"].mul_(beta1).add_(g, alpha=1 - beta1)
        return st["exp_avg"], st["exp_avg_sq"]

    def _radam(self, p, g, st):
        h = self.h
        m, v = self._moments(p, g, st)
        rect, step_size = self._schedule(lambda n: n >= 5)
        if rect or step_size > 0:
            if h["weight_decay"] != 0:
                p.add_(p, alpha=-h["weight_decay"] * h["lr"])
            if rect:
                p.addcdiv_(m, v.sqrt().add_(h["eps"]), value=-step_size * h["lr"])
            else:
                p.add_(m, alpha=-step_size * h["lr"])

    def _ranger(self, p, g, st):
        h = self.h
        if "slow_buffer" not in st:
            st["slow_buffer"] = p.clone()
        m, v = self._moments(p, g, st)
        rect, step_size = self._schedule(lambda n: n > h["N_sma_threshhold"])
        if h["weight_decay"] != 0:
            p.add_(p, alpha=-h["weight_decay"] * h["lr"])
        if rect:
            p.addcdiv_(m, v.sqrt().add_(h["eps"]), value=-step_size * h["lr"])
        else:
            p.add_(m, alpha=-step_size * h["lr"])
        if self.t % h["k"] == 0:
            slow = st["slow_buffer"]
            slow.add_(p - slow, alpha=h["alpha"])
            p.copy_(slow)

    def flat_state(self, name):
        """State tensor `name` of every parameter, flattened and concatenated (None where the optimizer keeps none)."""
        if not self.state or name not in self.state[0]:
            return None
        return torch.cat([st[name].reshape(-1) for st in self.state])


def g20_inputs(shapes, seed, steps):
    """Initial parameters and the gradient of every update of tests/golden/g20_optimizers.npz, from tests/hashprng.py:
    (list of parameters, [list of gradients per update])."""
    import hashprng as H
    params = [H.uniform(seed, f"p{i}", tuple(s), -1.0, 1.0) for i, s in enumerate(shapes)]
    grads = [[H.normal(seed, f"g{i}/{t}", tuple(s)) * (0.5 + 0.1 * t) for i, s in enumerate(shapes)]
             for t in range(steps)]
    return params, grads
