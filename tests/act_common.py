"""Shared helpers of the activation tests (test_mlp_activations.py, test_gpu_activations.py): the g18 fixture, the
activation modules it records, a plain torch CPU restatement of modules.MLP and the reference's gradient summaries."""
import os

import numpy as np
import torch

import hashprng as H

nn = torch.nn
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_activations.npz")

# the activations g18 records (tests/golden/make_act_golden.py)
ACTS = {
    "leaky_def": lambda: nn.LeakyReLU(),
    "leaky": lambda: nn.LeakyReLU(0.2),
    "elu_def": lambda: nn.ELU(),
    "elu": lambda: nn.ELU(0.7),
    "sp_def": lambda: nn.Softplus(),
    "sp": lambda: nn.Softplus(beta=2, threshold=5),
}
MLP_HIDDEN = dict(in_ch=20, out_ch=3, depth=4, width=64, skips=[2])
MLP_WIDE = dict(in_ch=20, out_ch=40, depth=2, width=64, skips=[])


def golden():
    return np.load(GOLDEN)


def mlp_kwargs(kind, act_name):
    kw = dict(MLP_HIDDEN if kind == "hidden" else MLP_WIDE)
    kw["hidden_activation" if kind == "hidden" else "output_activation"] = ACTS[act_name]()
    return kw


def load_mlp_weights(m, seed=18):
    """The fixture's weights: hashed state dict, linears.0.bias zeroed (make_act_golden.prepare_mlp)."""
    sd = m.state_dict()
    new = H.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed)
    new["linears.0.bias"] = torch.zeros_like(new["linears.0.bias"])
    m.load_state_dict(new)
    return new


def mlp_restated(sd, x, depth, skips, hidden_act, out_act):
    """modules.MLP.forward (reference hypernerf/modules.py:116-127) in plain torch: Linear + activation, the input
    re-appended after every layer in `skips`, then the logit layer and the output activation."""
    h = x
    for i in range(max(depth, 1)):
        h = hidden_act(torch.nn.functional.linear(h, sd[f"linears.{i}.weight"], sd[f"linears.{i}.bias"]))
        if i in skips:
            h = torch.cat([h, x], -1)
    y = torch.nn.functional.linear(h, sd["logit_layer.weight"], sd["logit_layer.bias"])
    return out_act(y) if out_act is not None else y


def grad_stats_close(named_grads, g, prefix, tol):
    """Compare gradients with the reference's summaries (sum / abs-sum / L2 + 16 sampled entries)."""
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
