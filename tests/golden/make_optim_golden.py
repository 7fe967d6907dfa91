#!/usr/bin/env python3
"""Golden optimizer trajectories from the REFERENCE's own `utils.get_optimizer` (utils/__init__.py:23-41) and its
RAdam / Ranger classes (utils/optimizers.py:6-95, 266-405), build container only:

    python tests/golden/make_optim_golden.py        -> tests/golden/g20_optimizers.npz

A handful of parameter tensors of odd sizes (several lengths not a multiple of 4) start from hash-PRNG values and take
STEPS updates with hash-PRNG gradients (tests/optim_restated.py: g20_inputs), so the fixture stores trajectories only:
the parameters after every update ('<case>/params', (STEPS, N), the tensors flattened and concatenated) and the final
optimizer state ('<case>/<exp_avg | exp_avg_sq | slow_buffer | momentum_buffer>', (N,)).  'cases' (JSON) holds, per
case, the arena optimizer and keywords that state the same optimizer.  14 updates cross RAdam's N_sma threshold
(t = 6 at beta2 = 0.999) and, at k = 6, two of Ranger's lookahead syncs.
Written with fixed zip timestamps, so that a regeneration is byte-identical.  Import shims as in make_lr_golden.py."""
import io
import json
import os
import sys
import types
import warnings
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))          # tests/ (hashprng, optim_restated)

import numpy as np
import torch

from optim_restated import g20_inputs


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


tv = _stub("torchvision")
tv.transforms = _stub("torchvision.transforms")
_stub("cv2", COLORMAP_JET=2)
pil = _stub("PIL")
pil.Image = _stub("PIL.Image")
sys.path.insert(0, REF)
import utils as R_utils            # noqa: E402
from utils import optimizers as R_opt  # noqa: E402

SEED = 20
STEPS = 14
SHAPES = [(9, 7), (31,), (5, 3, 2), (12, 25), (1,), (13, 11)]

# name: (how the reference builds it, its arguments, the arena class, the arena keywords)
CASES = {
    "sgd_m09": ("get_optimizer", dict(optimizer="sgd", lr=0.05, momentum=0.9, weight_decay=0.0),
                "ArenaSGD", dict(lr=0.05, momentum=0.9, weight_decay=0.0)),
    "sgd_m09_wd": ("get_optimizer", dict(optimizer="sgd", lr=0.05, momentum=0.9, weight_decay=1e-2),
                   "ArenaSGD", dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
    "sgd_m0": ("get_optimizer", dict(optimizer="sgd", lr=0.05, momentum=0.0, weight_decay=0.0),
               "ArenaSGD", dict(lr=0.05, momentum=0.0, weight_decay=0.0)),
    "adam": ("get_optimizer", dict(optimizer="adam", lr=1e-2, momentum=0.9, weight_decay=0.0),
             "ArenaAdam", dict(lr=1e-2, eps=1e-8, weight_decay=0.0)),
    "radam": ("get_optimizer", dict(optimizer="radam", lr=1e-2, momentum=0.9, weight_decay=0.0),
              "ArenaRAdam", dict(lr=1e-2, eps=1e-8, weight_decay=0.0)),
    "radam_wd": ("get_optimizer", dict(optimizer="radam", lr=1e-2, momentum=0.9, weight_decay=1e-2),
                 "ArenaRAdam", dict(lr=1e-2, eps=1e-8, weight_decay=1e-2)),
    "radam_nodegen": ("RAdam", dict(lr=1e-2, degenerated_to_sgd=False),
                      "ArenaRAdam", dict(lr=1e-2, degenerated_to_sgd=False)),
    "radam_b099": ("RAdam", dict(lr=1e-2, betas=(0.9, 0.99)),
                   "ArenaRAdam", dict(lr=1e-2, betas=(0.9, 0.99))),
    "ranger": ("get_optimizer", dict(optimizer="ranger", lr=1e-2, momentum=0.9, weight_decay=0.0),
               "ArenaRanger", dict(lr=1e-2, eps=1e-8, weight_decay=0.0)),
    "ranger_wd": ("get_optimizer", dict(optimizer="ranger", lr=1e-2, momentum=0.9, weight_decay=1e-2),
                  "ArenaRanger", dict(lr=1e-2, eps=1e-8, weight_decay=1e-2)),
    "ranger_k3": ("Ranger", dict(lr=1e-2, k=3, alpha=0.8),
                  "ArenaRanger", dict(lr=1e-2, k=3, alpha=0.8)),
}
STATE_NAMES = ("exp_avg", "exp_avg_sq", "slow_buffer", "momentum_buffer")


def _reference_optimizer(how, args, params):
    if how == "get_optimizer":
        return R_utils.get_optimizer(types.SimpleNamespace(**args), torch.nn.ParameterList(params))
    return getattr(R_opt, how)(params, **args)


def record(name):
    how, args, _, _ = CASES[name]
    init, grads = g20_inputs(SHAPES, SEED, STEPS)
    params = [torch.nn.Parameter(p.clone()) for p in init]
    opt = _reference_optimizer(how, args, params)
    traj = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the reference's deprecated add_(scalar, tensor) overloads
        for t in range(STEPS):
            for p, g in zip(params, grads[t]):
                p.grad = g.clone()
            opt.step()
            traj.append(torch.cat([p.detach().reshape(-1) for p in params]))
    out = {f"{name}/params": torch.stack(traj).numpy()}
    for s in STATE_NAMES:
        st = [opt.state[p].get(s) for p in params]
        if st[0] is not None:
            out[f"{name}/{s}"] = torch.cat([x.reshape(-1) for x in st]).numpy()
    return out


def save_npz(path, arrays):
    """np.savez with a fixed timestamp on every member (np.savez stamps the current time: not reproducible)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    out = {}
    for name in CASES:
        out.update(record(name))
        p = out[f"{name}/params"]
        print(f"{name:14s} |p_final - p_0| max {np.abs(p[-1] - p[0]).max():.4f}")
    meta = {"seed": SEED, "steps": STEPS, "shapes": SHAPES,
            "cases": {k: {"reference": v[0], "reference_args": v[1], "cls": v[2], "kw": v[3]} for k, v in CASES.items()}}
    out["meta"] = np.asarray(json.dumps(meta, sort_keys=True))
    save_npz(os.path.join(HERE, "g20_optimizers.npz"), out)


if __name__ == "__main__":
    main()
