"""Print the MLP-machine op programs a set of model configurations compiles, as JSON (no GPU needed).

    python tools/op_lists.py > ops.json

Every program's forward and backward op words (slot ids, and resolved for 4096 points in both modes) are listed per
configuration: the reference's own configurations (bench.py configs 2 / 5, the g11 model variants, the stand-alone
modules at their reference defaults).  Diffing the output of two checkouts shows whether a change touched the programs
those configurations run.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hypernerf_torch_amd import _lib as L  # noqa: E402
from hypernerf_torch_amd.hypernerf import modules, warping  # noqa: E402
from hypernerf_torch_amd.hypernerf.models import NerfModel  # noqa: E402

EMB = {"warp": list(range(100)), "camera": [0], "appearance": list(range(100)), "time": list(range(100))}

MODELS = {
    "bendy_warp": dict(hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True),
    "bendy": dict(hyper_slice_method="bendy_sheet"),
    "axis_se3": dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_warp=True,
                     use_nerf_embed=True, use_alpha_cond=True),
    "nowarp_cond": dict(hyper_slice_method="none", use_nerf_embed=True, use_alpha_cond=True),
}


def words(prog):
    out = {"fwd": prog.fwd_ops.tolist(), "bwd": prog.bwd_ops.tolist()}
    for mode in (L.HN_MODE_BF16, L.HN_MODE_F32):
        f, b = prog.resolved_ops(mode, 4096)
        out[f"resolved_{mode}"] = [f.tolist(), b.tolist()]
    return out


def words_or_error(build):
    try:
        return words(build().program)
    except Exception as e:
        return f"error: {type(e).__name__}"


def model_programs(name, kw):
    torch.manual_seed(0)
    m = NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, view_fourier_dim=6, **kw)
    if name == "axis_se3":
        m.warp_field = warping.SE3Field(in_ch=3)
    out = {}
    for level in ("coarse", "fine"):
        out[f"level_{level}"] = words_or_error(lambda: m._level_call(level))    # SE3Field: not fusable
        for n_ch in range(3, 12):       # the template's point channels: 3 + hyper dimensions
            for xyz_grad in (False, True):
                try:
                    call = m._template_call(level, n_ch, xyz_grad, False)
                except RuntimeError:
                    continue
                out[f"template_{level}_{n_ch}_{xyz_grad}"] = words(call.program)
        # the templates that gather their conditions (and axis-aligned hyper coordinates) from the GLO table: every
        # argument combination, those that do not compile recorded by what they raise
        for from_table in (False, True):
            for grad in (False, True):
                out[f"gather_{level}_{from_table}_{grad}"] = words_or_error(
                    lambda: m._template_gather_call(level, from_table, grad))
                for n_hyper in (0, 2, 4, 8):
                    out[f"reuse_{level}_{n_hyper}_{from_table}_{grad}"] = words_or_error(
                        lambda: m._template_reuse_call(level, n_hyper, from_table, grad))
    return out


def module_programs():
    torch.manual_seed(0)
    out = {}
    mods = {"MLP": modules.MLP(in_ch=16, out_ch=3), "MLP_wide_relu": modules.MLP(in_ch=16, out_ch=64,
                                                                                 output_activation=torch.nn.ReLU()),
            "NerfMLP": modules.NerfMLP(in_ch=63), "HyperSheetMLP": modules.HyperSheetMLP(),
            "TranslationField": warping.TranslationField(in_ch=3)}
    for k, mod in mods.items():
        if k.startswith("MLP"):
            out[k] = words(mod._call(True).program)
        elif k == "NerfMLP":
            out[k] = words(mod._call(False, 8, False, 39, False).program)
        else:
            out[k] = words(mod._call(True, True, True).program)
    return out


def main():
    res = {}
    for name, kw in MODELS.items():
        try:
            res[name] = model_programs(name, kw)
        except Exception as e:          # a configuration that compiles lazily elsewhere: recorded, not fatal
            res[name] = f"error: {type(e).__name__}: {e}"
    res["modules"] = module_programs()
    json.dump(res, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
