"""The lean ReLU-only builds of the MLP machine kernels, without a GPU: hipcc's resource report and assembly for
hn_mlp.hip (one gfx950 cross-compile per session), and which programs machine.py announces as ReLU-only
(HnMlpArgs.wide_ops bit 2)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import machine as M
from hypernerf_torch_amd.hypernerf import models, warping

ARGS = "Ev9HnMlpArgs"
LEAN_FWD = ["_Z22hn_mlp_fwd_relu_kernelILi2ELb1ELb1ELb0ELb0ELb0E" + ARGS,       # <AUXG 2, training>
            "_Z22hn_mlp_fwd_relu_kernelILi2ELb0ELb1ELb0ELb0ELb0E" + ARGS,       # <AUXG 2, inference>
            "_Z22hn_mlp_fwd_relu_kernelILi3ELb1ELb1ELb0ELb0ELb0E" + ARGS]       # <AUXG 3, training>
LEAN_BWD = "_Z22hn_mlp_bwd_relu_kernelILb1ELb0ELb0ELb0E" + ARGS
# (VGPRs, scratch bytes per lane, waves per SIMD, code bytes) of the kernels test_host_api pins by name, as hipcc reports
# them for the commit before the lean builds existed: the generic kernels are to come out of this one unchanged
PARENT = {
    "_Z17hn_mlp_fwd_kernelILb1ELi2ELb0ELb1ELb0E" + ARGS: (233, 0, 2, 60312),
    "_Z17hn_mlp_fwd_kernelILb1ELi3ELb0ELb1ELb0E" + ARGS: (249, 0, 2, 67892),
    "_Z17hn_mlp_fwd_kernelILb1ELi2ELb0ELb0ELb0E" + ARGS: (254, 0, 2, 54464),
    "_Z17hn_mlp_fwd_kernelILb1ELi3ELb0ELb0ELb0E" + ARGS: (256, 44, 2, 62280),
    "_Z17hn_mlp_fwd_kernelILb1ELi2ELb1ELb1ELb0E" + ARGS: (256, 8, 2, 88548),
    "_Z17hn_mlp_fwd_kernelILb1ELi3ELb1ELb1ELb0E" + ARGS: (256, 92, 2, 108388),
    "_Z17hn_mlp_bwd_kernelILb1ELb0ELb0E" + ARGS: (230, 0, 2, 68788),
    "_Z17hn_mlp_bwd_kernelILb1ELb1ELb0E" + ARGS: (256, 152, 2, 106692),
    "_Z17hn_mlp_fwd_kernelILb1ELi2ELb0ELb1ELb1E" + ARGS: (235, 0, 2, 61916),
    "_Z17hn_mlp_fwd_kernelILb1ELi3ELb0ELb1ELb1E" + ARGS: (251, 0, 2, 69820),
    "_Z17hn_mlp_bwd_kernelILb1ELb0ELb1E" + ARGS: (231, 0, 2, 56044),
    "_Z15hn_wgrad_kernelILb1ELb0EEv14HnDwBatchTable": (199, 0, 2, 23440),
    "_Z15hn_wgrad_kernelILb1ELb1EEv14HnDwBatchTable": (186, 0, 2, 27260),
    "_Z15hn_wgrad_kernelILb0ELb0EEv14HnDwBatchTable": (188, 0, 2, 23496),
}


@pytest.fixture(scope="session")
def compiled(tmp_path_factory):
    """{kernel: {"VGPRs", "scratch", "occupancy", "code", "asm"}} of hn_mlp.hip, flags as the product build's."""
    asm_path = str(tmp_path_factory.mktemp("lean") / "hn_mlp.s")
    cmd = [L.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics", "-S",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", asm_path, os.path.join(L.CSRC, "hn_mlp.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    info, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = info.setdefault(m.group(1), {})
        for key, short in (("VGPRs", "VGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy")):
            m2 = re.search(re.escape(key) + r": (\d+)", line)
            if m2 and cur is not None and "AGPR" not in line.split(key)[0][-3:] and "Spill" not in line:
                cur[short] = int(m2.group(1))
    name, body = None, []
    with open(asm_path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):", line)
            if m and m.group(1) in info:
                name, body = m.group(1), []
                info[name]["asm"] = body
            elif name is not None:
                body.append(line)
                m = re.search(r"; codeLenInByte = (\d+)", line)
                if m:
                    info[name]["code"] = int(m.group(1))
                    name = None
    return info


def test_lean_entries_fit_two_waves_without_scratch(compiled):
    for name in LEAN_FWD + [LEAN_BWD]:
        assert name in compiled, sorted(k for k in compiled if "relu" in k)
        k = compiled[name]
        assert k["VGPRs"] <= 256 and k["occupancy"] == 2 and k["scratch"] == 0, (name, k["VGPRs"], k["occupancy"], k["scratch"])
    # the lean backward is back under the 64 KB instruction cache two CUs share
    assert compiled[LEAN_BWD]["code"] < 65536, compiled[LEAN_BWD]["code"]
    siblings = ("_Z17hn_mlp_fwd_kernelILb1ELi2ELb0ELb1ELb0E", "_Z17hn_mlp_fwd_kernelILb1ELi2ELb0ELb0ELb0E", "_Z17hn_mlp_fwd_kernelILb1ELi3ELb0ELb1ELb0E")
    for name, sibling in zip(LEAN_FWD, siblings):           # and every lean forward is smaller than its generic sibling
        assert compiled[name]["code"] < compiled[sibling + ARGS]["code"], (name, sibling)
    assert compiled[LEAN_BWD]["code"] < compiled["_Z17hn_mlp_bwd_kernelILb1ELb0ELb0E" + ARGS]["code"]


def test_lean_builds_hold_no_activation_code(compiled):
    """None of hn_act_tile / hn_dact_y / the read-back of the layer output: no v_exp_f32 / v_log_f32 in the lean
    backward, no v_log_f32 (Softplus) in the lean forwards (their v_exp_f32 is the sigmoid of the OUT op), and no call
    anywhere — the helpers are forced inline, so a call would be one that escaped."""
    bwd = "".join(compiled[LEAN_BWD]["asm"])
    assert "v_exp_f32" not in bwd and "v_log_f32" not in bwd
    generic = "".join(compiled["_Z17hn_mlp_bwd_kernelILb1ELb0ELb0E" + ARGS]["asm"])
    assert "v_exp_f32" in generic          # what the check looks for is really what Softplus' derivative compiles to
    for name in LEAN_FWD + [LEAN_BWD]:
        asm = "".join(compiled[name]["asm"])
        assert "v_log_f32" not in asm and "s_swappc_b64" not in asm and "s_call_b64" not in asm, name
    assert "v_log_f32" in "".join(compiled["_Z17hn_mlp_fwd_kernelILb1ELi2ELb0ELb1ELb0E" + ARGS]["asm"])


def test_generic_kernels_are_those_of_the_parent_commit(compiled):
    for name, want in PARENT.items():
        assert name in compiled, name
        k = compiled[name]
        assert (k["VGPRs"], k["scratch"], k["occupancy"], k["code"]) == want, (name, k["VGPRs"], k["scratch"], k["occupancy"], k["code"])


def _config2_model():
    from gpu_common import EMB
    return models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, hyper_slice_method="bendy_sheet",
                            use_nerf_embed=True, use_alpha_cond=True)


def _programs():
    m = _config2_model()
    reuse = m._template_reuse_call("fine", m.hyper_sheet_out_dim, False, True).program
    assert reuse.name == "template_fine_reuse"
    relu = {"coarse level": m._level_call("coarse").program, "fine level": m._level_call("fine").program,
            "template_fine_reuse": reuse, "SE3 field": warping.SE3Field(in_ch=3)._field_call(True).program}
    leaky = warping.TranslationField(in_ch=3, in_ch_embed=8, activation=torch.nn.LeakyReLU(0.2))._call(False, True, True).program
    return relu, leaky


def test_relu_only_bit_follows_the_layers(monkeypatch):
    monkeypatch.setattr(M, "FORCE_GENERIC", False)
    relu, leaky = _programs()
    for name, prog in relu.items():
        assert all(ly.act in ("none", "relu") for ly in prog.layers), name
        assert prog.relu_only_bit() == 4, name
    assert sum(ly.act == "leaky_relu" for ly in leaky.layers) >= 1
    assert leaky.relu_only_bit() == 0
    one = warping.TranslationField(in_ch=3, in_ch_embed=8)._call(False, True, True).program      # one LeakyReLU layer among ReLUs
    assert one.relu_only_bit() == 4
    one.layers[2].act, one.layers[2].act_params = "leaky_relu", (0.2, 0.0)
    assert one.relu_only_bit() == 0


def test_force_generic_clears_the_bit(monkeypatch):
    monkeypatch.setattr(M, "FORCE_GENERIC", True)
    relu, leaky = _programs()
    assert [p.relu_only_bit() for p in relu.values()] == [0] * len(relu) and leaky.relu_only_bit() == 0
    # and the switch is the environment variable HN_FORCE_GENERIC, read when machine.py is imported
    code = "from hypernerf_torch_amd import machine as M; print(int(M.FORCE_GENERIC))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root,
                         env=dict(os.environ, HN_FORCE_GENERIC="1"), timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "1", (res.stdout, res.stderr[-500:])
