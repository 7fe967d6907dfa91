"""The lean ReLU-only builds of the MLP machine kernels against the generic ones, bit for bit, on the MI355X.

tests/lean_cases.py runs in two fresh child processes (the switch HN_FORCE_GENERIC is read when machine.py is imported),
once with the lean builds and once forced onto the generic kernels, on the same seeded inputs:
  warp128   TranslationField: encoder first layer, four plain 128 -> 128 ReLU layers (the lean backward's pipelined
            body), a skip layer and the head (the generic tile loop) in one program
  sheet64   HyperSheetMLP: the 64-wide chain
  model     the fused config-2 level programs, coarse and fine, GLO rows gathered inside the machine
  leaky128  TranslationField with LeakyReLU layers: announces no ReLU-only program, runs the generic kernels either way
each at 33 points (one full and one partly filled block, the other waves idle) and at 288 points as 9 rays x 32 samples
(two workgroup tiles, a second ws.start()).  Forward outputs, source gradients, every weight and bias gradient and the
GLO tables' gradients must agree byte for byte.

The generic kernels themselves are the parent commit's, instruction for instruction (test_lean_builds.py holds their
code sizes and registers), and on the day the lean builds were added all of these arrays, leaky128 included, were
byte-identical between the parent commit's library and this one's (profiles/r07_lean_builds.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean_cases")
    out = {}
    for label, force in (("lean", "0"), ("generic", "1")):
        path = str(d / f"{label}.npz")
        res = subprocess.run([sys.executable, os.path.join(HERE, "lean_cases.py"), path], capture_output=True, text=True,
                             env=dict(os.environ, HN_FORCE_GENERIC=force), timeout=300)
        assert res.returncode == 0, (label, res.stderr[-3000:])
        out[label] = dict(np.load(path))
    return out


CASES = [f"{tag}/n{n}" for tag in ("warp128", "sheet64", "model", "leaky128") for n in (33, 288)]


def test_the_two_runs_took_the_builds_they_should(runs):
    for case in CASES:
        lean, generic = runs["lean"][case + "/relu_only_bit"], runs["generic"][case + "/relu_only_bit"]
        assert (generic == 0).all(), case                      # forced: every launch on the generic kernels
        assert (lean == (0 if case.startswith("leaky128") else 4)).all(), (case, lean)
    # the shapes the cases are about: hidden layers of 128 (four of them plain, behind the encoder layer) and of 64
    assert list(runs["lean"]["warp128/n288/widths"]) == [128] * 6 + [32]
    assert list(runs["lean"]["sheet64/n288/widths"]) == [64] * 6 + [32]


@pytest.mark.parametrize("case", CASES)
def test_lean_and_generic_builds_agree_bit_for_bit(runs, case):
    lean = {k: v for k, v in runs["lean"].items() if k.startswith(case + "/") and not k.endswith("relu_only_bit")}
    generic = {k: v for k, v in runs["generic"].items() if k.startswith(case + "/") and not k.endswith("relu_only_bit")}
    assert sorted(lean) == sorted(generic) and len(lean) >= 5
    grads = [k for k in lean if "/grad/" in k]
    assert any(k.endswith("weight") for k in grads) and any(k.endswith("bias") for k in grads)
    if case.startswith("model"):
        assert case + "/grad/warp_embed.embed.weight" in lean and case + "/coarse/rgb" in lean and case + "/fine/rgb" in lean
        assert np.abs(lean[case + "/grad/warp_embed.embed.weight"]).max() > 0        # the GLO table's gradient is there
    else:
        assert {case + "/y", case + "/dpts", case + "/demb"} <= set(lean)
        assert np.abs(lean[case + "/dpts"]).max() > 0 and np.abs(lean[case + "/demb"]).max() > 0
    for k in sorted(lean):
        assert np.isfinite(lean[k]).all(), k
        assert lean[k].dtype == generic[k].dtype and lean[k].shape == generic[k].shape, k
        assert lean[k].tobytes() == generic[k].tobytes(), (k, float(np.abs(lean[k].astype(np.float64) - generic[k]).max()))
