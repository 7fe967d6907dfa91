"""The exactly representable MLP cases (tests/exact_mlp.py) checked WITHOUT a GPU: every listed case meets the exactness
conditions under both ReLU-at-zero rules, its hand-written float64 reference equals torch autograd in float64 on a plain
torch.nn.functional restatement, the list covers the table of shapes it promises, and every case compiles on the host."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import exact_mlp as X
import hypernerf_torch_amd  # noqa: F401
from hypernerf_torch_amd import _lib as L

NAMES = [c.name for c in X.ALL_CASES]


class _ReluKeepZero(torch.autograd.Function):
    """ReLU whose gradient is kept where the sign bit of z is clear (z >= 0): the bf16 mode's rule, hn_push_mask."""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return z.clamp_min(0.0)

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        return torch.where(z >= 0, g, torch.zeros_like(g))


def _act(z, kind, rule):
    if kind == "relu":
        return _ReluKeepZero.apply(z) if rule else torch.relu(z)
    if kind == "leaky":
        return TF.leaky_relu(z, X.SLOPE)
    return z


def _mlp(p, prefix, inp, n_hidden, skips, hidden, out_act, rule):
    h = inp
    for i in range(n_hidden):
        h = _act(TF.linear(h, p[f"{prefix}linears.{i}.weight"], p[f"{prefix}linears.{i}.bias"]), hidden, rule)
        if i in skips:
            h = torch.cat([h, inp], dim=-1)
    return _act(TF.linear(h, p[f"{prefix}logit_layer.weight"], p[f"{prefix}logit_layer.bias"]), out_act, rule)


def _torch_reference(case, rule):
    """The case through torch autograd in float64: {name: array} of outputs and gradients."""
    spec = case["spec"]
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in case["state"].items()}
    leaf = lambda a: torch.from_numpy(a).double().requires_grad_(True)      # noqa: E731
    if isinstance(spec, X.NerfSpec):
        x, ac, rc = leaf(case["x"]), leaf(case["ac"]), leaf(case["rc"])
        t = _mlp(p, "trunk_mlp.", x, spec.trunk_depth, spec.skips, "relu", "relu", rule)
        bn = TF.linear(t, p["bottleneck_mlp.weight"], p["bottleneck_mlp.bias"])
        rep = lambda c: c[:, None, :].expand(-1, spec.s, -1)                  # noqa: E731
        alpha = TF.linear(torch.cat([bn, rep(ac)], -1), p["alpha_mlp.weight"], p["alpha_mlp.bias"])
        rgb = _mlp(p, "rgb_mlp.", torch.cat([bn, rep(rc)], -1), spec.rgb_depth, (), "relu", "none", rule)
        ((rgb * torch.from_numpy(case["d_rgb"]).double()).sum()
         + (alpha * torch.from_numpy(case["d_alpha"]).double()).sum()).backward()
        out = {"rgb": rgb, "alpha": alpha, "dx": x.grad, "d_ac": ac.grad, "d_rc": rc.grad}
    else:
        x = leaf(case["x"])
        y = _mlp(p, "", x, spec.n_hidden, spec.skips, spec.hidden, spec.out_act, rule)
        (y * torch.from_numpy(case["dY"]).double()).sum().backward()
        out = {"y": y, "dx": x.grad}
    out = {k: v.detach().numpy() for k, v in out.items()}
    out["grads"] = {k: v.grad.numpy() for k, v in p.items()}
    return out


@pytest.mark.parametrize("name", NAMES)
def test_listed_case_is_exact_under_both_relu_rules(name):
    for rule in (0, 1):
        bad = X.check_exact(X.reference_of(name, rule))
        assert not bad, (name, rule, bad)


def test_check_exact_sees_what_it_should():
    """The conditions are not vacuous: an operand of 257 (9 significant bits), a -0.0 and a sum past 2^24 are reported."""
    base = {"operands": {"a": np.array([[256.0, 3.0]])}, "outputs": ("y",), "y": np.array([[1.0]]), "grads": {},
            "sums": {"w": (np.ones((4, 1)), np.ones((4, 1)))}}
    assert X.check_exact(base) == []
    assert any("not bfloat16" in b for b in X.check_exact(dict(base, operands={"a": np.array([[257.0]])})))
    assert any("-0.0" in b for b in X.check_exact(dict(base, y=np.array([[-0.0]]))))
    assert any("2^24" in b for b in X.check_exact(dict(base, sums={"w": (np.full((4, 1), 4096.0), np.full((4, 1), 1024.0))})))
    assert any("2^24" in b for b in X.check_exact(dict(base, sums={"w": (np.full((4, 1), 2048.5), np.full((4, 1), 1024.0))})))
    assert any("not float32" in b for b in X.check_exact(dict(base, grads={"g": np.array([2.0 ** 24 + 1])})))


def test_locate_names_elements_and_tiles():
    want = np.zeros((70, 100), np.float32)
    got = want.copy()
    got[33, 64:70] = 1.0
    got[69, 99] = np.nan
    msg = X.locate(got, want)
    assert msg.startswith("7 of 7000 elements differ") and "(33, 64): got 1.0 want 0.0" in msg
    assert "(1, 2): 6, (2, 3): 1" in msg and "[2 of 12 tiles]" in msg
    assert X.locate(want, want) == "identical"
    assert "(0, 1): 1" in X.locate(np.arange(40.0), np.where(np.arange(40) == 35, -1.0, np.arange(40.0)))   # a bias vector
    assert "(0, 0): 3, (1, 0): 3" in X.locate(np.ones((2, 20, 3)), np.concatenate([np.ones((2, 19, 3)), np.zeros((2, 1, 3))], 1))
    assert X.locate(np.zeros(3), np.zeros(4)).startswith("shape")


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_torch_autograd_in_float64(name):
    """Rule 0 is torch's own ReLU; rule 1 is restated with a ReLU that keeps the gradient at z == 0.  A case without
    exact zeros gives the same gradients under both, and both are compared with torch's own rule."""
    case = X.case_of(name)
    for rule in (0, 1):
        ref = X.reference_of(name, rule)
        rules = (0, 1) if ref["zero_hits"] + ref["zero_hits_out"] == 0 else (rule,)
        for torch_rule in rules:
            want = _torch_reference(case, torch_rule)
            keys = [k for k in want if k != "grads"]
            for k in keys:
                np.testing.assert_allclose(ref[k], want[k], rtol=1e-12, atol=1e-12, err_msg=f"{name} rule {rule} {k}")
            assert set(ref["grads"]) == set(want["grads"])
            for k, g in want["grads"].items():
                np.testing.assert_allclose(ref["grads"][k], g, rtol=1e-12, atol=1e-12, err_msg=f"{name} rule {rule} d {k}")


def test_the_zero_case_has_relu_units_at_exactly_zero_with_a_gradient_arriving():
    """The bf16 convention (a +0 pre-activation keeps its gradient) is pinned, not dodged: in ZERO_CASE the two rules
    give different gradients."""
    r0, r1 = X.reference_of(X.ZERO_CASE, 0), X.reference_of(X.ZERO_CASE, 1)
    assert r0["zero_hits"] > 0 and r1["zero_hits"] > 0
    assert np.array_equal(r0["y"], r1["y"])
    differing = [k for k in r0["grads"] if not np.array_equal(r0["grads"][k], r1["grads"][k])]
    assert "linears.0.weight" in differing and "linears.0.bias" in differing, differing
    assert not np.array_equal(r0["dx"], r1["dx"])


def test_case_list_covers_the_table():
    specs = X.MLP_CASES
    assert len(specs) >= 32 and len(set(NAMES)) == len(NAMES)
    have = lambda f: {f(s) for s in specs}                                   # noqa: E731
    assert have(lambda s: s.width) >= {8, 24, 32, 53, 64, 96, 128, 160, 200, 256}
    assert any(s.width == 128 and s.depth >= 3 and s.hidden == "relu" for s in specs)      # the pipelined 128 -> 128 body
    assert have(lambda s: s.depth) >= {0, 1, 2, 4, 8}
    assert have(lambda s: s.skips) >= {(), (0,), (1, 3)}
    assert have(lambda s: s.in_ch) >= {1, 3, 20, 33, 64, 71, 190}
    assert have(lambda s: s.out_ch) >= {1, 3, 4, 5, 8, 17, 32, 40}
    assert have(lambda s: s.out_act) == {"none", "relu"}
    assert have(lambda s: s.hidden) == {"relu", "leaky"}
    assert all(s.depth <= 3 for s in specs if s.hidden == "leaky")
    assert have(lambda s: s.n) >= {1, 31, 32, 33, 255, 256, 257, 700, X.N_PAST_CAP}
    dense = [s for s in specs if s.first_nnz == 0]
    assert len(dense) >= 6 and {190, 64} <= {s.in_ch for s in dense}
    assert any(s.hidden_nnz == 0 and s.depth <= 2 for s in specs)
    for s in specs:
        assert all(0 <= i < s.n_hidden - 1 for i in s.skips), s.name
        assert s.out_act == "none" or s.out_ch > 4, s.name      # a ReLU output is a wide output
    assert sum(s.arena for s in X.ALL_CASES) >= 2
    assert {(c.b, c.s) for c in X.NERF_CASES} == {(7, 9), (33, 32)}
    for c in X.NERF_CASES:
        assert (c.trunk_width, c.trunk_depth, c.alpha_cond, c.rgb_cond) == (256, 8, 8, 12) and c.skips


def test_past_the_cap_case_matches_the_constants_of_the_source():
    """N_PAST_CAP = the persistent-loop cap of hn_grid_for x the points of a bf16 workgroup, one more full tile, 37 points."""
    with open(os.path.join(L.CSRC, "hn_mlp.hip")) as f:
        src = f.read()
    body = src[src.index("static int hn_grid_for("):]
    m = re.search(r"const int cap = (\d+) \* (\d+);", body[:body.index("}")])
    assert m and int(m.group(1)) * int(m.group(2)) == X.GRID_CAP
    with open(os.path.join(L.CSRC, "hn_common.h")) as f:
        m = re.search(r"#define HN_BF16_WAVES (\d+)", f.read())
    assert m and 32 * int(m.group(1)) == X.BF16_WG_POINTS           # a wave carries a block of 32 points
    assert X.N_PAST_CAP == X.GRID_CAP * X.BF16_WG_POINTS + X.BF16_WG_POINTS + 37


@pytest.mark.parametrize("name", NAMES)
def test_listed_case_compiles_on_the_host(name):
    """A configuration the host compiler refuses raises NotImplementedError at program construction; none is listed."""
    spec = X.BY_NAME[name]
    m = X.build_module(spec)
    if isinstance(spec, X.NerfSpec):
        assert isinstance(m.rgb_mlp.output_activation, torch.nn.Identity)       # rgb_activation=None is the identity
        calls = [m._call(True, spec.alpha_cond, True, spec.rgb_cond, True),
                 m._call(False, spec.alpha_cond, False, spec.rgb_cond, False)]
        n = spec.b * spec.s
    else:
        calls = [m._call(spec.want_dx), m._call(False)]
        n = spec.n
    for call in calls:
        for mode in (L.HN_MODE_F32, L.HN_MODE_BF16):
            assert call.program.host_tables(mode) is not None
            assert len(call.program.wgrad_jobs(mode, n)) > 0
