"""The MLP machine (csrc/hn_mlp.hip: forward, backward-data, weight gradient) bit for bit on exactly representable
networks (tests/exact_mlp.py), in fp32 and in bf16 mode.

Every product and every partial sum of these cases is exact in either mode and in any order (conditions:
exact_mlp.check_exact, asserted on the host by tests/test_exact_mlp_host.py), so there is no tolerance: every element of
every output and of every gradient must equal the float64 reference.  A failure names the 32 x 32 tiles that differ
(exact_mlp.locate).  The reference follows the documented ReLU-at-zero rule of the mode (hn_push_mask):
fp32 mode keeps the gradient where z > 0, bf16 mode where the sign bit is clear.  bf16s8 is left out on purpose: its
8-bit stash is lossy by definition.

Run this file first after any change to hn_mlp.hip:  pytest -m gpu tests/test_gpu_mlp_exact.py
"""
import numpy as np
import pytest
import torch

import exact_mlp as X
import hypernerf_torch_amd as HN
from gpu_common import DEV

pytestmark = pytest.mark.gpu

RULE = {"fp32": 0, "bf16": 1}           # relu_grad_at_zero of the mode
MLP_NAMES = [c.name for c in X.MLP_CASES]
NERF_NAMES = [c.name for c in X.NERF_CASES]
ARENA_NAMES = [c.name for c in X.ALL_CASES if c.arena]


@pytest.fixture(params=["fp32", "bf16"])
def precision(request):
    old = HN.get_precision()
    HN.set_precision(request.param)
    yield request.param
    HN.set_precision(old)


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def mismatch(got, want, what):
    """torch.equal against the float64 reference (exactly a float32 by check_exact): None, or a message that locates the
    differing elements and tiles."""
    if got is None:
        return what + ": missing"
    got = got.detach().cpu()
    want = torch.from_numpy(np.asarray(want, np.float64).astype(np.float32))
    if got.dtype != torch.float32 or got.shape != want.shape:
        return f"{what}: {got.dtype} {tuple(got.shape)}, expected float32 {tuple(want.shape)}"
    return None if torch.equal(got, want) else f"{what}: {X.locate(got.numpy(), want.numpy())}"


def assert_all_identical(pairs):
    """Every (tensor, reference, name) compared before anything is asserted: a failure lists EVERY tensor that differs,
    in the order given (outputs, input gradients, parameter gradients from the first layer on), each with its tiles."""
    bad = [m for m in (mismatch(g, w, what) for g, w, what in pairs) if m is not None]
    assert not bad, f"{len(bad)} of {len(pairs)} tensors differ:\n" + "\n".join(bad)


def run(m, case, train):
    """One forward (and backward) of the case's module: ({output name: tensor}, {input-gradient name: tensor})."""
    spec = case["spec"]
    if isinstance(spec, X.NerfSpec):
        x, ac, rc = dev(case["x"], train), dev(case["ac"], train), dev(case["rc"], train)
        out = m(x, ac, rc)
        if train:
            torch.autograd.backward([out["rgb"], out["alpha"]], [dev(case["d_rgb"]), dev(case["d_alpha"])])
        return {"rgb": out["rgb"], "alpha": out["alpha"]}, {"dx": x.grad, "d_ac": ac.grad, "d_rc": rc.grad}
    x = dev(case["x"], train and spec.want_dx)
    y = m(x)
    if train:
        y.backward(dev(case["dY"]))
    return {"y": y}, ({"dx": x.grad} if spec.want_dx else {})


def check_inference(name, precision):
    case, ref = X.case_of(name), X.reference_of(name, RULE[precision])
    m = X.build_module(case["spec"]).to(DEV)
    with torch.no_grad():
        outs, _ = run(m, case, False)
    assert_all_identical([(v, ref[k], f"{name} {precision} inference {k}") for k, v in outs.items()])


def check_training(name, precision, arena):
    """Training forward + backward, then a second backward of a fresh forward into the same gradients: exactly twice
    the reference.  With `arena` the parameters live in a ParamArena and the gradients are read from its flat buffer."""
    case, ref = X.case_of(name), X.reference_of(name, RULE[precision])
    m = X.build_module(case["spec"]).to(DEV)
    named = dict(m.named_parameters())
    assert set(named) == set(ref["grads"])
    ar = HN.ParamArena(m.parameters()) if arena else None

    def grad_of(p):
        if ar is None:
            return p.grad
        off = ar.attached(p)
        assert off is not None
        return ar.grad[off:off + p.numel()].view(p.shape)

    for times in (1, 2):
        outs, dins = run(m, case, True)
        what = f"{name} {precision}{' arena' if arena else ''} backward {times}:"
        assert_all_identical([(v, ref[k], f"{what} {k}") for k, v in list(outs.items()) + list(dins.items())] +
                             [(grad_of(p), times * ref["grads"][k], f"{what} d {k}") for k, p in named.items()])


@pytest.mark.parametrize("name", MLP_NAMES)
def test_mlp_inference_forward_is_exact(name, precision):
    check_inference(name, precision)


@pytest.mark.parametrize("name", MLP_NAMES)
def test_mlp_forward_backward_and_accumulated_gradients_are_exact(name, precision):
    check_training(name, precision, arena=False)


@pytest.mark.parametrize("name", NERF_NAMES)
def test_nerf_mlp_inference_forward_is_exact(name, precision):
    check_inference(name, precision)


@pytest.mark.parametrize("name", NERF_NAMES)
def test_nerf_mlp_forward_backward_and_accumulated_gradients_are_exact(name, precision):
    check_training(name, precision, arena=False)


@pytest.mark.parametrize("name", ARENA_NAMES)
def test_gradients_in_the_param_arena_are_exact(name, precision):
    check_training(name, precision, arena=True)
