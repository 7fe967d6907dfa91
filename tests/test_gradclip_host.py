"""CPU tests of gradient clipping: the float64 restatement (tests/gradclip_restated.py) against torch's own
clip_grad_value_ + clip_grad_norm_, the argument checks of hn_grad_norm / hn_grad_scale that run before any launch, and the
refusals of optim.GradClip and TrainStep(clip_grad_norm=, clip_grad_value=) that fire before any device work."""
import math

import numpy as np
import pytest
import torch

import gradclip_restated as R
import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import optim
from hypernerf_torch_amd.training import TrainStep

NEW_SYMBOLS = ("hn_grad_norm", "hn_grad_scale")
INF = float("inf")
NAN = float("nan")
SHAPES = [(3, 5), (7,), (1,), (13, 11), (2, 3, 5), (9, 1)]          # odd shapes, 200 elements in all
N_TOTAL = sum(int(np.prod(s)) for s in SHAPES)
# torch works in fp32: its norm is a sum of N_TOTAL non-negative fp32 terms in an order of its own (a chain of at most
# N_TOTAL - 1 roundings of 2^-24 each, halved by the square root), the coefficient adds a sum and a division, the scaled
# gradient one product, the clamp nothing: (N_TOTAL + 8) * 2^-24 relative bounds every compared quantity
TOL = (N_TOTAL + 8) * 2.0 ** -24


def _grads(seed, spike=None):
    rng = np.random.default_rng(seed)
    gs = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    gs[3][4, 7], gs[0][1, 2] = 1e3, -1e3          # a few large entries: what the value clip is for
    if spike is not None:
        gs[4][1, 2, 3] = spike
    return gs


def _torch_clip(gs, max_norm, clip_value, grad_scale):
    """clip_grad_value_ then clip_grad_norm_ on CPU parameters whose gradients are grad_scale * g: (total_norm, list of
    clipped gradients), everything fp32."""
    params = [torch.nn.Parameter(torch.zeros(g.shape)) for g in gs]
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g.copy()) * grad_scale
    if clip_value is not None:
        torch.nn.utils.clip_grad_value_(params, clip_value)
    total = torch.nn.utils.clip_grad_norm_(params, INF if max_norm is None else max_norm, norm_type=2.0,
                                           error_if_nonfinite=False)
    return float(total), [p.grad.numpy().copy() for p in params]


def _check_against_torch(gs, max_norm, clip_value, grad_scale=1.0):
    flat = np.concatenate([g.reshape(-1) for g in gs])
    r = R.clip(flat, max_norm=max_norm, clip_value=clip_value, grad_scale=grad_scale)
    t_norm, t_grads = _torch_clip(gs, max_norm, clip_value, grad_scale)
    t_flat = np.concatenate([g.reshape(-1) for g in t_grads]).astype(np.float64)
    mine = grad_scale * r["buffer"]                # torch clipped s*g; the buffer holds the raw gradient
    if math.isfinite(t_norm):
        assert abs(r["total_norm"] - t_norm) <= TOL * t_norm, (r["total_norm"], t_norm)
    else:                                          # inf or NaN: the same non-finite value
        assert (math.isnan(t_norm) and math.isnan(r["total_norm"])) or r["total_norm"] == t_norm
    assert np.array_equal(np.isnan(mine), np.isnan(t_flat))
    ok = ~np.isnan(t_flat)
    assert np.all(np.abs(mine[ok] - t_flat[ok]) <= TOL * np.abs(t_flat[ok])), float(np.abs(mine[ok] - t_flat[ok]).max())
    return r, t_norm, t_flat


# ---- the restatement against torch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_value", [None, 2.5])
def test_restatement_equals_torch_when_the_clip_is_active(clip_value):
    gs = _grads(1)
    norm = R.clip(np.concatenate([g.reshape(-1) for g in gs]), clip_value=clip_value)["total_norm"]
    r, t_norm, _ = _check_against_torch(gs, norm / 3, clip_value)
    assert abs(r["coef_clamped"] - 1 / 3) < 1e-6 and r["coef"] == r["coef_clamped"]
    if clip_value is not None:
        assert np.abs(r["clamped"]).max() == 2.5 and norm < 100.0          # the spikes of 1e3 are gone from the norm
    else:
        assert norm > 1e3


def test_restatement_equals_torch_when_the_clip_is_inactive():
    gs = _grads(2)
    flat = np.concatenate([g.reshape(-1) for g in gs])
    norm = R.clip(flat)["total_norm"]
    r, _, t_flat = _check_against_torch(gs, 2 * norm, None)
    assert r["coef_clamped"] == 1.0 and r["coef"] > 1.9
    assert np.array_equal(r["buffer"], flat.astype(np.float64)) and np.array_equal(t_flat, flat.astype(np.float64))
    r = R.clip(flat, max_norm=INF)                 # measure only
    assert r["coef_clamped"] == 1.0 and r["total_norm"] == norm


def test_restatement_with_a_grad_scale_clips_the_scaled_gradient():
    gs = _grads(3)
    flat = np.concatenate([g.reshape(-1) for g in gs])
    half = R.clip(0.5 * flat.astype(np.float64), max_norm=4.0, clip_value=1.5)
    r, _, _ = _check_against_torch(gs, 4.0, 1.5, grad_scale=0.5)
    assert r["total_norm"] == pytest.approx(half["total_norm"], rel=1e-15)
    assert np.allclose(0.5 * r["buffer"], half["buffer"], rtol=1e-15, atol=0)
    assert R.threshold(1.5, 0.5) == np.float32(3.0) and R.threshold(None, 0.5) == np.float32(INF)


def test_an_all_zero_gradient_has_norm_zero_and_coefficient_one():
    gs = [np.zeros(s, dtype=np.float32) for s in SHAPES]
    r, t_norm, t_flat = _check_against_torch(gs, 1.0, 0.5)
    assert r["total_norm"] == 0.0 and t_norm == 0.0 and r["coef_clamped"] == 1.0
    assert not np.isnan(r["buffer"]).any() and not r["buffer"].any() and not t_flat.any()


def test_one_infinite_element():
    gs = _grads(4, spike=INF)
    r, t_norm, t_flat = _check_against_torch(gs, 1.0, None)
    assert r["total_norm"] == INF and t_norm == INF and r["coef_clamped"] == 0.0
    assert int(np.isnan(r["buffer"]).sum()) == 1 and not np.nan_to_num(r["buffer"]).any()      # inf * 0, the rest 0
    # the value clip runs first: it takes the infinity out of the norm
    r, t_norm, _ = _check_against_torch(gs, 1.0, 2.0)
    assert math.isfinite(r["total_norm"]) and not np.isnan(r["buffer"]).any()


def test_one_nan_element_poisons_everything_as_in_torch():
    gs = _grads(5, spike=NAN)
    for clip_value in (None, 2.0):                 # the clamp keeps a NaN
        r, t_norm, t_flat = _check_against_torch(gs, 1.0, clip_value)
        assert math.isnan(r["total_norm"]) and math.isnan(t_norm) and math.isnan(r["coef_clamped"])
        assert np.isnan(r["buffer"]).all() and np.isnan(t_flat).all()


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stands():
    assert set(NEW_SYMBOLS) <= set(L.EXPORTS) and set(NEW_SYMBOLS) <= set(L.ARGTYPES)
    HN.build()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.hn_version() == 340
    with open(L.HEADER) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name


FAKE = 0x1000          # a non-NULL, 16-byte aligned device address nothing reads: every refusal comes before a launch


def test_entry_points_refuse_bad_arguments_before_any_launch():
    HN.build()
    lib = L.load()

    def norm(grad=FAKE, n=8, s=1.0, v=INF, m=1.0, work=FAKE, out=FAKE):
        return lib.hn_grad_norm(grad, n, s, v, m, work, out, None)

    def scale(grad=FAKE, n=8, s=1.0, v=2.0, out=FAKE):
        return lib.hn_grad_scale(grad, n, s, v, out, None)

    common = (dict(n=0), dict(n=-4), dict(s=0.0), dict(s=-1.0), dict(s=NAN), dict(v=0.0), dict(v=-2.0), dict(v=NAN))
    for kw in common + (dict(m=0.0), dict(m=-1.0), dict(m=NAN)):
        assert norm(**kw) == -2, kw
    for kw in common:
        assert scale(**kw) == -2, kw
    # the argument check comes first, then the pointers, then their alignment
    assert norm(n=0, grad=None) == -2 and norm(grad=None, work=FAKE + 4) == -3 and scale(s=NAN, grad=None) == -2
    for kw in (dict(grad=None), dict(work=None), dict(out=None)):
        assert norm(**kw) == -3, kw
    assert scale(grad=None) == -3
    for kw in (dict(grad=FAKE + 4), dict(grad=FAKE + 8), dict(work=FAKE + 4), dict(work=FAKE + 12), dict(out=FAKE + 2),
               dict(out=FAKE + 1)):
        assert norm(**kw) == -4, kw
    for kw in (dict(grad=FAKE + 4), dict(grad=FAKE + 8), dict(out=FAKE + 2), dict(out=FAKE + 3)):
        assert scale(**kw) == -4, kw


# ---- optim.GradClip / TrainStep ------------------------------------------------------------------------------------
def _cpu_arena():
    return HN.ParamArena([torch.nn.Parameter(torch.zeros(5))])


BAD_KEYWORDS = [dict(), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=NAN), dict(clip_value=0.0),
                dict(clip_value=-0.5), dict(clip_value=NAN), dict(max_norm=1.0, clip_value=-1.0),
                dict(max_norm=NAN, clip_value=1.0)]


@pytest.mark.parametrize("kw", BAD_KEYWORDS, ids=[str(sorted(k.items())) for k in BAD_KEYWORDS])
def test_grad_clip_refuses_bad_keywords_before_device_work(kw):
    with pytest.raises(ValueError):
        HN.GradClip(_cpu_arena(), **kw)


def test_grad_clip_refuses_a_bad_grad_scale_and_cpu_arenas():
    for s in (0.0, -0.5, NAN):
        with pytest.raises(ValueError):
            optim.GradClip(_cpu_arena(), max_norm=1.0, grad_scale=s)
    # past the argument checks the arena must live on the GPU: there is no CPU fallback.  inf is legal: "measure only"
    for kw in (dict(max_norm=1.0), dict(max_norm=INF), dict(clip_value=0.5), dict(max_norm=2.0, clip_value=0.5)):
        with pytest.raises(L.HnError):
            optim.GradClip(_cpu_arena(), **kw)


@pytest.mark.parametrize("kw", [dict(clip_grad_norm=0.0), dict(clip_grad_norm=-1.0), dict(clip_grad_norm=NAN),
                                dict(clip_grad_value=0.0), dict(clip_grad_value=NAN),
                                dict(clip_grad_norm=1.0, clip_grad_value=-2.0)])
def test_train_step_refuses_bad_clip_keywords_at_construction(kw):
    """Before any device work: the model is on the CPU, and a valid keyword gets as far as the arena optimizer's refusal
    of CPU tensors."""
    model = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError):
        TrainStep(model, **kw)
    with pytest.raises(L.HnError):
        TrainStep(torch.nn.Linear(3, 2), clip_grad_norm=1.0)
