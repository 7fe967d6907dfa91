"""GPU tests (MI355X) of gradient clipping: hn_grad_norm / hn_grad_scale against their float64 restatement
(tests/gradclip_restated.py) and torch's own clip_grad_value_ + clip_grad_norm_, optim.GradClip on an arena eagerly and as
a replayed graph, and TrainStep(clip_grad_norm=, clip_grad_value=)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradclip_restated as R
import hashprng as H
import hypernerf_torch_amd as HN
from gpu_common import DEV
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.graphs import GraphedStep
from hypernerf_torch_amd.hypernerf import model_utils
from hypernerf_torch_amd.losses import MSELoss
from hypernerf_torch_amd.training import TrainStep
from test_gpu_background import B, NC, NF, _Spy, _eager_launches, _ts_inputs, _ts_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
# one vector | a vector and a tail | a tail-only remainder behind one vector | fewer than 256 blocks | exactly one full grid
# stride (256 blocks x 256 threads x 4) | two strides and a tail
SIZES = [4, 5, 7, 1020, 262144, 524293]
# The norm: a chain of fp32 additions of non-negative terms, each rounding at most 2^-24 relative, so a chain of depth d
# is within d * 2^-24 of the exact sum (and the square root halves it).  The bound is the one for depth 64.  The kernel's
# chain at the largest size here, 524293: a thread owns at most 3 vectors = 12 terms (12 additions), then 6 shuffle steps
# of the wave-64 sum and 3 additions of the four wave sums through LDS: depth 21, plus one rounding per square — below 64.
# The fp64 combine of at most 256 partials adds nothing visible.
NORM_TOL = 64 * 2.0 ** -24


def _gradient(n, seed=0, scale=1.0):
    """Seeded normal gradients with a few entries of 1e3."""
    g = (np.random.default_rng(1000 * seed + n).standard_normal(n) * scale).astype(np.float32)
    g[1] = 1e3
    if n > 100:
        g[n // 2], g[n - 2] = -1e3, 1e3
    return g


def _launch(g, max_norm=None, clip_value=None, grad_scale=1.0):
    """The two entry points driven directly on a buffer of exactly len(g) floats (an arena pads to a multiple of four), with
    a fresh work / out pair: (out as float32[2], the buffer afterwards)."""
    buf = torch.from_numpy(np.asarray(g, dtype=np.float32).copy()).to(DEV)
    work = torch.zeros(260, dtype=torch.float32, device=DEV)
    out = torch.zeros(2, dtype=torch.float32, device=DEV)
    n, s = C.c_longlong(buf.numel()), C.c_float(grad_scale)
    v = C.c_float(INF if clip_value is None else clip_value)
    if max_norm is not None:
        L.launch("hn_grad_norm", L.ptr(buf), n, s, v, C.c_float(max_norm), L.ptr(work), L.ptr(out), L.stream_handle())
    L.launch("hn_grad_scale", L.ptr(buf), n, s, v, L.ptr(out if max_norm is not None else None), L.stream_handle())
    torch.cuda.synchronize()
    assert not bool(work[256:].view(torch.int32).any()), "the ticket word must be left at zero"
    return out.cpu().numpy(), buf.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(x):
    return float(np.float32(x))


def _check(g, out, buf, max_norm, clip_value, grad_scale, what):
    """out and the buffer of one run against the restatement: the norm to NORM_TOL, the coefficient within 2 ulp of the
    float64 formula at the kernel's own published norm, the buffer bit for bit given the kernel's own published
    coefficient."""
    r = R.clip(g, max_norm=max_norm, clip_value=clip_value, grad_scale=grad_scale)
    err = abs(float(out[0]) - r["total_norm"]) / r["total_norm"] if r["total_norm"] > 0 else abs(float(out[0]))
    want_coef = R.coef_of(np.float64(out[0]), max_norm)[1]
    ulps = abs(float(out[1]) - want_coef) / float(np.spacing(np.float32(want_coef)))
    print(f"grad clip {what}: n = {len(g)}, norm {float(out[0]):.8g} (restated {r['total_norm']:.8g}, rel err {err:.2e}), "
          f"coef {float(out[1]):.8g} ({ulps:.2f} ulp)")
    assert err <= NORM_TOL, (what, float(out[0]), r["total_norm"])
    assert ulps <= 2.0, (what, float(out[1]), want_coef)
    want = R.clamp(np.asarray(g, dtype=np.float32), R.threshold(clip_value, grad_scale)) * np.float32(out[1])
    assert want.dtype == np.float32 and np.array_equal(_bits(buf), _bits(want)), what
    return r


@pytest.mark.parametrize("n", SIZES)
def test_norm_coefficient_and_scaled_buffer(n):
    g = _gradient(n)
    norm = R.clip(g)["total_norm"]
    max_norm = _f32(norm / 3)
    out, buf = _launch(g, max_norm=max_norm)
    r = _check(g, out, buf, max_norm, None, 1.0, "active")
    assert norm > 1e3 and abs(float(out[1]) - 1 / 3) < 1e-5 and r["coef_clamped"] < 1.0
    # the same input twice: the same bits (no float atomics, the partials added in index order)
    out2, buf2 = _launch(g, max_norm=max_norm)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(_bits(buf), _bits(buf2))


@pytest.mark.parametrize("n", SIZES)
def test_an_inactive_clip_changes_no_bit(n):
    g = _gradient(n)
    norm = R.clip(g)["total_norm"]
    out, buf = _launch(g, max_norm=_f32(2 * norm))
    assert float(out[1]) == 1.0 and np.array_equal(_bits(buf), _bits(g))
    assert abs(float(out[0]) - norm) <= NORM_TOL * norm
    zero = np.zeros(n, dtype=np.float32)
    out, buf = _launch(zero, max_norm=1.0, clip_value=0.5)
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0 and np.array_equal(_bits(buf), _bits(zero))


@pytest.mark.parametrize("n", SIZES)
def test_value_then_norm_of_the_scaled_gradient(n):
    """Both clips with grad_scale = 0.5: the restatement of clipping the halved gradient (tests/test_gradclip_host.py pins
    that restatement to torch), the buffer itself still unscaled."""
    g = _gradient(n)
    half = R.clip(0.5 * g.astype(np.float64), max_norm=None, clip_value=1.5)
    max_norm = _f32(half["total_norm"] / 2)
    out, buf = _launch(g, max_norm=max_norm, clip_value=1.5, grad_scale=0.5)
    r = _check(g, out, buf, max_norm, 1.5, 0.5, "value + norm, grad_scale 0.5")
    ref = R.clip(0.5 * g.astype(np.float64), max_norm=max_norm, clip_value=1.5)
    assert abs(r["total_norm"] - ref["total_norm"]) <= 1e-12 * ref["total_norm"]
    assert abs(float(out[0]) - ref["total_norm"]) <= NORM_TOL * ref["total_norm"]
    # the entries of 1e3 (500 once halved) never reached the norm: no element of the halved gradient counts for more than 1.5
    assert np.abs(buf).max() <= 3.0 and float(out[0]) <= 1.5 * np.sqrt(n) * (1 + NORM_TOL) and float(out[0]) < 500.0
    # the value clip alone: no norm launch, the clamp bit for bit
    _, buf = _launch(g, clip_value=1.5, grad_scale=0.5)
    assert np.array_equal(_bits(buf), _bits(R.clamp(g, np.float32(3.0))))


def _arena(n):
    a = HN.ParamArena([torch.nn.Parameter(torch.zeros(n, device=DEV))])
    assert a.numel == (n + 3) // 4 * 4
    return a


def test_grad_clip_launches_only_what_can_change_something():
    n = 1020
    g = torch.from_numpy(_gradient(n)).to(DEV)
    norm = R.clip(g.cpu().numpy())["total_norm"]
    for kw, names in ((dict(max_norm=INF), ["hn_grad_norm"]), (dict(clip_value=2.0), ["hn_grad_scale"]),
                      (dict(max_norm=1.0), ["hn_grad_norm", "hn_grad_scale"]),
                      (dict(max_norm=INF, clip_value=2.0), ["hn_grad_norm", "hn_grad_scale"]),
                      (dict(max_norm=1.0, clip_value=2.0), ["hn_grad_norm", "hn_grad_scale"])):
        a = _arena(n)
        a.grad.copy_(g)
        clip = HN.GradClip(a, **kw)
        assert (clip.max_norm, clip.clip_value, clip.grad_scale) == (kw.get("max_norm"), kw.get("clip_value"), 1.0)
        assert clip.total_norm.dim() == 0 and clip.coef.dim() == 0 and clip.total_norm.is_cuda
        with pytest.raises(AttributeError):      # launch arguments, frozen into a captured graph: read-only
            clip.max_norm = 3.0
        with pytest.raises(AttributeError):
            clip.clip_value = 3.0
        with _Spy() as spy:
            clip.apply()
        torch.cuda.synchronize()
        assert spy.names == names, (kw, spy.names)
        if kw == dict(max_norm=INF):             # measure only
            assert torch.equal(a.grad, g) and float(clip.coef) == 1.0
            assert abs(float(clip.total_norm) - norm) <= NORM_TOL * norm
        if kw == dict(clip_value=2.0):
            assert np.array_equal(_bits(a.grad.cpu().numpy()), _bits(R.clamp(g.cpu().numpy(), np.float32(2.0))))


@pytest.mark.parametrize("spike", [INF, float("nan")], ids=["inf", "nan"])
def test_non_finite_elements_behave_as_in_torch(spike):
    """One inf or one NaN element (kernel level only, never through an optimizer): out and the buffer equal torch's CPU
    result of clip_grad_norm_ NaN for NaN — an inf makes the norm inf and the coefficient 0 (inf * 0 = NaN at the element,
    0 elsewhere), a NaN poisons the norm, the coefficient and every element."""
    n = 1020
    g = _gradient(n)
    g[777] = spike
    out, buf = _launch(g, max_norm=1.0)
    p = torch.nn.Parameter(torch.zeros(n))
    p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_([p], 1.0, norm_type=2.0, error_if_nonfinite=False)
    coef = torch.clamp(1.0 / (total + 1e-6), max=1.0)
    want = p.grad.numpy()
    assert np.array_equal(out, np.array([float(total), float(coef)], dtype=np.float32), equal_nan=True), (out, total, coef)
    assert np.array_equal(np.isnan(buf), np.isnan(want)) and np.array_equal(buf, want, equal_nan=True)
    assert int(np.isnan(buf).sum()) == (1 if spike == INF else n)
    # the value clip first: an inf is clamped out of the norm, a NaN stays
    p.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_value_([p], 2.0)
    total = torch.nn.utils.clip_grad_norm_([p], 1.0, norm_type=2.0, error_if_nonfinite=False)
    out, buf = _launch(g, max_norm=1.0, clip_value=2.0)
    assert np.isnan(out[0]) == bool(torch.isnan(total)) and np.array_equal(np.isnan(buf), np.isnan(p.grad.numpy()))
    if spike == INF:
        assert abs(float(out[0]) - float(total)) <= (128 + 64) * 2.0 ** -24 * float(total)
        # torch's own fp32 norm of 1020 terms (eight or more accumulators: chains of at most 128), this kernel's (64), and
        # the roundings of the two coefficients and products
        assert np.allclose(buf, p.grad.numpy(), rtol=(128 + 64 + 8) * 2.0 ** -24, atol=0)


def test_replays_of_a_captured_apply_equal_eager_runs():
    """apply() captured once, replayed three times on three different gradients (the second below the threshold: the
    early return of hn_grad_scale): out and the buffer equal a fresh eager run bit for bit, so the ticket re-arms itself
    and nothing is left over from the replay before."""
    n = 524293
    a = _arena(n)
    max_norm, value = 1500.0, 500.0          # norms of about 2300, 940 and 5100 behind the value clip
    clip = HN.GradClip(a, max_norm=max_norm, clip_value=value)
    a.grad[:n].copy_(torch.from_numpy(_gradient(n, seed=9)).to(DEV))
    graph = GraphedStep(clip.apply, warmup=1, mutates_params=False)
    coefs = []
    for k, scale in enumerate((3.0, 0.5, 7.0)):
        g = _gradient(n, seed=k + 1, scale=scale)
        a.grad[:n].copy_(torch.from_numpy(g).to(DEV))
        graph()
        torch.cuda.synchronize()
        out = torch.stack([clip.total_norm, clip.coef]).cpu().numpy()
        buf = a.grad.cpu().numpy()
        want_out, want_buf = _launch(np.concatenate([g, np.zeros(a.numel - n, dtype=np.float32)]), max_norm=max_norm,
                                     clip_value=value)
        assert np.array_equal(_bits(out), _bits(want_out)), (k, out, want_out)
        assert np.array_equal(_bits(buf), _bits(want_buf)), k
        coefs.append(float(out[1]))
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < coefs[0], coefs


# ----------------------------------------------------------------------------------------------------------------------
# on a real arena, and TrainStep(clip_grad_norm=, clip_grad_value=)
# ----------------------------------------------------------------------------------------------------------------------
SEED = 45
_EXTRA = {'nerf_alpha': None, 'warp_alpha': None, 'hyper_alpha': None, 'hyper_sheet_alpha': None}


def _rng(step=0):
    return {"t_rand": H.uniform(SEED + step, "t", (B, NC), 0, 1).to(DEV), "u": H.uniform(SEED + step, "u", (B, NF), 0, 1).to(DEV)}


@functools.lru_cache(maxsize=None)
def _n0():
    """The gradient norm of the first step of the small fp32 model, as TrainStep(clip_grad_norm=inf) logs it."""
    rays, rgbs = _ts_inputs(SEED)
    ts = TrainStep(_ts_model(SEED), lr=1e-3, use_graph=False, clip_grad_norm=INF)
    before = ts.arena.data.clone()
    log = ts.step(rays, rgbs, rng=_rng())
    assert set(log) == {"train/loss", "train/psnr", "train/grad_norm", "lr"}
    assert float(ts.clip.coef) == 1.0 and not torch.equal(ts.arena.data, before)
    return float(log["train/grad_norm"])


def test_logged_norm_and_clipped_buffer_on_a_real_arena():
    n0 = _n0()
    rays, rgbs = _ts_inputs(SEED)
    m = _ts_model(SEED)
    arena = HN.ParamArena(m.parameters())
    opt = HN.ArenaAdam(arena, lr=1e-3)
    clip = HN.GradClip(arena, max_norm=n0 / 2)
    F.backward(MSELoss()(m(model_utils.prepare_ray_dict(rays), dict(_EXTRA), rng=_rng()), rgbs))
    opt.finish_gradients()
    clones = [p.grad.detach().clone() for p in arena.params]
    flat = arena.grad.clone()
    clip.apply()
    torch.cuda.synchronize()
    ref = float(np.sqrt(sum(float((c.double() ** 2).sum()) for c in clones)))
    got = float(clip.total_norm)
    print(f"real arena: {arena.numel} floats, TrainStep logged {n0:.8g}, GradClip {got:.8g}, float64 {ref:.8g}")
    assert ref > 0 and abs(n0 - ref) <= NORM_TOL * ref and abs(got - ref) <= NORM_TOL * ref
    coef = clip.coef.clone()
    assert 0.49 < float(coef) < 0.51
    assert np.array_equal(_bits(arena.grad.cpu().numpy()), _bits((flat * coef).cpu().numpy()))
    pad = torch.ones(arena.numel, dtype=torch.bool, device=DEV)
    for p, o in zip(arena.params, arena.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 0 and not bool(arena.grad[pad].any()) and not bool(flat[pad].any())
    for p, c in zip(arena.params, clones):          # the parameters' own views see the clipped gradient
        assert torch.equal(p.grad, c * coef)


def test_clip_launches_sit_in_front_of_every_optimizer_launch(golden_dir):
    """Without the keywords two eager steps make exactly the recorded launches (tests/golden/g26_trainstep_launches.json);
    with clip_grad_norm the same list with hn_grad_norm, hn_grad_scale in front of each hn_adam_step."""
    with open(os.path.join(golden_dir, "g26_trainstep_launches.json")) as f:
        want = json.load(f)["launches"]
    n0 = _n0()
    rays, rgbs = _ts_inputs(SEED)
    F.seed_draws(5)
    plain = TrainStep(_ts_model(SEED), lr=1e-3, use_graph=False)
    assert plain.clip is None
    assert _eager_launches(plain, rays, rgbs) == want
    clipped = []
    for name in want:
        clipped += ["hn_grad_norm", "hn_grad_scale", name] if name == "hn_adam_step" else [name]
    assert want.count("hn_adam_step") == 2 and len(clipped) == len(want) + 4
    got = _eager_launches(TrainStep(_ts_model(SEED), lr=1e-3, use_graph=False, clip_grad_norm=n0 / 2), rays, rgbs)
    assert got == clipped, got
    value_only = _eager_launches(TrainStep(_ts_model(SEED), lr=1e-3, use_graph=False, clip_grad_value=1e-3), rays, rgbs)
    assert value_only == [n for n in clipped if n != "hn_grad_norm"]


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_clipped_graph_replays_equal_clipped_eager_steps(optimizer):
    """Three replayed steps against three eager ones with the norm clip active, every random tensor injected.  The bound
    is the one of the existing graph-versus-eager test, tests/test_gpu_training.py::
    test_first_graphed_step_applies_exactly_one_update: the same update up to the summation order of float atomics,
    |difference| > 1e-5 for fewer than 1e-3 of the parameters; 'train/grad_norm' within 1e-4 relative, as
    tests/test_gpu_background.py::test_graph_replays_equal_eager_steps holds the logged scalars under that same bound."""
    n0 = _n0()
    rays, rgbs = _ts_inputs(SEED)
    res, logs = {}, {}
    for use_graph in (False, True):
        ts = TrainStep(_ts_model(SEED), lr=1e-3, use_graph=use_graph, optimizer=optimizer, clip_grad_norm=n0 / 2,
                       clip_grad_value=n0 / 4)
        before = ts.arena.data.clone()
        snaps = []
        for step in range(3):
            log = ts.step(rays, rgbs, rng=_rng(step))
            snaps.append((ts.arena.data - before).clone())
            assert set(log) == {"train/loss", "train/psnr", "train/grad_norm", "lr"}
            logs.setdefault(use_graph, []).append(float(log["train/grad_norm"]))
        assert float(ts.optimizer.step_count) == 3.0
        res[use_graph] = snaps
    assert abs(logs[False][0] - n0) <= 1e-4 * n0          # the first step's norm is the unclipped run's
    for step in range(3):
        diff = (res[True][step] - res[False][step]).abs()
        frac = float((diff > 1e-5).float().mean())
        a, b = logs[True][step], logs[False][step]
        print(f"{optimizer}, clipped graph vs eager, step {step}: max |diff| {float(diff.max()):.3e}, fraction > 1e-5: "
              f"{frac:.2e}, grad norm {a:.8g} vs {b:.8g}")
        assert bool(res[True][step].any()) and frac < 1e-3, (step, frac)
        assert abs(a - b) <= 1e-4 * abs(b), (step, a, b)


_CHILD = r"""
import json, os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import torch
from hypernerf_torch_amd import _lib as L, optim
from hypernerf_torch_amd.training import TrainStep
from test_gpu_background import _Spy, _ts_inputs, _ts_model
assert optim.FUSE_REDUCE
rays, rgbs = _ts_inputs(45)
ts = TrainStep(_ts_model(45), lr=1e-3, use_graph=False, clip_grad_norm=1.0)
with _Spy() as spy:
    ts.step(rays, rgbs)
torch.cuda.synchronize()
print(json.dumps({"fuse_reduce": ts.optimizer.fuse_reduce, "names": spy.names}))
"""


def test_a_clipped_step_never_takes_the_fused_reduce_adam_launch():
    """HN_FUSE_REDUCE=1 (read at import, hence a child process): the fused launch never materialises the gradient, so a
    clipped TrainStep completes it with the plain reduce, clips, and steps with hn_adam_step."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["HN_FUSE_REDUCE"] = "1"
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    names = got["names"]
    assert got["fuse_reduce"] is False and "hn_mlp_wgrad_reduce_adam" not in names
    assert names[-4:] == ["hn_mlp_wgrad_reduce", "hn_grad_norm", "hn_grad_scale", "hn_adam_step"], names[-6:]
