"""CPU proofs of tests/se3_restated.py, the reference that tests/test_gpu_se3.py holds the SE(3) exponential-map kernels
against: its float64 path equals the oracle's matrix form and torch autograd where that form is itself accurate, its
hand-written gradients equal autograd through its own forward at every angle (0 and the switch points included), nothing
jumps where it changes from the series to the closed forms, the six coefficients equal a 40-digit evaluation, and the same
formulas in float32 stay within a quarter of the bound the kernels are held to."""
import math

import pytest
import torch

import se3_restated as R
from oracle import hypernerf_oracle as O

F32, F64 = torch.float32, torch.float64
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def _ratios(got, ref, g):
    return [err / scale for err, scale, _ in R.band_errors(got, ref, g)]


def _oracle_forward(w, v, p):
    theta = torch.norm(w, dim=-1)
    rot, pvec = O.exp_se3(torch.cat([w / theta[:, None], v / theta[:, None]], dim=-1), theta)
    return (rot @ p[..., None])[..., 0] + pvec


MODERATE = [b for b in R.BANDS if 1e-2 <= b[0] <= 4.0]


@pytest.mark.parametrize("band", MODERATE, ids=lambda b: f"{b[0]:.3g}-{b[1]:.3g}")
def test_float64_restatement_equals_the_oracle_and_its_autograd(band):
    """oracle.exp_se3 with w / theta, v / theta, theta in float64 and torch autograd through it, in the bands where that
    form keeps nine digits (sigma_w from 1e-2 to 4): 1e-9 of the band's largest entry, forward and all three gradients."""
    assert len(MODERATE) == 18
    w, v, p, g = R.band_inputs(*band)
    got = R.apply(w, v, p, g, dtype=F64)
    ref = R.autograd(w, v, p, g, dtype=F64, fn=_oracle_forward)
    ratios = _ratios(got, ref, g)
    print(f"sigma_w {band[0]:.3g}, sigma_v {band[1]:.3g}: " + ", ".join(f"{n} {r:.2e}" for n, r in zip(R.NAMES, ratios)))
    assert max(ratios) <= 1e-9, ratios


@pytest.mark.parametrize("band", list(R.BANDS) + ["sweep"], ids=lambda b: b if b == "sweep" else f"{b[0]:.3g}-{b[1]:.3g}")
def test_hand_written_gradients_equal_autograd_through_the_own_forward(band):
    """Float64, every band and the sweep (theta = 0, theta^2 underflowing, both sides of the switch).  Bound 1e-10 of the
    band's largest entry: 2^-53 = 1.1e-16, times the 1 / theta^2 = 1e4 that the closed forms of C and C1 lose just above the
    switch, times 100 for the few dozen operations of each side.  With the float32 path's switch (theta = 1) in float64 as
    well: there the hand-written side takes A1, B1, C1 from their own seven-term series, autograd differentiates the
    seven-term series of A, B, C; the two differ by the first dropped term, at most 14 / 15! = 1.1e-11 at theta = 1."""
    if band == "sweep":
        _, w, v, p, g = R.sweep_inputs(dtype=F64)
    else:
        w, v, p, g = R.band_inputs(*band)
    for switch in (None, R.SWITCH[F32]):
        got = R.apply(w, v, p, g, dtype=F64, switch=switch)
        ref = R.autograd(w, v, p, g, dtype=F64, switch=switch)
        assert all(bool(torch.isfinite(t).all()) for t in got + ref)
        assert torch.equal(got[0], ref[0])
        ratios = _ratios(got, ref, g)
        print(f"{band}, switch {switch}: " + ", ".join(f"{n} {r:.2e}" for n, r in zip(R.NAMES, ratios)))
        assert max(ratios) <= 1e-10, (switch, ratios)


def test_theta_zero_is_the_pure_translation():
    """w = 0 exactly, and |w| = 1e-25 whose square underflows in float32: y = p + v and d v = d points = g bit for bit,
    d w = p x g + (v x g) / 2, in both dtypes."""
    for sigma_w in (0.0, 1e-25):
        w, v, p, g = R.band_inputs(sigma_w, 0.3)
        for dtype in (F32, F64):
            y, d_w, d_v, d_p = R.apply(w, v, p, g, dtype=dtype)
            wd, vd, pd, gd = (t.to(dtype) for t in (w, v, p, g))
            if sigma_w == 0.0 or dtype == F32:
                assert torch.equal(y, pd + vd) and torch.equal(d_v, gd) and torch.equal(d_p, gd)
            want = torch.cross(p.double(), g.double(), dim=-1) + 0.5 * torch.cross(v.double(), g.double(), dim=-1)
            assert float((d_w.double() - want).abs().max()) <= 8 * (EPS32 if dtype == F32 else EPS64) * float(want.abs().max())


# the switch point under test | the dtype of the arithmetic | the rounding unit of that dtype
SWITCHES = [(R.SWITCH[F32], F32, EPS32), (R.SWITCH[F64], F64, EPS64), (R.SWITCH[F32], F64, EPS64)]


@pytest.mark.parametrize("switch,dtype,eps", SWITCHES, ids=["float32-at-1", "float64-at-1e-2", "float64-at-1"])
def test_nothing_jumps_between_neighbouring_angles(switch, dtype, eps):
    """4096 log-uniform thetas from 1e-8 to 10 (neighbours 0.5 % apart) on one axis with v, p, g fixed.  The step of every
    output from one theta to the next may exceed the step of a smooth evaluation of the same inputs (float64, its only
    switch moved to theta = 0.1, away from the two under test) by rounding alone, relative to the output's largest entry
    up to there: 16 units of the dtype times (max(1, theta): sin and cos of a rounded theta; plus, on the closed-form side,
    3 / theta: C1 = (B - 3 C) / theta^2 carries 3 units / theta^4 and meets theta^3 in d w), plus, on the series side, twice
    the first term the series of A drops, theta^14 / 15! (7.6e-13 at theta = 1, 1e-5 of a float32 unit; nothing at 1e-2).
    The float32 path has the one switch at theta = 1; its formulas are also run in float64 with that switch, where a jump
    of the truncated series against the closed forms larger than that term cannot hide under float32 rounding."""
    _, w, v, p, g = R.sweep_inputs(dtype=dtype)
    got = R.apply(w, v, p, g, dtype=dtype, switch=switch)
    smooth = R.apply(w, v, p, g, dtype=F64, switch=0.1)
    theta = torch.linalg.norm(w.double(), dim=-1)
    at = int((theta < switch).sum())
    assert 0 < at < len(theta) - 1
    allowed = 16 * eps * (torch.clamp(theta, min=1.0) + torch.where(theta < switch, 0.0, 3.0 / theta))
    allowed = allowed + torch.where(theta < switch, 2.0 * theta ** (2 * R.TERMS) / math.factorial(2 * R.TERMS + 1), 0.0)
    allowed = allowed + 16 * EPS64 * torch.where(theta < 0.1, 0.0, 3.0 / theta)       # the smooth evaluation's own closed forms
    allowed = torch.maximum(allowed[1:], allowed[:-1])
    for name, a, b in zip(R.NAMES, got, smooth):
        a = a.double()
        step, want = (a[1:] - a[:-1]).abs().amax(-1), (b[1:] - b[:-1]).abs().amax(-1)
        scale = torch.cummax(b.abs().amax(-1), 0).values[1:]
        excess = ((a[1:] - a[:-1]) - (b[1:] - b[:-1])).abs().amax(-1) / scale
        print(f"{name}: largest step beyond the smooth one / allowed {float((excess / allowed).max()):.2f}, across the switch "
              f"{float(excess[at - 1]):.2e} (allowed {float(allowed[at - 1]):.2e})")
        assert bool((excess <= allowed).all()), (name, float((excess / allowed).max()))
        assert bool((step <= want + allowed * scale).all()), name


def test_coefficients_at_forty_digits():
    """A, B, C, A1, B1, C1 on the sweep against mpmath at 40 digits, every 16th angle and the angles next to the two switch
    points.  Above theta = 1 an error counts with the power of theta the coefficient meets in the outputs (A theta,
    B theta^2, C theta^2, A1 theta^2, B1 theta^3, C1 theta^3 are bounded functions of theta).  Allowed: 32 rounding units
    of the dtype, times what the closed forms lose below theta = 1 by subtracting: theta - sin(theta), cos - A and A - 2 B are
    differences of numbers of size theta, 1 and 1 divided by theta^3, theta^2 and theta^2 (1 / theta^2 each), and B - 3 C
    inherits three times the error of C and divides it by theta^2 again (3 / theta^4).  That loss is why float64 switches
    to the series at 1e-2; the series side is allowed none."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 100        # (b - 3 c) / x^2 at x = 1e-8 cancels 50 digits: what is left is good to more than 40
    theta = R.sweep_thetas()
    pick = sorted(set(range(0, len(theta), 16)) | {int((theta < s).sum()) + d for s in R.SWITCH.values() for d in (-1, 0)})
    powers = (1, 2, 2, 2, 3, 3)
    for dtype, eps in ((F32, EPS32), (F64, EPS64)):
        th = theta[pick].to(dtype)
        t = th * th
        got = [c.double() for c in R.coefficients(t)]
        worst = [0.0] * 6
        for i, ti in enumerate(t.double().tolist()):
            x = mp.sqrt(mp.mpf(ti))
            s, c = mp.sin(x), mp.cos(x)
            a, b, cc = s / x, (1 - c) / x ** 2, (x - s) / x ** 3
            exact = (a, b, cc, (c - a) / x ** 2, (a - 2 * b) / x ** 2, (b - 3 * cc) / x ** 2)
            m2 = 1.0 if float(x) < R.SWITCH[dtype] else max(1.0, 1.0 / ti)
            loss = (1.0, 1.0, m2, m2, m2, 3.0 * m2 * m2)
            for k in range(6):
                err = abs(float(mp.mpf(float(got[k][i])) - exact[k])) * max(1.0, float(x)) ** powers[k]
                worst[k] = max(worst[k], err / (32 * eps * loss[k]))
        print(f"{dtype}: worst error / allowance per coefficient " + ", ".join(f"{n} {w_:.2f}" for n, w_ in zip(R.COEF_NAMES, worst)))
        assert max(worst) <= 1.0, (dtype, worst)


def _float32_cases():
    for band in R.BANDS:
        w, v, p, g = R.band_inputs(*band)
        yield f"sigma_w {band[0]:.3g}, sigma_v {band[1]:.3g}", R.gpu_bound(band[0]), (w, v, p, g), slice(None)
    theta, w, v, p, g = R.sweep_inputs(dtype=F32)
    for label, rows in R.sweep_decades(theta):
        yield "sweep, " + label, R.GPU_BOUND_MODERATE, (w, v, p, g), rows


def test_float32_path_stays_within_a_quarter_of_the_gpu_bound():
    """Every band and every decade of the sweep, per output, max |err| / max |ref| inside the band: plain float32
    arithmetic meets the kernels' bound four times over, so the bound asks nothing of the hardware."""
    worst = {}
    for label, bound, inputs, rows in _float32_cases():
        ref = [t[rows] for t in R.apply(*inputs, dtype=F64)]
        got = [t[rows] for t in R.apply(*inputs, dtype=F32)]
        g = inputs[3][rows]
        for name, (err, scale, relative) in zip(R.NAMES, R.band_errors(got, ref, g)):
            allowed = 0.25 * bound * scale
            print(f"{label}: {name} {err / scale:.2e} of {'max |ref|' if relative else 'max |g|'} (allowed {0.25 * bound:.2e})")
            assert err <= allowed, (label, name, err / scale)
            key = (name, bound)
            worst[key] = max(worst.get(key, 0.0), err / scale)
    print("worst per output and bound:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert len(worst) == 8
