"""GPU tests (MI355X) of the SE(3) exponential-map kernels, hn_se3_forward_kernel / hn_se3_backward_kernel behind
hn_se3_apply_* / hn_se3_warp_*, functional.se3_apply / se3_warp and SE3Field, against their float64 restatement
(tests/se3_restated.py, proven on the CPU by tests/test_se3_host.py) over the whole range of the rotation angle.

Every comparison is made per band (4096 rows of one (sigma_w, sigma_v), or one decade of the angle sweep) and per output:
max |err| / max |ref| INSIDE the band, never pooled — next to a band of moderate angles the error of a small-angle band
vanishes in the pooled maximum.  Bound: 1e-5 for sigma_w <= 4, 5e-5 for sigma_w = 20 (se3_restated.gpu_bound); the same
formulas in float32 on the CPU measure 6.1e-7 and 4.1e-6 (tests/test_se3_host.py holds them to a quarter of the bound),
the margin is for sinf / cosf a few units off.  Measured on an MI355X, worst band per output (y, d w, d v, d points):
6.1e-7, 4.6e-7, 2.5e-7, 5.6e-7 for sigma_w <= 4 and on the sweep, 4.0e-6, 2.0e-6, 2.5e-7, 2.6e-6 at sigma_w = 20.  The
kernels' earlier form, which divided by theta, measured 5.6e-5, 14, 9.6e-5, 5.6e-7 and NaN at theta = 0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
import se3_restated as R
from gpu_common import DEV, _record, assert_close, assert_grad_close
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import warping
from oracle import hypernerf_oracle as O

pytestmark = pytest.mark.gpu
KIND = "band max |err| / max |ref|"
SENTINEL = -7.25e11


def _se3_apply(w, v, p, g):
    """(y, d w, d v, d points) on the CPU through functional.se3_apply and autograd."""
    wd, vd, pd = (t.clone().to(DEV).requires_grad_(True) for t in (w, v, p))
    y = F.se3_apply(wd, vd, pd)
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return tuple(t.detach().cpu() for t in (y, wd.grad, vd.grad, pd.grad))


def _judge(label, got, ref, g, bound, rows=slice(None)):
    """Records and prints the four figures of one band; returns the list of (label, output, figure) above the bound."""
    bad = []
    for name, (err, scale, relative) in zip(R.NAMES, R.band_errors([t[rows] for t in got], [t[rows] for t in ref], g[rows])):
        _record(f"se3 {label}: {name}", KIND if relative else "band max |err| / max |g| (reference identically zero)",
                err / scale, bound)
        print(f"se3 {label}: {name} {err / scale:.3e} (bound {bound:.0e})")
        if not err <= bound * scale:
            bad.append((label, name, err / scale))
    return bad


@functools.lru_cache(maxsize=None)
def _all_bands():
    """Every band and the sweep through ONE forward and ONE backward launch: {band: (inputs, got, ref)}, 'sweep' included."""
    inputs = {band: R.band_inputs(*band) for band in R.BANDS}
    inputs["sweep"] = R.sweep_inputs()[1:]
    cat = [torch.cat([inputs[k][j] for k in inputs]).contiguous() for j in range(4)]
    got, ref = _se3_apply(*cat), R.apply(*cat)
    out, at = {}, 0
    for k, x in inputs.items():
        rows = slice(at, at + x[0].shape[0])
        out[k] = (x, tuple(t[rows] for t in got), tuple(t[rows] for t in ref))
        at = rows.stop
    return out


@pytest.mark.parametrize("sigma_w", R.SIGMA_W, ids=lambda s: f"{s:.3g}")
def test_se3_apply_in_every_band(sigma_w):
    """functional.se3_apply, forward and all three gradients, in the bands sigma_v = sigma_w, 0.3 and 0 of one sigma_w."""
    bad = []
    for band in (b for b in R.BANDS if b[0] == sigma_w):
        x, got, ref = _all_bands()[band]
        assert all(bool(torch.isfinite(t).all()) for t in got), band
        bad += _judge(f"sigma_w {band[0]:.3g}, sigma_v {band[1]:.3g}", got, ref, x[3], R.gpu_bound(sigma_w))
    assert not bad, bad


def test_se3_apply_on_the_angle_sweep_per_decade():
    """4096 angles, log-uniform from 1e-8 to 10, on one axis with v, p, g fixed: every decade is a band of its own."""
    x, got, ref = _all_bands()["sweep"]
    theta = torch.linalg.norm(x[0].double(), dim=-1)
    bad = []
    for label, rows in R.sweep_decades(theta):
        assert int(rows.sum()) > 400
        bad += _judge("sweep, " + label, got, ref, x[3], R.GPU_BOUND_MODERATE, rows)
    assert not bad, bad


def test_theta_zero_rows_among_moderate_ones():
    """A sixth of the rows of the band (0.5, 0.3) get w = 0 at hashed positions: there y = p + v bit for bit, the gradients
    are finite and meet the bound as a band of their own; the other rows keep the bits they have without the zero rows."""
    w, v, p, g = R.band_inputs(0.5, 0.3)
    zero = torch.from_numpy(H.uniform01(7, "se3 zero rows", w.shape[0]) < 1.0 / 6.0)
    assert 500 < int(zero.sum()) < 900 and bool((zero[1:] != zero[:-1]).sum() > 500)
    wz = torch.where(zero[:, None], torch.zeros_like(w), w)
    got, ref, plain = _se3_apply(wz, v, p, g), R.apply(wz, v, p, g), _se3_apply(w, v, p, g)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert torch.equal(got[0][zero], (p + v)[zero])
    assert torch.equal(got[2][zero], g[zero]) and torch.equal(got[3][zero], g[zero])
    bad = _judge("w = 0 rows among sigma_w 0.5", got, ref, g, R.GPU_BOUND_MODERATE, zero)
    bad += _judge("the rows next to w = 0 rows", got, ref, g, R.GPU_BOUND_MODERATE, ~zero)
    assert not bad, bad
    for a, b in zip(got, plain):
        assert torch.equal(a[~zero], b[~zero])


def _buffer(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.float32, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _apply_abi(w, v, p, g, n, need=(True, True, True)):
    """hn_se3_apply_forward / _backward on the first n rows of device tensors, into outputs one row longer than n that
    were filled with the sentinel: (y, d w, d v, d points), None where `need` says NULL."""
    y = _buffer(n + 1, 3)
    grads = [_buffer(n + 1, 3) if k else None for k in need]
    L.launch("hn_se3_apply_forward", L.ptr(w), L.ptr(v), L.ptr(p), C.c_int(n), L.ptr(y), L.stream_handle())
    L.launch("hn_se3_apply_backward", L.ptr(w), L.ptr(v), L.ptr(p), L.ptr(g), C.c_int(n), L.ptr(grads[0]), L.ptr(grads[1]),
             L.ptr(grads[2]), L.stream_handle())
    torch.cuda.synchronize()
    return (y, *grads)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_ragged_sizes_leave_the_row_past_the_end_alone(n):
    """One thread, one short of a block, a block, a block and a thread, four blocks short by 24: the first n rows of the
    band (1, 0.3) through the C ABI; row n of every output still holds the sentinel, rows 0 .. n-1 meet the bound."""
    x = [t[:n].contiguous() for t in R.band_inputs(1.0, 0.3)]
    out = _apply_abi(*(t.to(DEV) for t in x), n)
    for name, t in zip(R.NAMES, out):
        assert bool((_bits(t[n:]) == _bits(_buffer(1, 3))).all()), name
    bad = _judge(f"n = {n}", [t[:n].cpu() for t in out], R.apply(*x), x[3], R.GPU_BOUND_MODERATE)
    assert not bad, bad


def test_strided_operands_equal_the_contiguous_entry_points_bit_for_bit():
    """hn_se3_warp_forward / _backward driven directly: w | v interleaved in one (P, 6) buffer, points with row stride 5,
    the output gradient with row stride 7, d w | d v into one (P, 6) buffer, every combination of NULL d w / d v /
    d points.  Padding columns, the columns of a NULL gradient and the row past the end keep the sentinel; what is
    written equals hn_se3_apply_* on the same rows bit for bit."""
    n = 257
    w, v, p, g = (t[:n].contiguous().to(DEV) for t in R.band_inputs(1.0, 0.3))
    want = _apply_abi(w, v, p, g, n)
    wv, ps, gs = _buffer(n + 1, 6), _buffer(n + 1, 5), _buffer(n + 1, 7)
    wv[:n, :3], wv[:n, 3:], ps[:n, :3], gs[:n, :3] = w, v, p, g
    before = [t.clone() for t in (wv, ps, gs)]
    y = _buffer(n + 1, 3)
    wv_w, wv_v = C.c_void_p(wv.data_ptr()), C.c_void_p(wv.data_ptr() + 12)
    L.launch("hn_se3_warp_forward", wv_w, C.c_int(6), wv_v, C.c_int(6), L.ptr(ps), C.c_int(5), C.c_int(n), L.ptr(y), None,
             C.c_int(0), None, None, C.c_int(0), C.c_int(0), C.c_int(1), L.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(want[0]))
    for need in [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)]:
        d_wv, d_p = _buffer(n + 1, 6), _buffer(n + 1, 3)
        L.launch("hn_se3_warp_backward", wv_w, C.c_int(6), wv_v, C.c_int(6), L.ptr(ps), C.c_int(5), L.ptr(gs), C.c_int(7),
                 C.c_int(n), C.c_void_p(d_wv.data_ptr()) if need[0] else None, C.c_int(6),
                 C.c_void_p(d_wv.data_ptr() + 12) if need[1] else None, C.c_int(6), L.ptr(d_p) if need[2] else None,
                 L.stream_handle())
        torch.cuda.synchronize()
        untouched = _buffer(n + 1, 3)
        assert torch.equal(_bits(d_wv[:, :3]), _bits(want[1] if need[0] else untouched)), need
        assert torch.equal(_bits(d_wv[:, 3:]), _bits(want[2] if need[1] else untouched)), need
        assert torch.equal(_bits(d_p), _bits(want[3] if need[2] else untouched)), need
    for t, b in zip((wv, ps, gs), before):
        assert torch.equal(_bits(t), _bits(b))


@pytest.mark.parametrize("spr", [1, 32])
def test_rows_out_carries_xyz_and_the_table_row(spr):
    """rows_out = [xyz | table[idx[i / samples_per_ray]]] at n = 257 with a row stride two wider than 3 + H: the xyz columns
    equal `out` bit for bit, the table columns equal the table's rows exactly, the two padding columns and the row past
    the end keep the sentinel; an index below 0 or past the table gives NaN in the table columns of its rows only."""
    n, hdim, n_rows = 257, 8, 11
    rays = (n + spr - 1) // spr
    w, v, p, _ = (t[:n].contiguous().to(DEV) for t in R.band_inputs(1.0, 0.3))
    table = H.normal(9, "se3 table", (n_rows, hdim)).to(DEV)
    idx = torch.from_numpy((H.uniform01(9, "se3 idx", rays) * n_rows).astype(np.int64))
    for bad_rays in ((), (0, rays - 1)):
        ix = idx.clone()
        if bad_rays:
            ix[bad_rays[0]], ix[bad_rays[1]] = -1, n_rows
        out, rows = _buffer(n + 1, 3), _buffer(n + 1, 3 + hdim + 2)
        L.launch("hn_se3_warp_forward", L.ptr(w), C.c_int(3), L.ptr(v), C.c_int(3), L.ptr(p), C.c_int(3), C.c_int(n),
                 L.ptr(out), L.ptr(rows), C.c_int(3 + hdim + 2), L.ptr(table), L.ptr(ix.to(DEV)), C.c_int(hdim),
                 C.c_int(n_rows), C.c_int(spr), L.stream_handle())
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(_apply_abi(w, v, p, p, n, need=(False, False, True))[0]))
        assert torch.equal(_bits(rows[:, :3]), _bits(out))
        assert bool((_bits(rows[:, 3 + hdim:]) == _bits(_buffer(1, 1))).all()) and bool((_bits(rows[n:]) == _bits(_buffer(1, 1))).all())
        ray = torch.arange(n) // spr
        ok = (ix[ray] >= 0) & (ix[ray] < n_rows)
        got = rows[:n, 3:3 + hdim].cpu()
        assert torch.equal(got[ok], table.cpu()[ix[ray][ok]])
        assert int((~ok).sum()) == (min(spr, n) + n - (rays - 1) * spr if bad_rays else 0)      # the first ray's rows and the last one's
        assert bool(torch.isnan(got[~ok]).all()) and bool(torch.isfinite(rows[:n, :3]).all())


def _field(config):
    torch.manual_seed(1234)
    f = warping.SE3Field(in_ch=3)
    with torch.no_grad():
        if config in ("both logit biases zero", "w_net logit bias zero"):
            f.w_net.logit_layer.bias.zero_()
        if config == "both logit biases zero":
            f.v_net.logit_layer.bias.zero_()
    return f


@pytest.mark.parametrize("config", ["as constructed", "both logit biases zero", "w_net logit bias zero"])
def test_se3_field_warp_from_its_own_initialisation(config):
    """SE3Field.warp end to end in fp32 mode on 6 x 50 points against oracle.se3_field in float64 on the same parameters:
    as torch.manual_seed constructs it (logit weights uniform(1e-4), nn.Linear's default biases: |w| about 0.1), with
    both logit biases zeroed (HyperNeRF's own initialisation: |w| and |v| about 1e-3) and with the w_net one zeroed alone
    (|w| << |v|).  Output 1e-4 element-wise; every parameter gradient and d points 1e-3 of the tensor's largest entry,
    the bounds of tests/test_gpu_model.py::test_se3_field_warp_vs_oracle."""
    HN.set_precision("fp32")
    try:
        f = _field(config)
        sd = {k: v.detach().clone() for k, v in f.state_dict().items()}
        f = f.to(DEV)
        pts = H.uniform(41, "se3pts", (6, 50, 3), -1.0, 1.0)
        g = H.normal(41, "se3go", (6, 50, 3))
        prm = {"wf." + k: v.double().requires_grad_(True) for k, v in sd.items()}
        pr = pts.double().requires_grad_(True)
        ref = O.se3_field(prm, "wf", pr)
        assert ref.dtype == torch.float64
        (ref * g.double()).sum().backward()
        pg = pts.to(DEV).requires_grad_(True)
        out = f.warp(pg, None, {"warp_alpha": None})
        (out * g.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        with torch.no_grad():
            t = O.mlp(prm, "wf.trunk", O.posenc_jax(pr, 0, 8, use_identity=False), depth=6)
            wn = O.mlp(prm, "wf.w_net", t, depth=0).norm(dim=-1)
            vn = O.mlp(prm, "wf.v_net", t, depth=0).norm(dim=-1)
        print(f"SE3Field, {config}: |w| from {float(wn.min()):.2e} to {float(wn.max()):.2e}, |v| from {float(vn.min()):.2e} "
              f"to {float(vn.max()):.2e}")
        assert_close(out, ref, 1e-4, f"SE3Field.warp, {config}")
        bad = []
        for k, x in list(f.named_parameters()) + [("points", pg)]:
            want = pr.grad if k == "points" else prm["wf." + k].grad
            err = float((x.grad.double().cpu() - want).abs().max()) / (float(want.abs().max()) + 1e-12)
            print(f"SE3Field, {config}: d {k} {err:.3e}")
            try:
                assert_grad_close(x.grad, want, 1e-3, f"SE3Field, {config}: d {k}")
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, bad
    finally:
        HN.set_precision("bf16")
