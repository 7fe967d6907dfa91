"""Exactly representable networks for the MLP machine: generator, float64 reference, exactness conditions (NumPy only).

The idea of test_depth_index_bitexact_on_exact_sums applied to hn_mlp.hip: inputs in {-2..2}, weights 0 / +-1 with a
few non-zeros per row, biases in {-1, 0, 1}.  Then every pre-activation, activation, output and backward operand is a
small integer (a multiple of 2^-k with LeakyReLU(0.5)) that bfloat16 holds exactly, and every partial sum of every
product, in any order, is exact in fp32.  Summation order, bf16 rounding and float atomics drop out: the machine must
return the float64 reference in every bit, in fp32 and in bf16 mode alike.

`make_case` builds a case from a spec, `reference` evaluates it by hand in float64 (forward and backward, with every
tensor the machine feeds to a matrix product), `check_exact` states the conditions on the reference alone, `locate`
turns a mismatch into element indices and 32 x 32 tile coordinates.  MLP_CASES / NERF_CASES is the fixed case list.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

SLOPE = 0.5                 # the LeakyReLU slope of the exact cases: one fractional bit per layer
IN_VALUES = (-2, -1, 0, 1, 2)
DX_MAX_IN = 24              # inputs of at most this many channels are differentiated (as in test_mlp_random_shapes_fuzz)

# hn_grid_for (csrc/hn_mlp.hip) caps a launch at 256 * 4 workgroups; a bf16 workgroup is 8 waves x 32 points.  Past
# that a workgroup walks several tiles (the persistent loop).  tests/test_exact_mlp_host.py reads the cap back from
# the source.
GRID_CAP = 1024
BF16_WG_POINTS = 256
N_PAST_CAP = GRID_CAP * BF16_WG_POINTS + BF16_WG_POINTS + 37


@dataclass(frozen=True)
class Spec:
    """One modules.MLP case.  first_nnz / hidden_nnz / logit_nnz: non-zeros per weight row (0 = fully dense +-1,
    None = the default: 6 in the first layer, 2-3 in hidden layers, width / out_ch clamped to 3..8 in the logit layer)."""
    name: str
    in_ch: int
    width: int
    depth: int
    out_ch: int
    n: int
    skips: Tuple[int, ...] = ()
    out_act: str = "none"           # "none" | "relu"
    hidden: str = "relu"            # "relu" | "leaky"
    first_nnz: Optional[int] = None
    hidden_nnz: Optional[int] = None
    logit_nnz: Optional[int] = None
    seed: int = 0
    arena: bool = False             # also run with the parameters attached to a ParamArena

    @property
    def n_hidden(self):
        return max(self.depth, 1)

    @property
    def want_dx(self):
        return self.in_ch <= DX_MAX_IN


@dataclass(frozen=True)
class NerfSpec:
    """One modules.NerfMLP case: trunk 256 x 8 with skip [4], bottleneck 128, alpha head on [bottleneck | alpha
    condition (8)], rgb branch 128 x 1 on [bottleneck | rgb condition (12)], identity rgb activation."""
    name: str
    b: int
    s: int
    seed: int = 0
    in_ch: int = 12                 # 12 + 8 + 12 differentiated components: all 32 rows of the source-gradient tile
    trunk_depth: int = 8
    trunk_width: int = 256
    skips: Tuple[int, ...] = (4,)
    rgb_depth: int = 1
    rgb_width: int = 128
    alpha_cond: int = 8
    rgb_cond: int = 12
    arena: bool = False


# ---------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------
def _sparse_rows(rs, rows, cols, nnz):
    """(rows, cols) matrix of 0 / +-1.  nnz: per-row count, an int, a (lo, hi) range or 0 for dense.  The columns are
    dealt from shuffled decks, so every column is used about equally often: no input of a layer goes unread and the
    column sums (the backward products) stay small."""
    w = np.zeros((rows, cols), np.float32)
    if nnz == 0:
        return rs.choice(np.array([-1.0, 1.0], np.float32), size=(rows, cols))
    deck = []
    for r in range(rows):
        k = nnz if isinstance(nnz, int) else int(rs.randint(nnz[0], nnz[1] + 1))
        k = min(k, cols)
        pick = []
        while len(pick) < k:
            if not deck:
                deck = [int(c) for c in rs.permutation(cols)]
            c = deck.pop()
            if c not in pick:
                pick.append(c)
        w[r, pick] = rs.choice(np.array([-1.0, 1.0], np.float32), size=k)
    return w


def _bias(rs, n):
    return rs.randint(-1, 2, size=n).astype(np.float32) + np.float32(0.0)      # + 0.0: never -0.0


def _mlp_state(rs, prefix, in_ch, width, n_hidden, out_ch, skips, first_nnz, hidden_nnz, logit_nnz, main_in=0):
    """state-dict entries of one modules.MLP (nn.Linear layout (out, in)).  main_in: leading input columns that carry a
    running activation (the rgb branch's bottleneck) and get hidden-layer density."""
    sd = {}
    first = 6 if first_nnz is None else first_nnz
    hid = (2, 3) if hidden_nnz is None else hidden_nnz
    for i in range(n_hidden):
        if i == 0:
            if main_in:
                w = np.concatenate([_sparse_rows(rs, width, main_in, hid),
                                    _sparse_rows(rs, width, in_ch - main_in, 2)], axis=1)
            else:
                w = _sparse_rows(rs, width, in_ch, first)
        elif (i - 1) in skips:
            w = np.concatenate([_sparse_rows(rs, width, width, hid), _sparse_rows(rs, width, in_ch, 2)], axis=1)
        else:
            w = _sparse_rows(rs, width, width, hid)
        sd[f"{prefix}linears.{i}.weight"] = w
        sd[f"{prefix}linears.{i}.bias"] = _bias(rs, width)
    lg = max(3, min(8, -(-width // out_ch))) if logit_nnz is None else logit_nnz
    sd[f"{prefix}logit_layer.weight"] = _sparse_rows(rs, out_ch, width, lg)
    sd[f"{prefix}logit_layer.bias"] = _bias(rs, out_ch)
    return sd


def _ints(rs, shape, lo, hi):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32) + np.float32(0.0)


def make_case(spec, seed=None):
    """Integer-valued float32 arrays: inputs, output gradients and the module's state dict."""
    # the stream depends on the case's name, so no two cases share weights; `seed` picks among the streams of a name
    rs = np.random.RandomState((zlib.crc32(spec.name.encode()) + (spec.seed if seed is None else seed)) % 2 ** 32)
    if isinstance(spec, NerfSpec):
        sd = _mlp_state(rs, "trunk_mlp.", spec.in_ch, spec.trunk_width, spec.trunk_depth, spec.trunk_width, spec.skips,
                        None, None, (2, 3))
        bw = spec.trunk_width // 2
        sd["bottleneck_mlp.weight"] = _sparse_rows(rs, bw, spec.trunk_width, (2, 3))
        sd["bottleneck_mlp.bias"] = _bias(rs, bw)
        sd.update(_mlp_state(rs, "rgb_mlp.", bw + spec.rgb_cond, spec.rgb_width, spec.rgb_depth, 3, (), None, None, 8,
                             main_in=bw))
        sd["alpha_mlp.weight"] = np.concatenate([_sparse_rows(rs, 1, bw, 8), _sparse_rows(rs, 1, spec.alpha_cond, 3)], 1)
        sd["alpha_mlp.bias"] = _bias(rs, 1)
        return {"spec": spec, "state": sd,
                "x": _ints(rs, (spec.b, spec.s, spec.in_ch), -2, 2),
                "ac": _ints(rs, (spec.b, spec.alpha_cond), -2, 2),
                "rc": _ints(rs, (spec.b, spec.rgb_cond), -2, 2),
                "d_rgb": _ints(rs, (spec.b, spec.s, 3), -1, 1),
                "d_alpha": _ints(rs, (spec.b, spec.s, 1), -1, 1)}
    sd = _mlp_state(rs, "", spec.in_ch, spec.width, spec.n_hidden, spec.out_ch, spec.skips, spec.first_nnz,
                    spec.hidden_nnz, spec.logit_nnz)
    return {"spec": spec, "state": sd,
            "x": _ints(rs, (spec.n, spec.in_ch), IN_VALUES[0], IN_VALUES[-1]),
            "dY": _ints(rs, (spec.n, spec.out_ch), -2, 2)}


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference, by hand
# ---------------------------------------------------------------------------------------------------------------------
def _act(z, kind):
    if kind == "relu":
        return np.where(z > 0, z, 0.0)
    if kind == "leaky":
        return np.where(z > 0, z, SLOPE * z)
    assert kind == "none", kind
    return z


def _dact(dh, z, kind, rule):
    """dZ from the gradient w.r.t. the activation.  ReLU: kept where z > 0, and at z == 0 iff rule == 1 (bf16 mode
    keeps a clear sign bit; hn_push_mask).  LeakyReLU: z > 0 in both modes.  np.where, not a product: no -0.0."""
    if kind == "relu":
        keep = (z >= 0) if rule else (z > 0)
        return np.where(keep, dh, 0.0)
    if kind == "leaky":
        return np.where(z > 0, dh, SLOPE * dh) + 0.0
    return dh


class _Ref:
    def __init__(self):
        self.operands = {}      # name -> array the machine feeds to a matrix product
        self.grads = {}         # state-dict key -> gradient
        self.sums = {}          # name -> (|A|, |B|) factors of a float-accumulated gradient: sum_p |A[p, i]| |B[p, j]|
        self.zero_hits = 0      # hidden ReLU units with z == 0 exactly and a non-zero upstream gradient
        self.zero_hits_out = 0  # the same for the units of a ReLU output


def _mlp_forward(r, sd, prefix, inp, n_hidden, skips, hidden, out_act):
    """modules.MLP.forward (hypernerf/modules.py: linears[i] + activation, after layer i in skips the running activation
    becomes cat([activation, inputs]), then logit_layer + output activation)."""
    cache = {"inp": inp, "X": [], "Z": []}
    h = inp
    for i in range(n_hidden):
        w, b = sd[f"{prefix}linears.{i}.weight"].astype(np.float64), sd[f"{prefix}linears.{i}.bias"].astype(np.float64)
        r.operands[f"{prefix}linears.{i}.in"] = h
        z = h @ w.T + b
        cache["X"].append(h)
        cache["Z"].append(z)
        h = _act(z, hidden)
        if i in skips:
            h = np.concatenate([h, inp], axis=1)
    w, b = sd[f"{prefix}logit_layer.weight"].astype(np.float64), sd[f"{prefix}logit_layer.bias"].astype(np.float64)
    r.operands[f"{prefix}logit_layer.in"] = h
    z = h @ w.T + b
    cache["X"].append(h)
    cache["Z"].append(z)
    return _act(z, out_act), cache


def _linear_backward(r, sd, name, x, dz):
    """dW, db of one Linear and W^T dZ."""
    w = sd[name + ".weight"].astype(np.float64)
    r.operands[name + ".dZ"] = dz
    r.grads[name + ".weight"] = dz.T @ x
    r.grads[name + ".bias"] = dz.sum(0)
    r.sums[name + ".weight"] = (np.abs(dz), np.abs(x))
    r.sums[name + ".bias"] = (np.abs(dz), np.ones((x.shape[0], 1)))
    dh = dz @ w
    r.operands[name + ".WtdZ"] = dh
    return dh


def _mlp_backward(r, sd, prefix, cache, dy, n_hidden, skips, hidden, out_act, rule, width):
    """Gradient w.r.t. the MLP input: the first layer's term plus one term per skip, each recorded on its own."""
    if out_act == "relu":
        r.zero_hits_out += int(np.count_nonzero((cache["Z"][n_hidden] == 0) & (dy != 0)))
    dz = _dact(dy, cache["Z"][n_hidden], out_act, rule)
    dh = _linear_backward(r, sd, f"{prefix}logit_layer", cache["X"][n_hidden], dz)
    parts = []
    for i in reversed(range(n_hidden)):
        if i in skips:
            dh, dskip = dh[:, :width], dh[:, width:]
            r.operands[f"{prefix}linears.{i + 1}.WtdZ"] = dh
            r.operands[f"{prefix}linears.{i + 1}.dskip"] = dskip
            parts.append(dskip)
        z = cache["Z"][i]
        if hidden == "relu":
            r.zero_hits += int(np.count_nonzero((z == 0) & (dh != 0)))
        dz = _dact(dh, z, hidden, rule)
        dh = _linear_backward(r, sd, f"{prefix}linears.{i}", cache["X"][i], dz)
    parts.append(dh)
    d_inp = functools.reduce(np.add, parts[::-1])
    r.operands[f"{prefix}d_input"] = d_inp
    return d_inp, parts


def reference(case, relu_grad_at_zero):
    """The case in float64, forward and backward.  Returns a dict: outputs, input gradients, `grads` (state-dict key ->
    gradient), `operands`, `sums`, `zero_hits` and `zero_hits_out` (see _Ref)."""
    spec, sd = case["spec"], case["state"]
    r = _Ref()
    rule = int(relu_grad_at_zero)
    if isinstance(spec, NerfSpec):
        # modules.NerfMLP.forward: trunk (logit + hidden activation) -> bottleneck Linear -> alpha = Linear([bottleneck |
        # alpha condition]), rgb = MLP([bottleneck | rgb condition]); conditions (B, C) repeated over the S samples
        b, s = spec.b, spec.s
        n, bw = b * s, spec.trunk_width // 2
        x = case["x"].astype(np.float64).reshape(n, -1)
        ac = np.repeat(case["ac"].astype(np.float64), s, axis=0)
        rc = np.repeat(case["rc"].astype(np.float64), s, axis=0)
        t, c_t = _mlp_forward(r, sd, "trunk_mlp.", x, spec.trunk_depth, spec.skips, "relu", "relu")
        r.operands["bottleneck_mlp.in"] = t
        bn = t @ sd["bottleneck_mlp.weight"].astype(np.float64).T + sd["bottleneck_mlp.bias"].astype(np.float64)
        a_in = np.concatenate([bn, ac], axis=1)
        r.operands["alpha_mlp.in"] = a_in
        alpha = a_in @ sd["alpha_mlp.weight"].astype(np.float64).T + sd["alpha_mlp.bias"].astype(np.float64)
        r_in = np.concatenate([bn, rc], axis=1)
        rgb, c_r = _mlp_forward(r, sd, "rgb_mlp.", r_in, spec.rgb_depth, (), "relu", "none")
        d_rgb = case["d_rgb"].astype(np.float64).reshape(n, 3)
        d_alpha = case["d_alpha"].astype(np.float64).reshape(n, 1)
        d_rin, _ = _mlp_backward(r, sd, "rgb_mlp.", c_r, d_rgb, spec.rgb_depth, (), "relu", "none", rule, spec.rgb_width)
        d_ain = _linear_backward(r, sd, "alpha_mlp", a_in, d_alpha)
        d_bn = d_rin[:, :bw] + d_ain[:, :bw]
        d_t = _linear_backward(r, sd, "bottleneck_mlp", t, d_bn)
        dx, _ = _mlp_backward(r, sd, "trunk_mlp.", c_t, d_t, spec.trunk_depth, spec.skips, "relu", "relu", rule,
                              spec.trunk_width)
        d_ac, d_rc = d_ain[:, bw:], d_rin[:, bw:]
        r.operands["d_alpha_condition"], r.operands["d_rgb_condition"] = d_ac, d_rc
        ray = np.repeat(np.eye(b), s, axis=0)          # (n, b): the sum over a ray's samples
        r.sums["d_alpha_condition"], r.sums["d_rgb_condition"] = (ray, np.abs(d_ac)), (ray, np.abs(d_rc))
        out = {"rgb": rgb.reshape(b, s, 3), "alpha": alpha.reshape(b, s, 1), "dx": dx.reshape(b, s, -1),
               "d_ac": d_ac.reshape(b, s, -1).sum(1), "d_rc": d_rc.reshape(b, s, -1).sum(1)}
        outputs = ("rgb", "alpha")
    else:
        x = case["x"].astype(np.float64)
        y, cache = _mlp_forward(r, sd, "", x, spec.n_hidden, spec.skips, spec.hidden, spec.out_act)
        dx, _ = _mlp_backward(r, sd, "", cache, case["dY"].astype(np.float64), spec.n_hidden, spec.skips, spec.hidden,
                              spec.out_act, rule, spec.width)
        if not spec.want_dx:            # wide direct features: the machine forms no input gradient
            for k in [k for k in r.operands if k.endswith("dskip") or k in ("d_input", "linears.0.WtdZ")]:
                del r.operands[k]
        out = {"y": y, "dx": dx}
        outputs = ("y",)
    out.update(grads=r.grads, operands=r.operands, sums=r.sums, zero_hits=r.zero_hits, zero_hits_out=r.zero_hits_out,
               outputs=outputs)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# conditions
# ---------------------------------------------------------------------------------------------------------------------
def bf16_round_trip(a):
    """float32 -> bfloat16 (round to nearest even) -> float32, on the bit patterns."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _frac_bits(a):
    """smallest k >= 0 such that a * 2^k is all integers"""
    for k in range(0, 64):
        s = a * (2.0 ** k)
        if np.array_equal(s, np.rint(s)):
            return k
    raise AssertionError("not a dyadic tensor")


def _has_neg_zero(a):
    return bool(np.any(np.signbit(a) & (a == 0)))


def check_exact(ref):
    """The conditions under which any summation order and either numeric mode return the reference exactly.  Returns a
    list of violations (empty = exact); all of it on the reference alone."""
    bad = []
    ops = dict(ref["operands"])
    for k in ref["outputs"]:
        ops[k] = ref[k]
    for name, a in ops.items():
        f = a.astype(np.float32)
        if not np.array_equal(f.astype(np.float64), a):
            bad.append(f"{name}: not float32")
        elif not np.array_equal(bf16_round_trip(f), f):
            worst = float(np.abs(a[bf16_round_trip(f) != f]).max())
            bad.append(f"{name}: not bfloat16 (e.g. |v| = {worst})")
        if _has_neg_zero(a):
            bad.append(f"{name}: -0.0")
    results = dict(ref["grads"])
    for k in ("dx", "d_ac", "d_rc"):
        if k in ref:
            results[k] = ref[k]
    for name, a in results.items():
        if not np.array_equal(a.astype(np.float32).astype(np.float64), a):
            bad.append(f"{name}: not float32")
        if _has_neg_zero(a):
            bad.append(f"{name}: -0.0")
    for name, (fa, fb) in ref["sums"].items():
        gran = 2.0 ** -(_frac_bits(fa) + _frac_bits(fb))
        worst = float((fa.T @ fb).max()) if fa.size and fb.size else 0.0
        if not worst < 2.0 ** 24 * gran:
            bad.append(f"{name}: sum of |terms| {worst} >= 2^24 x {gran}")
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# failure messages
# ---------------------------------------------------------------------------------------------------------------------
def locate(got, want, first=6, max_tiles=12):
    """Where two arrays differ: the count, the first few (index, got, want) and the 32 x 32 tiles (row // 32, col // 32
    of the array seen as (-1, last dimension); a vector is one row) with the count per tile."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    n = int(np.count_nonzero(diff))
    if n == 0:
        return "identical"
    idx = np.argwhere(diff)
    head = ", ".join(f"{tuple(int(v) for v in i)}: got {got[tuple(i)]} want {want[tuple(i)]}" for i in idx[:first])
    d2 = diff.reshape(-1, diff.shape[-1]) if diff.ndim >= 1 and diff.size else diff.reshape(1, -1)
    rows, cols = np.nonzero(d2)
    tiles, counts = np.unique(np.stack([rows // 32, cols // 32], axis=1), axis=0, return_counts=True)
    tl = ", ".join(f"({int(t[0])}, {int(t[1])}): {int(c)}" for t, c in list(zip(tiles, counts))[:max_tiles])
    more = f", ... {len(tiles) - max_tiles} more tiles" if len(tiles) > max_tiles else ""
    return (f"{n} of {diff.size} elements differ; first: {head}; 32x32 tiles (row // 32, col // 32): count = {tl}{more} "
            f"[{len(tiles)} of {-(-d2.shape[0] // 32) * -(-d2.shape[1] // 32)} tiles]")


# ---------------------------------------------------------------------------------------------------------------------
# the case list: explicit and fixed (tests/test_exact_mlp_host.py asserts the coverage below and that every case is
# exact and compiles; tests/test_gpu_mlp_exact.py runs every one of them in fp32 and bf16 mode)
# ---------------------------------------------------------------------------------------------------------------------
def _S(name, in_ch, width, depth, out_ch, n, **kw):
    return Spec(name, in_ch, width, depth, out_ch, n, **kw)


MLP_CASES = (
    # -- every width x depth {0, 1, 2, 4, 8}, inputs with dx (1, 3, 20) and without (33, 64, 71, 190), narrow heads (1, 3,
    #    4: written from the raw accumulator) and wide outputs (5, 8, 17, 32, 40), point counts around the 32-point
    #    block and the 256-point workgroup
    _S("w8_d0_in3_o1_n1", 3, 8, 0, 1, 1),                                    # one Linear + head, a single point
    _S("w24_d1_in1_o3_n31", 1, 24, 1, 3, 31),                                # one input channel, width < one tile
    _S("w32_d2_skip0_in20_o4_n32", 20, 32, 2, 4, 32, skips=(0,), arena=True),   # skip [0] with dx, one full block
    _S("w53_d4_in33_o5relu_n33", 33, 53, 4, 5, 33, out_act="relu"),          # odd width, wide ReLU output, block + 1
    _S("w64_d8_skip13_in64_o8_n255", 64, 64, 8, 8, 255, skips=(1, 3), first_nnz=0),   # dense first layer in 64, two skips
    _S("w96_d4_skip0_in71_o17relu_n256", 71, 96, 4, 17, 256, skips=(0,), out_act="relu"),
    _S("w160_d2_in190_o32_n257", 190, 160, 2, 32, 257, first_nnz=0),         # dense first layer in 190 (3 aux groups)
    _S("w200_d8_skip13_in3_o40relu_n700", 3, 200, 8, 40, 700, skips=(1, 3), out_act="relu"),
    _S("w256_d8_skip0_in20_o3_n257", 20, 256, 8, 3, 257, skips=(0,), arena=True),
    _S("w256_d4_in190_o1_n700", 190, 256, 4, 1, 700),
    _S("w256_d2_in64_o40_n33", 64, 256, 2, 40, 33),
    # -- width 128 with depth >= 3: the pipelined 128 -> 128 body (ReLU), plain, with skips, feature-fed
    _S("w128_d4_in20_o3_n256", 20, 128, 4, 3, 256, arena=True),
    _S("w128_d8_skip13_in3_o1_n700", 3, 128, 8, 1, 700, skips=(1, 3)),
    _S("w128_d3_in64_o8relu_n33", 64, 128, 3, 8, 33, out_act="relu", first_nnz=0),
    _S("w128_d8_in71_o17_n255", 71, 128, 8, 17, 255),
    # -- LeakyReLU(0.5), depth <= 3 (one fractional bit per layer); width 128 takes the generic body here
    #    (the depth-3 ones with 4 / 3 non-zeros per first / logit row: y carries 4 fractional bits next to its integer part)
    _S("leaky_w32_d2_in3_o3_n33", 3, 32, 2, 3, 33, hidden="leaky"),
    _S("leaky_w64_d3_skip0_in20_o5_n257", 20, 64, 3, 5, 257, hidden="leaky", skips=(0,), first_nnz=4, logit_nnz=3),
    _S("leaky_w128_d3_in33_o4_n256", 33, 128, 3, 4, 256, hidden="leaky", first_nnz=4, logit_nnz=3),
    _S("leaky_w53_d1_in1_o17relu_n31", 1, 53, 1, 17, 31, hidden="leaky", out_act="relu"),
    _S("leaky_w200_d2_in71_o8_n32", 71, 200, 2, 8, 32, hidden="leaky"),
    # -- fully dense +-1 first layers (every K chunk of every tile at work), dense hidden layers at depth <= 2
    _S("dense_w256_d2_in20_o1_n700", 20, 256, 2, 1, 700, first_nnz=0),
    _S("dense_w96_d1_in3_o40_n255", 3, 96, 1, 40, 255, first_nnz=0),
    _S("dense_w200_d4_skip0_in71_o4_n31", 71, 200, 4, 4, 31, skips=(0,), first_nnz=0),
    _S("dense_w256_d8_skip13_in190_o3_n256", 190, 256, 8, 3, 256, skips=(1, 3), first_nnz=0, hidden_nnz=2),
    _S("dense_w8_d2_in1_o5_n32_hidden_dense", 1, 8, 2, 5, 32, first_nnz=0, hidden_nnz=0, logit_nnz=0),
    _S("dense_w24_d2_in20_o8relu_n1_hidden_dense", 20, 24, 2, 8, 1, first_nnz=0, hidden_nnz=0, out_act="relu"),
    _S("dense_w32_d2_in33_o32_n257_hidden_dense", 33, 32, 2, 32, 257, first_nnz=0, hidden_nnz=0),
    _S("dense_w64_d1_in64_o17_n33_logit_dense", 64, 64, 1, 17, 33, first_nnz=0, logit_nnz=0),
    # -- the rest of the cross: depth 0 on a wide net, narrow widths deep, padded widths with skips
    _S("w160_d0_in33_o4_n255", 33, 160, 0, 4, 255),
    _S("w8_d8_skip13_in3_o8_n256", 3, 8, 8, 8, 256, skips=(1, 3)),
    _S("w24_d4_skip0_in64_o1_n700", 64, 24, 4, 1, 700, skips=(0,)),
    _S("w53_d8_skip13_in20_o32relu_n31", 20, 53, 8, 32, 31, skips=(1, 3), out_act="relu"),
    _S("w96_d2_skip0_in1_o3_n1", 1, 96, 2, 3, 1, skips=(0,)),
    _S("w32_d4_in190_o40_n32", 190, 32, 4, 40, 32),
    _S("w200_d1_in20_o5_n33", 20, 200, 1, 5, 33),
    _S("w160_d8_skip13_in71_o17_n257", 71, 160, 8, 17, 257, skips=(1, 3)),
    # -- ReLU at exactly zero with a gradient arriving: biases in {-1, 0, 1} on integer sums make z == 0 common; the host
    #    test asserts that this case has such units (fp32 mode drops their gradient, bf16 mode keeps it)
    _S("relu_at_zero_w64_d4_in3_o8_n257", 3, 64, 4, 8, 257),
    # -- one workgroup past the persistent-loop cap in bf16 mode: 1024 full tiles + one more + 37 points
    _S("past_cap_w32_d2_in3_o3", 3, 32, 2, 3, N_PAST_CAP),
)

NERF_CASES = (
    NerfSpec("nerf_b7_s9", 7, 9, arena=True),          # 63 points: a partial second block, rays that straddle blocks
    NerfSpec("nerf_b33_s32", 33, 32),                  # 1056 points: 4 bf16 workgroups + one block
)

ZERO_CASE = "relu_at_zero_w64_d4_in3_o8_n257"
ALL_CASES = MLP_CASES + NERF_CASES
BY_NAME = {c.name: c for c in ALL_CASES}


@functools.lru_cache(maxsize=None)
def case_of(name):
    return make_case(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def reference_of(name, relu_grad_at_zero):
    """The reference of a listed case, computed once and shared: treat it as read-only."""
    return reference(case_of(name), relu_grad_at_zero)


def build_module(spec):
    """The module of a listed case on the CPU, its exact weights loaded (the only function here that needs torch)."""
    import torch
    from hypernerf_torch_amd.hypernerf import modules
    if isinstance(spec, NerfSpec):
        m = modules.NerfMLP(in_ch=spec.in_ch, trunk_depth=spec.trunk_depth, trunk_width=spec.trunk_width,
                            rgb_branch_depth=spec.rgb_depth, rgb_branch_width=spec.rgb_width, skips=list(spec.skips),
                            hidden_activation=torch.nn.ReLU(), rgb_activation=None,
                            alpha_brach_width=spec.trunk_width // 2, alpha_condition_dim=spec.alpha_cond,
                            rgb_condition_dim=spec.rgb_cond)
    else:
        m = modules.MLP(in_ch=spec.in_ch, out_ch=spec.out_ch, depth=spec.depth, width=spec.width, skips=list(spec.skips),
                        hidden_activation=torch.nn.LeakyReLU(SLOPE) if spec.hidden == "leaky" else torch.nn.ReLU(),
                        output_activation=torch.nn.ReLU() if spec.out_act == "relu" else None)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case_of(spec.name)["state"].items()})
    return m
