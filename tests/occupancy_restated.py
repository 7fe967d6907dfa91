"""csrc/hn_occupancy.hip restated in NumPy: the bit layout, the mark, the dilation, the fp32 DDA of
hn_occ_clip_rays operation by operation (vectorised over the rays, every float32 operation rounded on its own as the
kernel's are), and beside it a float64 brute force — every ray against every occupied cell — with the interval property
the clip must satisfy.  No GPU."""
import numpy as np

F = np.float32
# the probe grid of the interval property: 12 x 10 x 9 cells of edge 0.25 — every plane is exact in fp32, so the float64
# statement and the fp32 walk talk about the same cells
CELLS = (12, 10, 9)
BOUNDS = (-1.5, 1.5, -1.25, 1.25, -1.0, 1.25)
NEAR, FAR = 0.5, 6.0


# ---- bits ---------------------------------------------------------------------------------------------------------------------
def words(cz):
    return (cz + 63) // 64


def pack(cells_bool):
    """(cx, cy, cz) bool -> (cx, cy, words) int64: bit b of word w is cell 64 w + b, the padding bits are zero."""
    cx, cy, cz = cells_bool.shape
    padded = np.zeros((cx, cy, 64 * words(cz)), dtype=np.uint64)
    padded[:, :, :cz] = cells_bool
    shifts = np.arange(64, dtype=np.uint64)
    out = (padded.reshape(cx, cy, words(cz), 64) << shifts).sum(axis=-1, dtype=np.uint64)
    return out.view(np.int64)


def unpack(bits, cz):
    """(cx, cy, words) int64 -> ((cx, cy, cz) bool, (cx, cy, 64 words - cz) bool: the padding bits)."""
    u = np.ascontiguousarray(bits).view(np.uint64)
    shifts = np.arange(64, dtype=np.uint64)
    flat = ((u[..., None] >> shifts) & np.uint64(1)).astype(bool).reshape(u.shape[0], u.shape[1], -1)
    return flat[:, :, :cz], flat[:, :, cz:]


def popcount(bits):
    cells, pad = unpack(bits, 64 * bits.shape[2])
    return int(cells.sum())


def mark(grid, sigma_min):
    """(nx-1, ny-1, nz-1) bool: a cell is occupied iff one of its 8 corners is >= sigma_min or NaN."""
    with np.errstate(invalid="ignore"):
        point = ~(grid.astype(F) < F(sigma_min))
    nx, ny, nz = grid.shape
    out = np.zeros((nx - 1, ny - 1, nz - 1), dtype=bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                out |= point[di:di + nx - 1, dj:dj + ny - 1, dk:dk + nz - 1]
    return out


def dilate(cells_bool, radius=1):
    """The brute-force cube maximum: a cell is set iff a cell within `radius` steps along every axis was; no wrap."""
    cx, cy, cz = cells_bool.shape
    out = np.zeros_like(cells_bool)
    for i, j, k in zip(*np.nonzero(cells_bool)):
        out[max(i - radius, 0):i + radius + 1, max(j - radius, 0):j + radius + 1, max(k - radius, 0):k + radius + 1] = True
    return out


def dilate_words(bits, cz):
    """hn_occ_dilate on the packed words, as the kernel does it: per word the OR over the 3 x 3 neighbouring rows of the
    word, its two shifts and the carry bits of the words before and behind it, then the padding mask."""
    u = np.ascontiguousarray(bits).view(np.uint64)
    cx, cy, nw = u.shape
    one, top = np.uint64(1), np.uint64(63)
    row = u | (u << one) | (u >> one)
    row[:, :, 1:] |= u[:, :, :-1] >> top
    row[:, :, :-1] |= u[:, :, 1:] << top
    out = np.zeros_like(u)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            dst_i, src_i = slice(max(-di, 0), cx - max(di, 0)), slice(max(di, 0), cx - max(-di, 0))
            dst_j, src_j = slice(max(-dj, 0), cy - max(dj, 0)), slice(max(dj, 0), cy - max(-dj, 0))
            out[dst_i, dst_j] |= row[src_i, src_j]
    tail = cz - 64 * (nw - 1)
    if tail < 64:
        out[:, :, -1] &= np.uint64((1 << tail) - 1)
    return out.view(np.int64)


# ---- the fp32 walk of hn_occ_clip_rays ---------------------------------------------------------------------------------------
def grid_of(cells, bounds):
    lo, hi = np.asarray(bounds[0::2], dtype=F), np.asarray(bounds[1::2], dtype=F)
    return lo, (hi - lo) / np.asarray(cells, dtype=F)


def clip_rays(rays, occupied, bounds, near, far, clip_far=True, min_span=0.0):
    """{'t': (N, 2), 'hit': (N,) uint8, 'rays': (N, ld), 'affine': (N, 2)} as hn_occ_clip_rays gives them, float32."""
    rays = np.ascontiguousarray(rays, dtype=F)
    n = rays.shape[0]
    cells = occupied.shape
    lo, cell = grid_of(cells, bounds)
    near, far, min_span = F(near), F(far), F(min_span)
    o, d = rays[:, 0:3], rays[:, 3:6]
    inf = F(np.inf)

    def plane(a, i):
        return lo[a] + np.asarray(i).astype(F) * cell[a]

    def T(a, i, rows):
        with np.errstate(all="ignore"):
            return (plane(a, i) - o[rows, a]) / d[rows, a]

    every = np.arange(n)
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    te, tx = np.full(n, near, dtype=F), np.full(n, far, dtype=F)
    for a in range(3):
        zero = d[:, a] == 0
        ok &= ~zero | ((o[:, a] >= plane(a, 0)) & (o[:, a] <= plane(a, cells[a])))
        tlo, thi = T(a, 0, every), T(a, cells[a], every)
        pos = d[:, a] > 0
        with np.errstate(invalid="ignore"):
            te = np.where(zero | ~ok, te, np.maximum(te, np.where(pos, tlo, thi)))
            tx = np.where(zero | ~ok, tx, np.minimum(tx, np.where(pos, thi, tlo)))
    with np.errstate(invalid="ignore"):
        ok &= te < tx
    rows = np.nonzero(ok)[0]
    idx = np.zeros((n, 3), dtype=np.int64)
    for a in range(3):
        last = cells[a] - 1
        da, oa, t = d[rows, a], o[rows, a], te[rows]
        with np.errstate(all="ignore"):
            p = np.where(da == 0, oa, oa + da * t)
            fl = np.floor((p - lo[a]) / cell[a])
        i = np.where(~(fl > 0), 0, np.where(fl > F(last), last, np.nan_to_num(fl, posinf=0.0).astype(np.int64)))
        i = np.clip(i, 0, last)
        t_i, t_i1 = T(a, i, rows), T(a, i + 1, rows)
        pos, neg, zero = da > 0, da < 0, da == 0
        with np.errstate(invalid="ignore"):
            down = (pos & (i > 0) & (t_i > t)) | (neg & ~((i < last) & (t_i1 > t)) & (i > 0) & (t_i <= t)) \
                | (zero & (i > 0) & (plane(a, i) > oa))
            up = (pos & ~((i > 0) & (t_i > t)) & (i < last) & (t_i1 <= t)) | (neg & (i < last) & (t_i1 > t)) \
                | (zero & ~((i > 0) & (plane(a, i) > oa)) & (i < last) & (plane(a, i + 1) <= oa))
        idx[rows, a] = i - down + up
    t0, t1 = np.full(n, near, dtype=F), np.full(n, far, dtype=F)
    hit = np.zeros(n, dtype=bool)
    tc = te.copy()
    active = ok.copy()
    for _ in range(sum(cells) + 3):
        rows = np.nonzero(active)[0]
        if rows.size == 0:
            break
        tn = np.empty((rows.size, 3), dtype=F)
        for a in range(3):
            da = d[rows, a]
            tn[:, a] = np.where(da > 0, T(a, idx[rows, a] + 1, rows), np.where(da < 0, T(a, idx[rows, a], rows), inf))
        tout = np.minimum(np.minimum(tn[:, 0], tn[:, 1]), np.minimum(tn[:, 2], tx[rows]))
        count = occupied[idx[rows, 0], idx[rows, 1], idx[rows, 2]] & (tout > tc[rows])
        first = count & ~hit[rows]
        t0[rows[first]] = tc[rows[first]]
        t1[rows[count]] = tout[count]
        hit[rows[count]] = True
        go = tout < tx[rows]
        axis = np.where((tn[:, 0] <= tn[:, 1]) & (tn[:, 0] <= tn[:, 2]), 0, np.where(tn[:, 1] <= tn[:, 2], 1, 2))
        step = np.where(d[rows, axis] > 0, 1, -1)
        moved = idx[rows, axis] + step
        inside = (moved >= 0) & (moved < np.asarray(cells)[axis])
        go_rows = go & inside
        idx[rows[go_rows], axis[go_rows]] = moved[go_rows]
        tc[rows[go_rows]] = np.maximum(tc[rows[go_rows]], tout[go_rows])
        active[rows[~go_rows]] = False
    if not clip_far:
        t1 = np.where(hit, far, t1)
    span = t1 - t0
    short = hit & (span < min_span)
    grow = F(0.5) * (min_span - span)
    t0 = np.where(short, np.maximum(near, t0 - grow), t0)
    t1 = np.where(short, np.minimum(far, t1 + grow), t1)
    t0, t1 = np.where(hit, t0, near).astype(F), np.where(hit, t1, far).astype(F)
    identity = (t0 == near) & (t1 == far)
    b = np.where(identity, F(1), (t1 - t0) / (far - near)).astype(F)
    a = np.where(identity, F(0), t0 - b * near).astype(F)
    out = rays.copy()
    moved = ~identity
    with np.errstate(all="ignore"):
        out[moved, 0:3] = o[moved] + d[moved] * a[moved, None]
        out[moved, 3:6] = b[moved, None] * d[moved]
    return {'t': np.stack([t0, t1], axis=1), 'hit': hit.astype(np.uint8), 'rays': out, 'affine': np.stack([a, b], axis=1)}


# ---- float64: every ray against every occupied cell ---------------------------------------------------------------------------
def cell_chords(rays, occupied, bounds, near, far):
    """(t_in, t_out), both (N, M) float64 over the M occupied cells, clamped to [near, far]: the closed cell
    [x(i), x(i + 1)]^3 with x(i) = lo + i (hi - lo) / c in float64 against the ray in float64.  t_out - t_in is the chord,
    negative where the ray does not reach the cell; a ray that is not finite reaches none (chord -inf)."""
    rays = np.asarray(rays, dtype=np.float64)
    cells = np.asarray(occupied.shape)
    lo, hi = np.asarray(bounds[0::2], dtype=np.float64), np.asarray(bounds[1::2], dtype=np.float64)
    ijk = np.stack(np.nonzero(occupied), axis=1)
    c_lo = lo + ijk * (hi - lo) / cells
    c_hi = lo + (ijk + 1) * (hi - lo) / cells
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    with np.errstate(all="ignore"):
        ta, tb = (c_lo[None] - o) / d, (c_hi[None] - o) / d
        zero = d == 0
        inside = (o >= c_lo[None]) & (o <= c_hi[None])
        t_in = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
        t_out = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
        t_in = np.maximum(t_in.max(axis=2), near)
        t_out = np.minimum(t_out.min(axis=2), far)
    bad = ~np.isfinite(rays[:, 0:6]).all(axis=1)
    t_in[bad], t_out[bad] = np.inf, -np.inf
    t_in, t_out = np.nan_to_num(t_in, nan=np.inf, posinf=np.inf), np.nan_to_num(t_out, nan=-np.inf, neginf=-np.inf)
    return t_in, t_out


def interval_eps(t_max):
    """32 ulp of t_max: each plane distance is one subtraction and one correctly rounded division, about 4 ulp at most."""
    return 32.0 * 2.0 ** -23 * float(t_max)


def check_intervals(rays, occupied, bounds, near, far, t, hit, need_required=True):
    """The interval property of (t, hit) against the float64 statement; returns the shares it measured.  With
    eps = interval_eps(far): cells with chord > 2 eps are required, cells with chord >= -2 eps are allowed; the interval
    of a hit must reach both ends of the required cells and each of its ends must lie in an allowed cell, all within eps;
    hit is 1 with a required cell and 0 without an allowed one.  need_required=False (hand-made degenerate rays, where
    closed cells in float64 share faces): only the containment in the allowed cells, the hit rule for rays without an
    allowed cell, and finite outputs."""
    t, hit = np.asarray(t, dtype=np.float64), np.asarray(hit).astype(bool)
    assert np.isfinite(t).all() and (t[:, 0] <= t[:, 1]).all() and (t[:, 0] >= near).all() and (t[:, 1] <= far).all()
    eps = interval_eps(far)
    t_in, t_out = cell_chords(rays, occupied, bounds, near, far)
    chord = t_out - t_in
    required, allowed = chord > 2 * eps, chord >= -2 * eps
    any_required, any_allowed = required.any(axis=1), allowed.any(axis=1)
    assert not (hit & ~any_allowed).any(), f"hit without an allowed cell: rays {np.nonzero(hit & ~any_allowed)[0][:8]}"
    miss = ~hit
    assert (t[miss, 0] == near).all() and (t[miss, 1] == far).all()
    if need_required:
        assert not (any_required & ~hit).any(), f"miss with a required cell: rays {np.nonzero(any_required & ~hit)[0][:8]}"
        r_lo = np.where(required, t_in, np.inf).min(axis=1)
        r_hi = np.where(required, t_out, -np.inf).max(axis=1)
        rows = hit & any_required
        short = rows & ((t[:, 0] > r_lo + eps) | (t[:, 1] < r_hi - eps))
        assert not short.any(), f"interval misses a required cell: rays {np.nonzero(short)[0][:8]}"

    def distance(x):      # of every x to the nearest allowed interval (its cell may have a slightly negative chord)
        a, b = np.minimum(t_in, t_out), np.maximum(t_in, t_out)
        gap = np.maximum(np.maximum(a - x[:, None], x[:, None] - b), 0.0)
        return np.where(allowed, gap, np.inf).min(axis=1)

    outside = hit & ((distance(t[:, 0]) > eps) | (distance(t[:, 1]) > eps))
    assert not outside.any(), f"interval ends outside the allowed cells: rays {np.nonzero(outside)[0][:8]}"
    return {'ambiguous': float((required != allowed).any(axis=1).mean()), 'hit': float(hit.mean()),
            'miss': float(miss.mean())}


# ---- the probe ------------------------------------------------------------------------------------------------------------------
def probe_grid(seed=0, share=0.15):
    return np.random.default_rng(seed).random(CELLS) < share


def probe_rays(n=4000, seed=1, pad=0.5, columns=9):
    """n ray rows [o, d, near, far, frame]: origins at radius 0.2 .. 4 in a random direction, aimed at a random point of the
    box grown by `pad`, |d| in 0.7 .. 1.6."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    o = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.2, 4.0, size=(n, 1))
    lo, hi = np.asarray(BOUNDS[0::2]) - pad, np.asarray(BOUNDS[1::2]) + pad
    target = rng.uniform(lo, hi, size=(n, 3))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.6, size=(n, 1))
    rays = np.zeros((n, columns), dtype=F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, NEAR, FAR
    if columns > 8:
        rays[:, 8] = rng.integers(0, 50, size=n)
    return rays


def handmade_rays():
    """(rays (M, 9), names): the degenerate rays of the clip tests on the probe grid."""
    nan, inf = float("nan"), float("inf")
    rows = [
        ("axis-parallel +x", [-3.0, 0.1, 0.1, 1.0, 0.0, 0.0]),
        ("axis-parallel -z", [0.3, -0.4, 3.0, 0.0, 0.0, -1.0]),
        ("in the cell face y = 0.25", [-3.0, 0.25, 0.1, 1.0, 0.0, 0.0]),
        ("in the cell edge y = 0.25, z = 0.5", [-3.0, 0.25, 0.5, 1.0, 0.0, 0.0]),
        ("in the box face x = 1.5", [1.5, -3.0, 0.3, 0.0, 1.0, 0.0]),
        ("-0.0 components", [-3.0, 0.1, 0.1, 1.0, -0.0, -0.0]),
        ("-0.0 and a slope", [-3.0, 0.1, 0.1, 1.0, -0.0, 0.05]),
        ("origin inside, first cell", [0.1, 0.1, 0.1, 0.3, 0.5, 0.2]),
        ("origin inside, other cell", [-1.3, -1.1, -0.9, 0.6, 0.5, 0.4]),
        ("misses the box", [-3.0, 3.0, 0.0, 1.0, 0.0, 0.0]),
        ("points away", [-3.0, 0.0, 0.0, -1.0, 0.0, 0.0]),
        ("far ends inside", [-5.9, 0.1, 0.1, 1.0, 0.01, 0.0]),
        ("all negative", [1.4, 1.2, 1.2, -0.9, -0.7, -0.6]),
        ("diagonal through cell corners", [-2.5, -2.25, -2.0, 1.0, 1.0, 1.0]),
        ("NaN origin", [nan, 0.0, 0.0, 1.0, 0.0, 0.0]),
        ("NaN direction", [-3.0, 0.0, 0.0, 1.0, nan, 0.0]),
        ("inf origin", [inf, 0.0, 0.0, -1.0, 0.0, 0.0]),
        ("inf direction", [-3.0, 0.0, 0.0, inf, 0.0, 0.0]),
        ("zero direction inside", [0.1, 0.1, 0.1, 0.0, 0.0, 0.0]),
        ("zero direction outside", [3.0, 0.1, 0.1, 0.0, 0.0, -0.0]),
        ("grazes the corner (1.5, 1.25, z)", [1.5 - 2.0, 1.25 + 2.0 - 1e-4, 0.1, 1.0, -1.0, 0.0]),
    ]
    rays = np.zeros((len(rows), 9), dtype=F)
    for r, (_, v) in enumerate(rows):
        rays[r, 0:6] = v
    rays[:, 6], rays[:, 7], rays[:, 8] = NEAR, FAR, 7
    return rays, [name for name, _ in rows]
