"""CPU tests of the GIF path: the library's host LZW coder (hn_gif_lzw through ctypes) against the independent decoder
and coder of tests/gif_restated.py, the palette definition on cases worked out by hand and against Pillow's median cut,
the GIF container (write_gif / read_gif, and Pillow as a second reader where it imports), the stated JET table and the
validation stack.  No GPU: the library loads here, and quantised input is handed to write_gif as (palettes, indices)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gif_restated as R
import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import inference as I


@pytest.fixture(scope="module")
def lib():
    HN.build()
    return L.load()


def _lzw(lib, data: np.ndarray, cap=None):
    n = data.size
    cap = 2 * n + 16 if cap is None else cap
    out = np.full(cap + 8, 0xAB, dtype=np.uint8)                       # 8 guard bytes past the capacity
    out_len = C.c_longlong(-1)
    rc = lib.hn_gif_lzw(data.ctypes.data if n else None, n, out.ctypes.data, cap, C.byref(out_len))
    assert (out[cap:] == 0xAB).all(), "written past the capacity"
    return rc, out[:max(0, min(out_len.value, cap))].tobytes(), out_len.value


LZW_INPUTS = {
    "empty": np.zeros(0, dtype=np.uint8),
    "one": np.array([201], dtype=np.uint8),
    "equal4096": np.full(4096, 7, dtype=np.uint8),
    "ramp": np.arange(256, dtype=np.uint8),
    "random20000": np.random.default_rng(5).integers(0, 256, 20000).astype(np.uint8),
}


@pytest.mark.parametrize("name", list(LZW_INPUTS))
def test_lzw_against_restated_decoder_and_coder(lib, name):
    data = LZW_INPUTS[name]
    rc, codes, n_out = _lzw(lib, data)
    assert rc == 0 and n_out == len(codes)
    back, clears = R.lzw_decode(codes)
    assert back == data.tobytes()
    assert codes == R.lzw_encode(data)                                 # the definition leaves no freedom: same bytes
    assert codes == F.gif_lzw(data) == F.gif_lzw(torch.from_numpy(data.copy())) == F.gif_lzw(data.tobytes())
    if name == "random20000":
        assert clears >= 3, clears                                     # the opening clear and at least two resets
    elif name != "equal4096":
        assert clears == 1
    if name == "empty":
        assert codes == bytes([0x00, 0x03, 0x02])                      # 256 and 257 in 9 bits each, LSB first
    if name == "one":
        assert R.lzw_codes(data) == [(256, 9), (201, 9), (257, 9)]


def test_lzw_refusals(lib):
    data = LZW_INPUTS["random20000"]
    _, codes, need = _lzw(lib, data)
    for cap in (0, 1, need - 1):
        rc, _, n_out = _lzw(lib, data, cap=cap)
        assert rc == -6 and n_out == need                              # the needed size is reported, nothing past cap
    assert _lzw(lib, data, cap=need)[0] == 0
    out = np.zeros(64, dtype=np.uint8)
    n_out = C.c_longlong(0)
    one = np.array([1, 2, 3], dtype=np.uint8)
    assert lib.hn_gif_lzw(None, 3, out.ctypes.data, 64, C.byref(n_out)) == -3
    assert lib.hn_gif_lzw(one.ctypes.data, 3, None, 64, C.byref(n_out)) == -3
    assert lib.hn_gif_lzw(one.ctypes.data, 3, out.ctypes.data, 64, None) == -3
    assert lib.hn_gif_lzw(one.ctypes.data, -1, out.ctypes.data, 64, C.byref(n_out)) == -2
    assert lib.hn_gif_lzw(one.ctypes.data, 3, out.ctypes.data, -1, C.byref(n_out)) == -2
    assert not out.any()
    with pytest.raises(ValueError):
        F.gif_lzw(np.zeros(4, dtype=np.int32))


def test_c_abi_refuses_bad_arguments_before_any_launch(lib):
    names = {"hn_color_hist", "hn_palette_map", "hn_depth_range", "hn_depth_colormap", "hn_gif_lzw"}
    assert names <= set(L.EXPORTS) and "hn_gif.hip" in L.SOURCES
    one, odd, big = C.c_void_p(64), C.c_void_p(66), 2 ** 31 + 1       # never dereferenced: refused first
    assert lib.hn_color_hist(one, 0, one, None) == -2
    assert lib.hn_color_hist(one, big, one, None) == -2
    assert lib.hn_color_hist(None, 4, one, None) == -3
    assert lib.hn_color_hist(one, 4, None, None) == -3
    assert lib.hn_color_hist(one, 4, odd, None) == -4
    assert lib.hn_palette_map(one, 0, one, 4, one, None) == -2
    assert lib.hn_palette_map(one, 4, one, 0, one, None) == -2
    assert lib.hn_palette_map(one, 4, one, 257, one, None) == -2
    assert lib.hn_palette_map(None, 4, one, 4, one, None) == -3
    assert lib.hn_palette_map(one, 4, None, 4, one, None) == -3
    assert lib.hn_palette_map(one, 4, one, 4, None, None) == -3
    assert lib.hn_depth_range(one, 0, one, None) == -2
    assert lib.hn_depth_range(None, 4, one, None) == -3
    assert lib.hn_depth_range(one, 4, None, None) == -3
    assert lib.hn_depth_range(odd, 4, one, None) == -4
    assert lib.hn_depth_colormap(one, 0, one, one, one, None) == -2
    assert lib.hn_depth_colormap(one, 4, None, one, one, None) == -3
    assert lib.hn_depth_colormap(one, 4, one, None, one, None) == -3
    assert lib.hn_depth_colormap(one, 4, one, one, None, None) == -3
    assert lib.hn_depth_colormap(one, 4, odd, one, one, None) == -4


def test_ops_refuse_host_tensors_and_bad_shapes():
    px = torch.zeros((4, 3), dtype=torch.uint8)
    for call in (lambda: F.color_histogram(px), lambda: F.palette_map(px, px),
                 lambda: F.depth_colormap(torch.zeros(2, 2), I.jet_lut()), lambda: I.visualize_depth(torch.zeros(2, 2))):
        with pytest.raises(L.HnError):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(L.HnError):
            I.quantize_frames([torch.zeros((2, 2, 3), dtype=torch.uint8)])
    for call in (lambda: F.color_histogram(torch.zeros((4, 3))), lambda: F.color_histogram(torch.zeros((0, 3), dtype=torch.uint8)),
                 lambda: F.palette_map(px, torch.zeros((257, 3), dtype=torch.uint8)),
                 lambda: F.depth_colormap(torch.zeros(4), I.jet_lut()),
                 lambda: F.depth_colormap(torch.zeros(2, 2), torch.zeros((255, 3), dtype=torch.uint8)),
                 lambda: I.quantize_frames([torch.zeros((2, 2, 3), dtype=torch.uint8)], palette="local")):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------------------------
# the palette, by hand
# ------------------------------------------------------------------------------------------------------------------
def _table(rows):
    """{key: (count, sum r, sum g, sum b)} -> the 2^18-cell table."""
    h = np.zeros((R.HIST_BINS, 4), dtype=np.int64)
    for k, v in rows.items():
        h[k] = v
    return h


def _key(r, g, b):
    return ((r >> 2) << 12) | ((g >> 2) << 6) | (b >> 2)


def _both(h, colors=256):
    """The production palette, checked against the restatement on the way: (palette[:colors] as lists, used entries)."""
    pal, n = I.palette_from_histogram(h, colors)
    want, n_want = R.median_cut(h, colors)
    assert pal.dtype == np.uint8 and pal.shape == (256, 3) and not pal[colors:].any()
    assert n == n_want and np.array_equal(pal[:colors], want)
    pal_t, n_t = I.palette_from_histogram(torch.from_numpy(h), colors)
    assert n_t == n and np.array_equal(pal_t, pal)
    return pal, n


def test_palette_one_bin():
    # three pixels in cell (10, 20, 30) >> 2: (10, 20, 30), (11, 21, 31), (11, 23, 31): means 10.67, 21.33, 30.67
    pal, n = _both(_table({_key(10, 20, 30): (3, 32, 64, 92)}))
    assert n == 1 and pal[0].tolist() == [11, 21, 31] and not pal[1:].any()
    # a mean of exactly x.5 rounds up
    pal, n = _both(_table({_key(8, 8, 8): (2, 17, 19, 21)}))
    assert pal[0].tolist() == [9, 10, 11]
    with pytest.raises(ValueError):
        I.palette_from_histogram(np.zeros((R.HIST_BINS, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        I.palette_from_histogram(_table({0: (1, 0, 0, 0)}), colors=257)


def test_palette_256_bins_is_lossless():
    """256 colours on the lattice of step 4, one per cell, any counts: the palette is the colours, in key order."""
    cols = [(4 * (i // 64), 4 * ((i // 8) % 8), 4 * (i % 8)) for i in range(256)]
    cols = sorted(cols, key=lambda c: _key(*c))
    h = _table({_key(*c): (m, m * c[0], m * c[1], m * c[2]) for c, m in zip(cols, [1 + i % 5 for i in range(256)])})
    pal, n = _both(h)
    assert n == 256 and pal.tolist() == [list(c) for c in cols]
    frame = np.array(cols, dtype=np.uint8).reshape(16, 16, 3)
    assert np.array_equal(pal[R.palette_map(frame, pal)], frame)


def test_palette_257_bins_takes_exactly_one_merge():
    """257 single-pixel cells in 256 boxes: every cut adds one box, so 255 cuts leave ONE box with two entries and 255
    boxes with one.  255 colours come back exactly, and two share the entry floor(their mean + 0.5)."""
    cols = [(4 * (i % 64), 4 * (i // 64), 0) for i in range(257)]
    pal, n = _both(_table({_key(*c): (1, c[0], c[1], c[2]) for c in cols}))
    assert n == 256
    entries = {tuple(int(v) for v in p) for p in pal}
    merged = [c for c in cols if c not in entries]
    assert len(entries) == 256 and len(merged) == 2
    (r0, g0, _), (r1, g1, _) = merged
    assert (int(np.floor((r0 + r1) / 2 + 0.5)), int(np.floor((g0 + g1) / 2 + 0.5)), 0) in entries


def test_palette_cut_position_by_hand():
    """Four cells on the red axis at 0, 40, 80, 120 with 1, 1, 1, 5 pixels.  Ordered by red the cumulative counts are
    1, 2, 3, 8; half of 8 is first reached by the last entry, and the clamp moves the cut in front of it."""
    h = _table({_key(0, 0, 0): (1, 0, 0, 0), _key(40, 0, 0): (1, 40, 0, 0), _key(80, 0, 0): (1, 80, 0, 0),
                _key(120, 0, 0): (5, 600, 0, 0)})
    assert _both(h, 1)[0][:1].tolist() == [[90, 0, 0]]                               # 720 / 8
    assert _both(h, 2)[0][:2].tolist() == [[40, 0, 0], [120, 0, 0]]
    # only box 0 has more than one entry: counts 1, 1, 1, half = 1.5 is reached by the second; the right part is appended
    assert _both(h, 3)[0][:3].tolist() == [[20, 0, 0], [120, 0, 0], [80, 0, 0]]
    pal, n = _both(h, 4)
    assert n == 4 and pal[:4].tolist() == [[0, 0, 0], [40, 0, 0], [80, 0, 0], [120, 0, 0]]   # 4 entries: key order, no cut


def test_palette_tie_rules_by_hand():
    """Cells A (0,0,0) B (40,0,0) C (200,0,0) D (200,40,0) E (200,80,0) F (210,80,0), one pixel each.
    Cut 1: the red extent 210 beats green's 80; by (red, key) the order is A B C D E F, half of 6 is reached by C:
    {A, B, C} and {D, E, F}.  Box 0 scores 3 * 200 (red), box 1 3 * 40 (green): cut 2 takes box 0, order A B C, half of 3
    reached by B: {A, B} {D, E, F} {C}.  Now box 0 scores 2 * 40 = 80 on red and box 1 3 * 40 = 120 on green: cut 3 takes
    box 1, order D E F by green (E before F by key), half reached by E: {A, B} {D, E} {C} {F}.  Boxes 0 and 1 both score
    2 * 40: cut 4 takes the LOWER index, {A} {D, E} {C} {F} {B}."""
    cells = {"A": (0, 0, 0), "B": (40, 0, 0), "C": (200, 0, 0), "D": (200, 40, 0), "E": (200, 80, 0), "F": (210, 80, 0)}
    t = _table({_key(*c): (1, c[0], c[1], c[2]) for c in cells.values()})
    assert _both(t, 2)[0][:2].tolist() == [[80, 0, 0], [203, 67, 0]]
    assert _both(t, 3)[0][:3].tolist() == [[20, 0, 0], [203, 67, 0], [200, 0, 0]]
    assert _both(t, 4)[0][:4].tolist() == [[20, 0, 0], [200, 60, 0], [200, 0, 0], [210, 80, 0]]
    assert _both(t, 5)[0][:5].tolist() == [[0, 0, 0], [200, 60, 0], [200, 0, 0], [210, 80, 0], [40, 0, 0]]
    # equal extents on two channels: the LOWER channel is cut.  G (0,80,0) H (40,0,0) I (80,40,0): red and green both
    # span 80; by red the order is G H I and the cut after H gives {G, H} {I}; by green it would have been {H, I} {G}
    t = _table({_key(0, 80, 0): (1, 0, 80, 0), _key(40, 0, 0): (1, 40, 0, 0), _key(80, 40, 0): (1, 80, 40, 0)})
    assert _both(t, 2)[0][:2].tolist() == [[20, 40, 0], [80, 40, 0]]


def test_palette_no_worse_than_pillow_median_cut():
    Image = pytest.importorskip("PIL.Image")
    for surround in (False, True):
        frame = R.synthetic_frame(96, 128, surround=surround, seed=3)
        pal, n = I.palette_from_histogram(R.color_histogram(frame))
        want, n_want = R.median_cut(R.color_histogram(frame))
        assert n == n_want and np.array_equal(pal, want)
        ours = R.mse(pal[R.palette_map(frame, pal[:n])], frame)
        q = Image.fromarray(frame).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE)
        theirs = R.mse(np.asarray(q.convert("RGB")), frame)
        print(f"surround={surround}: this definition MSE {ours:.2f}, Pillow median cut MSE {theirs:.2f}")
        assert ours <= theirs, (surround, ours, theirs)


# ------------------------------------------------------------------------------------------------------------------
# the container
# ------------------------------------------------------------------------------------------------------------------
def _frames(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = R.synthetic_frame(h, w, surround=True, seed=seed)
    return [np.roll(base, 3 * i, axis=1) ^ rng.integers(0, 4, base.shape).astype(np.uint8) for i in range(n)]


def _quantised(frames, mode):
    pals, ns, idx = R.quantize(frames, mode)
    return ([torch.from_numpy(p) for p in pals], [torch.from_numpy(i) for i in idx]), pals, idx


@pytest.mark.parametrize("mode", ["global", "frame"])
def test_write_read_round_trip(tmp_path, mode):
    frames = _frames(3, 17, 33, seed=2)
    q, pals, idx = _quantised(frames, mode)
    path = str(tmp_path / "a.gif")
    I.write_gif(path, q, fps=30, loop=0, palette=mode)
    got = I.read_gif(path)
    assert got["loop"] == 0 and got["delays_cs"] == [3, 3, 3] and len(got["frames"]) == 3
    for i in range(3):
        assert np.array_equal(got["frames"][i], pals[0 if mode == "global" else i][idx[i]])
    data = open(path, "rb").read()
    assert data[:6] == b"GIF89a" and data[-1:] == b"\x3b"
    assert data[6:13] == bytes([33, 0, 17, 0, 0xF7 if mode == "global" else 0x70, 0, 0])
    off = 13 + (768 if mode == "global" else 0)
    assert data[off:off + 19] == b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
    assert data[off + 19:off + 27] == b"\x21\xf9\x04\x00\x03\x00\x00\x00"
    assert data[off + 27:off + 37] == bytes([0x2C, 0, 0, 0, 0, 33, 0, 17, 0, 0x00 if mode == "global" else 0x87])
    if mode == "global":
        assert data[13:13 + 768] == pals[0].tobytes()
    else:
        assert data[off + 37:off + 37 + 768] == pals[0].tobytes() and data[off + 37 + 768] == 8
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.size == (33, 17) and im.info.get("loop") == 0
        for i in range(3):
            im.seek(i)
            assert im.info["duration"] == 30
            assert np.array_equal(np.asarray(im.convert("RGB")), got["frames"][i])


def test_delays_loop_and_one_pixel(tmp_path):
    q, pals, idx = _quantised(_frames(2, 5, 7, seed=4), "global")
    for fps, delay in ((30, 3), (10, 10), (1000, 1), (24, 4), (0.001, None)):
        path = str(tmp_path / f"d{fps}.gif")
        if delay is None:
            with pytest.raises(ValueError):
                I.write_gif(path, q, fps=fps)
            continue
        I.write_gif(path, q, fps=fps, loop=5)
        got = I.read_gif(path)
        assert got["delays_cs"] == [delay, delay] and got["loop"] == 5
    one = np.array([[[9, 200, 31]]], dtype=np.uint8)
    q1, pals1, idx1 = _quantised([one], "frame")
    path = str(tmp_path / "one.gif")
    I.write_gif(path, q1, palette="frame")
    got = I.read_gif(path)
    assert len(got["frames"]) == 1 and np.array_equal(got["frames"][0], one) and got["delays_cs"] == [3]
    # a frame large enough for several sub-blocks and a table reset
    big = np.random.default_rng(1).integers(0, 256, (70, 90)).astype(np.uint8)
    pal = torch.from_numpy(np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], 1).astype(np.uint8))
    I.write_gif(path, ([pal], [torch.from_numpy(big)]))
    assert np.array_equal(I.read_gif(path)["frames"][0], pal.numpy()[big])


def test_write_gif_refusals(tmp_path):
    path = str(tmp_path / "x.gif")
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)      # noqa: E731
    pal = u8(256, 3)
    cases = [
        lambda: I.write_gif(path, []),
        lambda: I.write_gif(path, ([pal], [])),
        lambda: I.write_gif(path, [u8(4, 5, 3), u8(5, 4, 3)]),
        lambda: I.write_gif(path, ([pal], [u8(4, 5), u8(5, 4)])),
        lambda: I.write_gif(path, [u8(1, 65536, 3)]),
        lambda: I.write_gif(path, [u8(65536, 1, 3)]),
        lambda: I.write_gif(path, ([pal], [u8(1, 65536)])),
        lambda: I.write_gif(path, [torch.zeros((4, 5, 3))]),
        lambda: I.write_gif(path, [u8(4, 5, 4)]),
        lambda: I.write_gif(path, ([pal, pal], [u8(4, 5), u8(4, 5)]), palette="global"),
        lambda: I.write_gif(path, ([pal], [u8(4, 5), u8(4, 5)]), palette="frame"),
        lambda: I.write_gif(path, ([u8(255, 3)], [u8(4, 5)])),
        lambda: I.write_gif(path, ([pal], [u8(4, 5)]), palette="adaptive"),
        lambda: I.write_gif(path, ([pal], [u8(4, 5)]), fps=0),
        lambda: I.write_gif(path, ([pal], [u8(4, 5)]), loop=-1),
    ]
    for i, call in enumerate(cases):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} was accepted")
    import os
    assert not os.path.exists(path)
    with open(path, "wb") as f:
        f.write(b"GIF00a")
    with pytest.raises(ValueError):
        I.read_gif(path)


# ------------------------------------------------------------------------------------------------------------------
# the JET table and the stack
# ------------------------------------------------------------------------------------------------------------------
def _trapezoid(t, rise, top, fall, end):
    """The analytic jet channel on the 64-entry axis (0-based entries): 0 before `rise`, 1 on [top, fall], 0 from `end`
    on, linear between (slope 1/16 per entry)."""
    return float(np.clip(min((t - rise) / 16.0, (end - t) / 16.0), 0.0, 1.0)) if rise < t < end else 0.0


def test_jet_lut_against_the_analytic_trapezoids():
    lut = I.jet_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
    a = lut.numpy().astype(int)
    assert a[0].tolist() == [143, 0, 0]                                # blue 9/16 = 0.5625 -> 143.4
    assert a[255].tolist() == [0, 0, 128]                              # red 8/16 -> 127.5, to even
    # jet(64), 0-based entry t: red = trapezoid rising from 23 to 39, falling from 55 to 71; green 7 .. 23, 39 .. 55;
    # blue -9 .. 7, 23 .. 39
    for k in range(256):
        t = 63.0 * k / 255.0
        want = [_trapezoid(t, -9, 7, 23, 39), _trapezoid(t, 7, 23, 39, 55), _trapezoid(t, 23, 39, 55, 71)]
        for c in range(3):
            assert abs(a[k, c] - 255.0 * want[c]) <= 0.5 + 1e-9, (k, c, a[k, c], 255.0 * want[c])
    # monotone segments
    b, g, r = a[:, 0], a[:, 1], a[:, 2]
    k = lambda t: int(np.ceil(t * 255.0 / 63.0))           # noqa: E731  first table entry at or after 64-axis entry t
    assert (np.diff(b[:k(7)]) >= 0).all() and (b[k(7):k(23)] == 255).all() and (np.diff(b[k(23):]) <= 0).all()
    assert (b[k(39):] == 0).all()
    assert (g[:k(7) - 1] == 0).all() and (np.diff(g[:k(23)]) >= 0).all() and (g[k(23):k(39)] == 255).all()
    assert (np.diff(g[k(39):]) <= 0).all() and (g[k(55):] == 0).all()
    assert (r[:k(23) - 1] == 0).all() and (np.diff(r[:k(39)]) >= 0).all() and (r[k(39):k(55)] == 255).all()
    assert (np.diff(r[k(55):]) <= 0).all()
    assert torch.equal(I.jet_lut(), lut)


def test_validation_stack_shapes():
    h, w = 5, 7
    g = torch.Generator().manual_seed(0)
    gt, pred = torch.rand((h, w, 3), generator=g), torch.rand((h * w, 3), generator=g)
    pic = torch.rand((3, h, w), generator=g)
    s = I.validation_stack(gt, pred, pic)
    assert tuple(s.shape) == (3, 3, h, w) and s.dtype == torch.float32 and not s.is_cuda
    assert torch.equal(s[0], gt.permute(2, 0, 1)) and torch.equal(s[1], pred.view(h, w, 3).permute(2, 0, 1))
    assert torch.equal(s[2], pic)
    for bad in (lambda: I.validation_stack(gt, pred[:-1], pic), lambda: I.validation_stack(gt, pred, pic[:2]),
                lambda: I.validation_stack(gt[..., :2], pred, pic)):
        with pytest.raises(ValueError):
            bad()
    assert {"quantize_frames", "write_gif", "read_gif", "visualize_depth", "validation_stack", "jet_lut",
            "palette_from_histogram"} <= set(dir(I))
    assert {"color_histogram", "palette_map", "gif_lzw", "depth_colormap"} <= set(dir(F))
