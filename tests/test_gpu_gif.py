"""GPU tests (MI355X) of the GIF path (csrc/hn_gif.hip): the colour table, the palette search, the depth colour map and
what evaluate_images writes, each against the NumPy statements of tests/gif_restated.py.  Everything here is integer
arithmetic or individually rounded float32, so every comparison is for equality."""
import os

import numpy as np
import pytest
import torch

import gif_restated as R
from gpu_common import DEV
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import inference as I

pytestmark = pytest.mark.gpu


def _pixels(n, seed, kind="noise"):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (n, 3)).astype(np.uint8)
    # a few colours many times over, in runs and scattered: several lanes of a wave share a cell
    few = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    return few[np.sort(rng.integers(0, 5, n)) if kind == "runs" else rng.integers(0, 5, n)]


def _hist(px_np, out=None):
    return F.color_histogram(torch.from_numpy(px_np).to(DEV), out=out)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("kind", ["noise", "runs", "scattered"])
def test_histogram_equals_restated(n, kind):
    px = _pixels(n, 7 * n + len(kind), kind)
    got = _hist(px)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1 << 18, 4)
    want = R.color_histogram(px)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(got[:, 0].sum()) == n
    assert torch.equal(_hist(px), got)                                  # a second run: the same table


def test_histogram_frame_offset_contention_accumulation():
    # a 7 x 5 frame, as (H, W, 3)
    frame = _pixels(35, 1).reshape(7, 5, 3)
    assert np.array_equal(F.color_histogram(torch.from_numpy(frame).to(DEV)).cpu().numpy(), R.color_histogram(frame))
    # a base pointer one byte off any alignment
    raw = torch.from_numpy(_pixels(1001, 2).reshape(-1)).to(DEV)
    buf = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):
        view = buf[off:off + raw.numel()]
        view.copy_(raw)
        assert view.data_ptr() == buf.data_ptr() + off
        got = F.color_histogram(view.view(-1, 3))
        assert np.array_equal(got.cpu().numpy(), R.color_histogram(raw.cpu().numpy()))
    # every pixel in one cell: 65 536 pixels, three different colours of the cell (sums differ from count * colour)
    same = np.tile(np.array([[252, 253, 255], [255, 252, 254], [253, 255, 252]], dtype=np.uint8), (21846, 1))[:65536]
    got = _hist(same)
    assert np.array_equal(got.cpu().numpy(), R.color_histogram(same))
    assert int((got[:, 0] != 0).sum()) == 1 and int(got[:, 0].max()) == 65536
    # a white surround with a noisy inside: the common cell plus thousands of others
    frame = R.synthetic_frame(96, 128, surround=True, seed=3)
    assert np.array_equal(F.color_histogram(torch.from_numpy(frame).to(DEV)).cpu().numpy(), R.color_histogram(frame))
    # three frames into one table
    frames = [_pixels(n, 10 + n, kind) for n, kind in ((4097, "noise"), (300, "runs"), (65, "scattered"))]
    table, want = None, None
    for f in frames:
        table = _hist(f, out=table)
        want = R.color_histogram(f, want)
    assert np.array_equal(table.cpu().numpy(), want) and int(table[:, 0].sum()) == 4097 + 300 + 65
    with pytest.raises(ValueError):
        _hist(frames[0], out=torch.zeros((1 << 18, 4), dtype=torch.int32, device=DEV))


def _map(px_np, pal_np):
    return F.palette_map(torch.from_numpy(px_np).to(DEV), torch.from_numpy(pal_np).to(DEV)).cpu().numpy()


@pytest.mark.parametrize("k", [1, 2, 255, 256])
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 4099])
def test_palette_map_equals_restated_argmin(k, n):
    rng = np.random.default_rng(100 * k + n)
    pal = rng.integers(0, 256, (k, 3)).astype(np.uint8)
    px = _pixels(n, n + k)
    px[::3] = pal[rng.integers(0, k, px[::3].shape[0])]                  # exact hits among the pixels
    got = _map(px, pal)
    assert got.dtype == np.uint8 and got.shape == (n,)
    assert np.array_equal(got, R.palette_map(px, pal))


def test_palette_map_ties_take_the_lower_index():
    # equidistant entries: (10, 10, 10) lies between entries 0 and 1, and between 2 and 3 at a larger distance
    pal = np.array([[12, 10, 10], [8, 10, 10], [10, 14, 10], [10, 6, 10], [200, 200, 200]], dtype=np.uint8)
    px = np.array([[10, 10, 10], [10, 10, 9], [9, 10, 10], [11, 10, 10], [10, 11, 10]], dtype=np.uint8)
    assert _map(px, pal).tolist() == [0, 0, 1, 0, 0]
    assert _map(px, pal[::-1].copy()).tolist() == [3, 3, 3, 4, 3]        # the order reversed: entries 3 and 4 are 8, 12
    # duplicate entries: the first copy wins, wherever it sits
    pal = np.random.default_rng(0).integers(0, 256, (256, 3)).astype(np.uint8)
    pal[200] = pal[17]
    pal[255] = pal[3]
    px = np.concatenate([pal, pal[::-1]])[:, None, :].repeat(3, axis=1)   # (512, 3, 3): a frame-shaped input
    got = _map(px, pal)
    assert got.shape == (512, 3) and np.array_equal(got, R.palette_map(px, pal))
    assert got[200, 0] == 17 and got[255, 0] == 3 and (got[:256, 0] <= np.arange(256)).all()
    # the same permutation symmetric distances at the three channels: (5,0,0) (0,5,0) (0,0,5) (3,4,0) from the origin
    pal = np.array([[0, 0, 5], [0, 5, 0], [5, 0, 0], [3, 4, 0], [0, 3, 4]], dtype=np.uint8)
    for perm in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        assert _map(np.zeros((70, 3), dtype=np.uint8), pal[perm]).tolist() == [0] * 70


def _three_frames(lattice=False):
    rng = np.random.default_rng(8)
    if lattice:          # 200 colours in all, each alone in its cell: the palette is the colours, nothing is lost
        cell = rng.permutation(1 << 18)[:200]
        cols = (4 * np.stack([cell >> 12, (cell >> 6) & 63, cell & 63], axis=1) + rng.integers(0, 4, (200, 3))).astype(np.uint8)
        return [cols[rng.integers(0, 200, (33, 17))] for _ in range(3)]
    base = R.synthetic_frame(33, 17, seed=5)
    base[:5] = 255                                                       # a white band: one crowded cell
    return [np.roll(base, 2 * i, axis=0) ^ rng.integers(0, 8, base.shape).astype(np.uint8) for i in range(3)]


@pytest.mark.parametrize("mode", ["global", "frame"])
def test_quantize_and_write_gif_end_to_end(tmp_path, mode):
    frames = _three_frames()
    pals, ns, idx = R.quantize(frames, mode)
    assert min(ns) == 256                                                # more cells than entries: the median cut runs
    dev_frames = [torch.from_numpy(f).to(DEV) for f in frames]
    got_pals, got_idx = I.quantize_frames(dev_frames, palette=mode)
    assert len(got_pals) == len(pals) and len(got_idx) == 3
    for p, want in zip(got_pals, pals):
        assert p.dtype == torch.uint8 and tuple(p.shape) == (256, 3) and np.array_equal(p.numpy(), want)
    for x, want in zip(got_idx, idx):
        assert x.dtype == torch.uint8 and tuple(x.shape) == (33, 17) and np.array_equal(x.numpy(), want)
    path = str(tmp_path / "a.gif")
    # device frames, host frames and the quantised pair write the same file
    I.write_gif(path, dev_frames, palette=mode)
    data = open(path, "rb").read()
    I.write_gif(path, [torch.from_numpy(f) for f in frames], palette=mode)
    assert open(path, "rb").read() == data
    I.write_gif(path, (got_pals, got_idx), palette=mode)
    assert open(path, "rb").read() == data
    back = I.read_gif(path)
    assert back["delays_cs"] == [3, 3, 3] and back["loop"] == 0
    for i in range(3):
        assert np.array_equal(back["frames"][i], pals[0 if mode == "global" else i][idx[i]])


@pytest.mark.parametrize("mode", ["global", "frame"])
def test_lattice_frames_decode_exactly(tmp_path, mode):
    frames = _three_frames(lattice=True)
    path = str(tmp_path / "l.gif")
    I.write_gif(path, [torch.from_numpy(f).to(DEV) for f in frames], fps=10, loop=2, palette=mode)
    back = I.read_gif(path)
    assert back["delays_cs"] == [10, 10, 10] and back["loop"] == 2
    for f, g in zip(frames, back["frames"]):
        assert np.array_equal(f, g)


def _depth_cases():
    rng = np.random.default_rng(4)
    rand = (rng.random((37, 53)) * 9.0 + 0.5).astype(np.float32)
    nan_inf = rand.copy()
    nan_inf[3, 4] = np.nan
    nan_inf[30, 50] = np.nan
    nan_inf[10, 11] = np.inf
    both = rand.copy()
    both[0, 0], both[5, 5], both[6, 6] = np.inf, -np.inf, np.nan
    neg = (rng.standard_normal((5, 7)) * 1e-3).astype(np.float32)
    return {"random": rand, "constant": np.full((6, 8), 2.5, dtype=np.float32), "nan_and_inf": nan_inf,
            "both_infinities": both, "one_pixel": np.array([[3.0]], dtype=np.float32), "around_zero": neg,
            "large": (rng.random((129, 1031)) * 3.0).astype(np.float32)}


@pytest.mark.parametrize("name", list(_depth_cases()))
@pytest.mark.parametrize("table", ["jet", "random"])
def test_depth_colormap_equals_float32_restatement(name, table):
    d = _depth_cases()[name]
    lut = I.jet_lut().numpy() if table == "jet" else np.random.default_rng(2).integers(0, 256, (256, 3)).astype(np.uint8)
    got, rng = F.depth_colormap(torch.from_numpy(d).to(DEV), torch.from_numpy(lut), return_range=True)
    mi, ma = R.depth_range(d)
    assert rng.cpu().numpy().tobytes() == np.array([mi, ma], dtype=np.float32).tobytes()     # bit for bit
    want = R.depth_colormap(d, lut)
    assert got.dtype == torch.uint8 and tuple(got.shape) == d.shape + (3,)
    assert np.array_equal(got.cpu().numpy(), want)
    if name == "both_infinities":                                        # the stated NaN rule: the infinities take entry 0
        assert np.array_equal(want[0, 0], lut[0]) and np.array_equal(want[5, 5], lut[0])
    if name == "constant":
        assert (want == lut[0]).all()
    if table == "jet":
        pic = I.visualize_depth(torch.from_numpy(d).to(DEV))
        assert pic.dtype == torch.float32 and tuple(pic.shape) == (3,) + d.shape and pic.is_cuda
        assert np.array_equal(pic.cpu().numpy(), (want.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_validation_stack_on_the_device():
    h, w = 6, 8
    g = torch.Generator().manual_seed(1)
    gt, pred, depth = torch.rand((h * w, 3), generator=g), torch.rand((h * w, 3), generator=g), torch.rand((h, w), generator=g)
    s = I.validation_stack(gt.to(DEV), pred.to(DEV), depth.to(DEV))
    assert tuple(s.shape) == (3, 3, h, w) and not s.is_cuda
    assert torch.equal(s[0], gt.view(h, w, 3).permute(2, 0, 1)) and torch.equal(s[1], pred.view(h, w, 3).permute(2, 0, 1))
    want = R.depth_colormap(depth.numpy(), I.jet_lut().numpy()).astype(np.float32) / np.float32(255)
    assert np.array_equal(s[2].numpy(), want.transpose(2, 0, 1))


def test_evaluate_images_writes_the_gifs(tmp_path):
    """The 6 x 8 two-image setup of test_eval_image_loop_vs_oracle_deterministic: save_gif / save_depth_gif add the two
    files and nothing else; with the defaults the directory and the result are what they were."""
    from test_gpu_ssim import KW, small_model          # noqa: F401  (the shared small model of the eval-loop tests)
    h, w, focal = 6, 8, 7.5
    m, _ = small_model(61, 16, 16, noise_std=None, precision="fp32")
    m = m.eval()
    m.use_stratified_sampling = False
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.2], [0.0, 0.0, 1.0, 1.5]])
    samples = []
    for img_id in (3, 7):
        rays = F.generate_rays(h, w, focal, c2w.to(DEV), near=0.0, far=1.0, ndc=False, image_id=img_id)
        samples.append({"rays": rays, "rgbs": torch.rand((h * w, 3), generator=torch.Generator().manual_seed(img_id)).to(DEV),
                        "hw": (h, w)})
    base_dir, gif_dir, frame_dir = (str(tmp_path / d) for d in ("base", "gif", "frame"))
    base = I.evaluate_images(m, samples, chunk=20, save_dir=base_dir)
    assert sorted(os.listdir(base_dir)) == ["000.png", "001.png"]
    assert sorted(base) == ["depths", "images", "mean_psnr", "mean_ssim", "psnrs", "ssims"]
    res = I.evaluate_images(m, samples, chunk=20, save_dir=gif_dir, save_gif="s", save_depth_gif=True)
    assert sorted(os.listdir(gif_dir)) == ["000.png", "001.png", "s.gif", "s_depth.gif"]
    assert sorted(res) == sorted(base)
    for k in ("images", "depths"):
        assert all(torch.equal(a, b) for a, b in zip(res[k], base[k]))
    assert res["psnrs"] == base["psnrs"] and res["ssims"] == base["ssims"]
    frames = [x.numpy() for x in res["images"]]
    pals, ns, idx = R.quantize(frames, "global")
    back = I.read_gif(os.path.join(gif_dir, "s.gif"))
    assert len(back["frames"]) == 2 and back["delays_cs"] == [3, 3] and back["loop"] == 0
    distinct = len(set(R.keys_of(np.concatenate([f.reshape(-1, 3) for f in frames])).tolist())) == \
        len({tuple(p) for f in frames for p in f.reshape(-1, 3).tolist()})
    for i in range(2):
        assert back["frames"][i].shape == (h, w, 3)
        assert np.array_equal(back["frames"][i], pals[0][idx[i]])
        if distinct:                                                     # at most 96 colours, one per cell: lossless
            assert np.array_equal(back["frames"][i], frames[i])
    lut = I.jet_lut().numpy()
    depth_frames = [R.depth_colormap(np.asarray(d.numpy()), lut) for d in res["depths"]]
    pals_d, _, idx_d = R.quantize(depth_frames, "global")
    back_d = I.read_gif(os.path.join(gif_dir, "s_depth.gif"))
    assert len(back_d["frames"]) == 2
    for i in range(2):
        assert np.array_equal(back_d["frames"][i], pals_d[0][idx_d[i]])
    # per-frame palettes, another frame rate, the depth GIF alone
    I.evaluate_images(m, samples, chunk=20, save_dir=frame_dir, save_depth_gif=True, gif_palette="frame", gif_fps=10)
    assert sorted(os.listdir(frame_dir)) == ["000.png", "001.png", "depth.gif"]
    assert I.read_gif(os.path.join(frame_dir, "depth.gif"))["delays_cs"] == [10, 10]
    for kw in (dict(save_gif="s"), dict(save_depth_gif=True), dict(save_dir=gif_dir, save_gif="s", gif_palette="x")):
        with pytest.raises(ValueError):
            I.evaluate_images(m, samples, chunk=20, **kw)
