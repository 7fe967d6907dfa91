"""Host tests of LPIPS (csrc/hn_lpips.hip, ops/lpips/, losses.lpips), no GPU: properties of the float64 restatement
(tests/lpips_restated.py), the strict weight loader on both state-dict layouts, the binding, the refusals of every entry
point (all of them answered on the host, before any launch) and the mirrors of the kernel file's limits."""
import ctypes as C
import os
import re

import pytest
import torch

import hypernerf_torch_amd as HN
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import losses
from hypernerf_torch_amd.ops import lpips as P

import lpips_restated as R

REFUSED = (ValueError, L.HnError)      # an argument error, or "needs the GPU", before any launch


@pytest.fixture(scope="module")
def weights():
    return {net: R.random_weights(net, R.WEIGHT_SEED[net]) for net in R.NETS}


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,h,w", [("alex", 31, 31), ("vgg", 17, 23)])
def test_identical_images_give_zero_and_the_metric_is_symmetric(weights, net, h, w):
    pred, gt = R.image_pair(2, h, w, 5)
    assert torch.equal(R.lpips(net, weights[net], gt, gt), torch.zeros(2, dtype=torch.float64))
    ab, ba = R.lpips_layers(net, weights[net], pred, gt), R.lpips_layers(net, weights[net], gt, pred)
    assert torch.equal(ab, ba) and (ab > 0).all() and torch.isfinite(ab).all()


def test_all_zero_feature_pixel_gives_zero_not_nan():
    fa = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    fb = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    lin = torch.ones(4, dtype=torch.float64)
    assert float(R.layer_distance(fa, fb, lin)) == 0.0
    fb[0, :, 0, 0] = torch.tensor([3.0, 0.0, 4.0, 0.0])      # one pixel of unit norm against a zero pixel: 1 / 4 pixels
    assert abs(float(R.layer_distance(fa, fb, lin)) - 0.25) < 1e-9
    # a whole net with one conv's bias at -10: that tap is all zeros after its ReLU and its term is exactly 0
    w = R.random_weights("alex", 3)
    w["convs"][2] = (w["convs"][2][0], torch.full_like(w["convs"][2][1], -10.0))
    pred, gt = R.image_pair(1, 31, 31, 9)
    layers = R.lpips_layers("alex", w, pred, gt)
    assert torch.isfinite(layers).all() and float(layers[0, 2]) == 0.0 and float(layers[0, 1]) > 0.0


TAP_SHAPES = [
    ("alex", 31, 31, [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]),
    ("alex", 32, 47, [(64, 7, 11), (192, 3, 5), (384, 1, 2), (256, 1, 2), (256, 1, 2)]),
    ("alex", 378, 504, [(64, 93, 125), (192, 46, 62), (384, 22, 30), (256, 22, 30), (256, 22, 30)]),
    ("vgg", 16, 16, [(64, 16, 16), (128, 8, 8), (256, 4, 4), (512, 2, 2), (512, 1, 1)]),
    ("vgg", 17, 23, [(64, 17, 23), (128, 8, 11), (256, 4, 5), (512, 2, 2), (512, 1, 1)]),
]


@pytest.mark.parametrize("net,h,w,want", TAP_SHAPES)
def test_tap_shapes(weights, net, h, w, want):
    taps = R.features(net, weights[net], R.prepare(torch.rand(1, 3, h, w), torch.float32))
    assert [tuple(t.shape[1:]) for t in taps] == want
    # the host's own shape arithmetic walks the same table to the same shapes
    got, side = [], (h, w)
    for layer in P.lpips_net(net):
        k, s, p = (layer[4], layer[5], layer[6]) if layer[0] == "conv" else (layer[2], layer[3], 0)
        side = tuple(P._out_side(v, k, s, p) for v in side)
        if layer[0] == "conv" and layer[7]:
            got.append((layer[3],) + side)
    assert got == want


def test_min_sides_are_the_smallest_legal_sides(weights):
    for net in R.NETS:
        side = R.MIN_SIDE[net]
        assert P.lpips_min_side(net) == side
        assert len(R.features(net, weights[net], torch.zeros(1, 3, side, side, dtype=torch.float32))) == 5
        with pytest.raises(RuntimeError):      # one pixel less: the last pool has no output left
            R.features(net, weights[net], torch.zeros(1, 3, side, side - 1, dtype=torch.float32))
    with pytest.raises(ValueError):
        P.lpips_min_side("squeeze")


def test_layer_table_equals_the_restatements():
    for net in R.NETS:
        assert tuple(P.lpips_net(net)) == tuple(R.NETS[net])
        assert list(P.lpips_tap_channels(net)) == R.tap_channels(net)
    with pytest.raises(ValueError):
        P.lpips_net("squeeze")
    assert P.LPIPS_SHIFT == R.SHIFT and P.LPIPS_SCALE == R.SCALE


# ---- the loader -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_both_layouts_give_identical_packed_weights(weights, net, tmp_path):
    backbone, lin = R.split_state_dicts(net, weights[net])
    full = R.full_state_dict(net, weights[net])
    a = P.lpips_weights_from_state_dicts(net, backbone, lin)
    b = P.lpips_weights_from_state_dicts(net, full)
    assert a.net == b.net == net and a.device == torch.device("cpu") and a.to("cpu") is a
    assert len(a.tensors()) == len(b.tensors()) == 3 * len(R.convs_of(net)) + 5
    for x, y in zip(a.tensors(), b.tensors()):
        assert x.dtype == y.dtype and torch.equal(x, y)
    # the packing: wt[k][m] = weight[m].flatten()[k], zero padding, and the k table's (ci, ky, kx)
    for (wt, ktab, bias), layer, (w, bvec) in zip(a.convs, R.convs_of(net), weights[net]["convs"]):
        m, cin, k = layer[3], layer[2], layer[4]
        kk = cin * k * k
        assert wt.shape == (-(-kk // P.LPIPS_BK) * P.LPIPS_BK, -(-m // P.LPIPS_MPAD) * P.LPIPS_MPAD)
        assert torch.equal(wt[:kk, :m], w.reshape(m, kk).t()) and not wt[kk:].any() and not wt[:, m:].any()
        assert torch.equal(bias, bvec) and ktab.dtype == torch.int32 and ktab.shape == (wt.shape[0],)
        idx = torch.arange(kk)
        assert torch.equal(ktab[:kk].long(), (idx // (k * k)) * 256 + ((idx // k) % k) * 16 + idx % k)
        assert (ktab[kk:] == -1).all()
    for lin_vec, want in zip(a.lins, weights[net]["lins"]):
        assert torch.equal(lin_vec, want)
    # through files, as load_lpips_weights reads them
    torch.save(backbone, tmp_path / "backbone.pth")
    torch.save(lin, tmp_path / "lin.pth")
    torch.save(full, tmp_path / "full.pth")
    for c in (P.load_lpips_weights(net, tmp_path / "backbone.pth", tmp_path / "lin.pth"),
              P.load_lpips_weights(net, tmp_path / "full.pth"),
              losses.load_lpips(net, tmp_path / "full.pth", device="cpu")):
        assert all(torch.equal(x, y) for x, y in zip(a.tensors(), c.tensors()))


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_every_missing_or_misshaped_key_is_named(weights, net):
    backbone, lin = R.split_state_dicts(net, weights[net])
    full = R.full_state_dict(net, weights[net])
    needed_split = [k for k in backbone if k.startswith("features.")]
    needed_full = [k for k in full if k.startswith("net.") or re.match(r"lin\d\.", k)]
    assert len(needed_split) == 2 * len(R.convs_of(net)) and len(lin) == 5 and len(needed_full) == len(needed_split) + 5

    def variants(sd, key):
        t = sd[key]
        yield {k: v for k, v in sd.items() if k != key}                           # missing
        yield {**sd, key: t.reshape(-1)[:-1].clone()}                               # mis-shaped
        yield {**sd, key: t.unsqueeze(0).clone()}
        yield {**sd, key: t.double()}                                               # wrong dtype

    for key in needed_split:
        for bad in variants(backbone, key):
            with pytest.raises(ValueError, match=re.escape(f"'{key}'")):
                P.lpips_weights_from_state_dicts(net, bad, lin)
    for key in lin:
        for bad in variants(lin, key):
            with pytest.raises(ValueError, match=re.escape(f"'{key}'")):
                P.lpips_weights_from_state_dicts(net, backbone, bad)
    for key in needed_full:
        for bad in variants(full, key):
            with pytest.raises(ValueError, match=re.escape(f"'{key}'")):
                P.lpips_weights_from_state_dicts(net, bad)
    with pytest.raises(ValueError):
        P.lpips_weights_from_state_dicts("squeeze", backbone, lin)
    other = "vgg" if net == "alex" else "alex"
    with pytest.raises(ValueError):      # the other net's files
        P.lpips_weights_from_state_dicts(other, backbone, lin)


def test_tolerated_and_refused_extras(weights):
    w = weights["alex"]
    backbone, lin = R.split_state_dicts("alex", w)
    full = R.full_state_dict("alex", w)
    assert any(k.startswith("classifier.") for k in backbone) and any(k.startswith("lins.") for k in full)
    assert "scaling_layer.shift" in full and "scaling_layer.scale" in full
    base = P.lpips_weights_from_state_dicts("alex", full)
    bare = {k: v for k, v in full.items() if not k.startswith(("lins.", "scaling_layer."))}
    for x, y in zip(base.tensors(), P.lpips_weights_from_state_dicts("alex", bare).tensors()):
        assert torch.equal(x, y)
    for name in ("shift", "scale"):
        bad = dict(full)
        bad[f"scaling_layer.{name}"] = full[f"scaling_layer.{name}"] + 0.001
        with pytest.raises(ValueError, match=f"scaling_layer.{name}"):
            P.lpips_weights_from_state_dicts("alex", bad)


# ---- binding, mirrors, refusals ---------------------------------------------------------------------------------------------
ENTRIES = {"hn_lpips_prepare": 10, "hn_lpips_conv": 16, "hn_lpips_maxpool": 8, "hn_lpips_workspace_bytes": 4,
           "hn_lpips_distance": 10}


def test_binding_knows_the_new_entries():
    lib = L.load()
    assert lib.hn_version() == 340
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and len(L.ARGTYPES[name]) == nargs and hasattr(lib, name)
    assert "hn_lpips.hip" in L.SOURCES and "hn_lpips.hip" in HN.ops.__doc__
    for name in P.__all__:
        assert getattr(HN.functional, name) is getattr(P, name)
    for name in ("lpips_net", "LpipsWeights", "lpips_weights_from_state_dicts", "load_lpips_weights", "lpips_min_side",
                 "lpips_features", "lpips_layers"):
        assert name in P.__all__
    assert callable(losses.lpips) and callable(losses.load_lpips)


def test_limit_macros_equal_their_python_mirrors():
    src = open(os.path.join(L.CSRC, "hn_lpips.hip")).read()
    macros = {k: int(v) for k, v in re.findall(r"^#define HN_LPIPS_(\w+) (\d+)", src, flags=re.M)}
    assert macros == {"BK": P.LPIPS_BK, "MPAD": P.LPIPS_MPAD, "MAX_KERNEL": P.LPIPS_MAX_KERNEL,
                      "MAX_CHANNELS": P.LPIPS_MAX_CHANNELS, "ALEX_MIN_SIDE": P.lpips_min_side("alex"),
                      "VGG_MIN_SIDE": P.lpips_min_side("vgg"), "LAYERS": P.LPIPS_LAYERS,
                      "DIST_PIXELS": P.LPIPS_DIST_PIXELS, "DIST_GROUPS": 16, "SUM_THREADS": 256,
                      "FILL_BLOCKS": 256}
    assert not re.search(r"HN_LPIPS", open(L.HEADER).read())      # the header's set of macros is pinned at ABI 340


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 16, 16), (2, 7, 11), (1, 93, 125), (3, 378, 504), (1, 16, 17)])
def test_workspace_bytes_equal_the_python_mirror(n, h, w):
    nbytes = C.c_int64(-1)
    assert L.load().hn_lpips_workspace_bytes(n, h, w, C.byref(nbytes)) == 0
    assert nbytes.value == P.lpips_workspace_bytes(n, h, w) and nbytes.value % 16 == 0 and nbytes.value >= 4 * n


def test_every_refusal_is_answered_before_any_launch():
    """-2 from the host checks of every entry point.  The pointers below are not device memory (this machine may have
    no GPU at all): a call that got as far as a launch could not return -2."""
    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    st = (C.c_int64 * 4)(1, 1, 1, 1)
    nbytes = C.c_int64(0)
    for args in ((0, 4, 4, C.byref(nbytes)), (1, 0, 4, C.byref(nbytes)), (1, 4, -1, C.byref(nbytes)), (1, 4, 4, None),
                 (2, 40000, 40000, C.byref(nbytes))):
        assert lib.hn_lpips_workspace_bytes(*args) == -2, args

    def prepare(pred=p, ps=st, gt=p, gs=st, n=1, h=31, w=31, net=0, out=p):
        return lib.hn_lpips_prepare(pred, ps, gt, gs, n, h, w, net, out, None)
    for kw in (dict(pred=None), dict(ps=None), dict(gt=None), dict(gs=None), dict(out=None), dict(n=0), dict(n=-1),
               dict(h=0), dict(w=0), dict(net=2), dict(net=-1), dict(h=30), dict(w=30), dict(net=1, h=15, w=16),
               dict(net=1, h=16, w=15), dict(n=4, h=20000, w=20000)):
        assert prepare(**kw) == -2, kw

    def conv(x=p, wt=p, bias=p, ktab=p, y=p, imgs=1, cin=3, h=8, w=8, cout=4, k=3, s=1, pad=1, relu=1, tile=0):
        return lib.hn_lpips_conv(x, wt, bias, ktab, y, imgs, cin, h, w, cout, k, s, pad, relu, tile, None)
    for kw in (dict(x=None), dict(wt=None), dict(bias=None), dict(ktab=None), dict(y=None), dict(imgs=0), dict(cin=0),
               dict(h=0), dict(w=-3), dict(cout=0), dict(k=0), dict(k=P.LPIPS_MAX_KERNEL + 1), dict(s=0), dict(pad=-1),
               dict(pad=3), dict(tile=4), dict(tile=-1), dict(cin=P.LPIPS_MAX_CHANNELS + 1),
               dict(cout=P.LPIPS_MAX_CHANNELS + 1), dict(h=2, w=2, k=11, pad=2), dict(imgs=64, cin=64, h=1024, w=1024),
               dict(imgs=64, cout=64, h=1024, w=1024)):
        assert conv(**kw) == -2, kw

    def pool(x=p, y=p, planes=1, h=8, w=8, k=2, s=2):
        return lib.hn_lpips_maxpool(x, y, planes, h, w, k, s, None)
    for kw in (dict(x=None), dict(y=None), dict(planes=0), dict(h=0), dict(w=0), dict(k=0), dict(s=0), dict(h=2, k=3),
               dict(k=P.LPIPS_MAX_KERNEL + 1), dict(planes=4096, h=1024, w=1024)):
        assert pool(**kw) == -2, kw

    def dist(feat=p, lin=p, n=1, c=4, h=2, w=2, layer=0, out=p, ws=p):
        return lib.hn_lpips_distance(feat, lin, n, c, h, w, layer, out, ws, None)
    for kw in (dict(feat=None), dict(lin=None), dict(out=None), dict(ws=None), dict(n=0), dict(c=0), dict(h=0), dict(w=0),
               dict(layer=-1), dict(layer=P.LPIPS_LAYERS), dict(c=P.LPIPS_MAX_CHANNELS + 1), dict(n=65536),
               dict(n=8, c=512, h=1024, w=1024)):
        assert dist(**kw) == -2, kw


def test_python_refusals_without_a_gpu(weights):
    w = P.lpips_weights_from_state_dicts("alex", *R.split_state_dicts("alex", weights["alex"]))
    a, b = R.image_pair(1, 31, 31, 1)
    for call in (lambda: losses.lpips(a, b, w),                                  # CPU tensors
                 lambda: losses.lpips(a, b, w, reduction="sum"),
                 lambda: losses.lpips(a, b, "alex"),
                 lambda: losses.lpips(a[:, :2], b[:, :2], w),
                 lambda: losses.lpips(a.double(), b.double(), w),
                 lambda: losses.lpips(a[..., :30], b[..., :30], w),
                 lambda: losses.lpips(a, b[..., :30], w),
                 lambda: P.lpips_features(a, w)):
        with pytest.raises(REFUSED):
            call()
