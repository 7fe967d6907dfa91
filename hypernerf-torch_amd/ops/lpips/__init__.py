"""LPIPS v0.1 on the GPU (csrc/hn_lpips.hip): the layer tables of the two backbones, the strict weight loader and the
per-layer launches.  The definition is DESIGN.md 3.14's; tests/lpips_restated.py restates it in float64.

The trained weights are the user's files: nothing here fetches or ships any."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from ... import _lib as L
from ..metrics import _check_pair

__all__ = ["LPIPS_NETS", "LPIPS_SHIFT", "LPIPS_SCALE", "LPIPS_LAYERS", "LPIPS_BK", "LPIPS_MPAD", "LPIPS_MAX_KERNEL",
           "LPIPS_MAX_CHANNELS", "LPIPS_DIST_PIXELS", "lpips_net", "lpips_min_side", "lpips_tap_channels",
           "lpips_workspace_bytes", "LpipsWeights", "lpips_weights_from_state_dicts", "load_lpips_weights",
           "lpips_prepare", "lpips_conv", "lpips_maxpool", "lpips_features", "lpips_layers"]

LPIPS_NETS = ("alex", "vgg")
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
# mirrors of csrc/hn_lpips.hip's macros (no HN_* macro in the header: tests/test_lpips_host.py compares them)
LPIPS_LAYERS = 5
LPIPS_BK = 64
LPIPS_MPAD = 128
LPIPS_MAX_KERNEL = 15
LPIPS_MAX_CHANNELS = 4096
LPIPS_DIST_PIXELS = 64
_MIN_SIDE = {"alex": 31, "vgg": 16}


def _vgg_table():
    table, cin, index = [], 3, 0
    for block, (convs, width) in enumerate(((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))):
        if block:
            table.append(("pool", index, 2, 2))
            index += 1
        for j in range(convs):
            table.append(("conv", index, cin, width, 3, 1, 1, j == convs - 1))
            cin = width
            index += 2          # the conv and its ReLU
    return tuple(table)


_TABLES = {
    "alex": (("conv", 0, 3, 64, 11, 4, 2, True), ("pool", 2, 3, 2), ("conv", 3, 64, 192, 5, 1, 2, True), ("pool", 5, 3, 2),
             ("conv", 6, 192, 384, 3, 1, 1, True), ("conv", 8, 384, 256, 3, 1, 1, True),
             ("conv", 10, 256, 256, 3, 1, 1, True)),
    "vgg": _vgg_table(),
}


def _check_net(net):
    if net not in LPIPS_NETS:
        raise ValueError(f"lpips: net must be 'alex' or 'vgg', got {net!r}")


def lpips_net(name: str) -> tuple:
    """The backbone up to its last tap, in order: ('conv', i, cin, cout, kernel, stride, pad, tap) — a convolution with
    bias and zero padding followed by a ReLU, `tap` telling whether the ReLU's output is one of the five feature maps —
    and ('pool', i, kernel, stride), a floor-mode max pool without padding.  i is the module's index in torchvision's
    `features` (the number in the state-dict keys)."""
    _check_net(name)
    return _TABLES[name]


def lpips_min_side(net: str) -> int:
    """The smallest H and W the net accepts (31 for 'alex', 16 for 'vgg'): every tap then has at least one pixel."""
    _check_net(net)
    return _MIN_SIDE[net]


def lpips_tap_channels(net: str) -> Tuple[int, ...]:
    return tuple(l[3] for l in lpips_net(net) if l[0] == "conv" and l[7])


def _slice_of(net: str) -> Dict[int, int]:
    """{features index of a conv: the number k of the `net.slice<k>` that holds it in a full lpips state dict}."""
    out, k = {}, 1
    for layer in lpips_net(net):
        if layer[0] == "conv":
            out[layer[1]] = k
            if layer[7]:
                k += 1
    return out


def lpips_workspace_bytes(n: int, h: int, w: int) -> int:
    """hn_lpips_workspace_bytes in Python: one partial sum per 64 pixels of every pair of an (h, w) tap, in floats,
    rounded up to 16 bytes."""
    return (n * (-(-(h * w) // LPIPS_DIST_PIXELS)) * 4 + 15) // 16 * 16


def _pack_conv(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wt [Kpad][Mpad] fp32, ktab [Kpad] int32) of an (M, Cin, k, k) weight: transposed so that k = (ci * k + ky) * k + kx
    is the row, zero rows up to a multiple of LPIPS_BK, zero columns up to a multiple of LPIPS_MPAD."""
    m, cin, k, _ = weight.shape
    kk = cin * k * k
    kpad, mpad = -(-kk // LPIPS_BK) * LPIPS_BK, -(-m // LPIPS_MPAD) * LPIPS_MPAD
    wt = torch.zeros((kpad, mpad), dtype=torch.float32)
    wt[:kk, :m] = weight.reshape(m, kk).t()
    idx = torch.arange(kk, dtype=torch.int64)
    ktab = torch.full((kpad,), -1, dtype=torch.int32)
    ktab[:kk] = ((idx // (k * k)) << 8 | ((idx // k) % k) << 4 | (idx % k)).to(torch.int32)
    return wt.contiguous(), ktab


class LpipsWeights:
    """The frozen weights of one LPIPS net on one device, laid out once for the kernels: per convolution the packed
    weights, the k table and the bias, and the five lin vectors.  `to(device)` returns the copy on that device (made at the
    first request and kept)."""

    def __init__(self, net: str, convs: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]], lins: List[torch.Tensor]):
        _check_net(net)
        self.net, self.convs, self.lins = net, convs, lins
        self.device = lins[0].device
        self._copies: Dict[torch.device, "LpipsWeights"] = {self.device: self}

    def to(self, device) -> "LpipsWeights":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        copy = self._copies.get(device)
        if copy is None:
            copy = LpipsWeights(self.net, [tuple(t.to(device) for t in conv) for conv in self.convs],
                                [t.to(device) for t in self.lins])
            copy._copies = self._copies
            self._copies[device] = copy
        return copy

    def tensors(self) -> List[torch.Tensor]:
        return [t for conv in self.convs for t in conv] + list(self.lins)


def _take(sd, key, shape, where):
    t = sd.get(key)
    if t is None:
        raise ValueError(f"lpips weights: {where} has no key '{key}'")
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"lpips weights: '{key}' must have shape {tuple(shape)}, got {got}")
    if t.dtype != torch.float32:
        raise ValueError(f"lpips weights: '{key}' must be float32, got {t.dtype}")
    return t.detach().cpu()


def lpips_weights_from_state_dicts(net: str, backbone_sd, lin_sd=None) -> LpipsWeights:
    """The weights of `net` from state dicts, on the CPU (`.to(device)` moves them).  Two layouts:

      backbone_sd = torchvision's alexnet / vgg16 state dict (`features.<i>.weight|bias`; `classifier.*` is ignored) and
      lin_sd = the lpips package's weights/v0.1/{alex,vgg}.pth (`lin<k>.model.1.weight`, (1, C_k, 1, 1), k = 0 .. 4);

      backbone_sd = a full `lpips.LPIPS(net=...).state_dict()` (`net.slice<k>.<i>.weight|bias`, `lin<k>.model.1.weight`)
      and lin_sd = None; `scaling_layer.shift|scale`, if present, must hold this module's constants.

    Strict: a missing key, a wrong shape or a dtype other than float32 raises ValueError naming the key.  Keys the metric
    does not use (`classifier.*`, the duplicates under `lins.*`) are not looked at."""
    _check_net(net)
    full = lin_sd is None
    slices = _slice_of(net)
    convs = []
    for layer in lpips_net(net):
        if layer[0] != "conv":
            continue
        _, i, cin, cout, k = layer[:5]
        stem = f"net.slice{slices[i]}.{i}" if full else f"features.{i}"
        where = "the lpips state dict" if full else "the backbone state dict"
        weight = _take(backbone_sd, stem + ".weight", (cout, cin, k, k), where)
        bias = _take(backbone_sd, stem + ".bias", (cout,), where)
        convs.append(_pack_conv(weight) + (bias.clone().contiguous(),))
    src = backbone_sd if full else lin_sd
    lins = [_take(src, f"lin{k}.model.1.weight", (1, c, 1, 1), "the lpips state dict" if full else "the lin state dict")
            .reshape(c).clone().contiguous() for k, c in enumerate(lpips_tap_channels(net))]
    for name, want in (("shift", LPIPS_SHIFT), ("scale", LPIPS_SCALE)):
        key = f"scaling_layer.{name}"
        if full and key in backbone_sd:
            got = backbone_sd[key]
            if not isinstance(got, torch.Tensor) or got.numel() != 3 or \
                    not torch.equal(got.detach().cpu().reshape(3).float(), torch.tensor(want, dtype=torch.float32)):
                raise ValueError(f"lpips weights: '{key}' differs from the constants of LPIPS v0.1 {want}")
    return LpipsWeights(net, convs, lins)


def load_lpips_weights(net: str, backbone_path, lin_path=None) -> LpipsWeights:
    """lpips_weights_from_state_dicts of the user's files: `backbone_path` a torchvision checkpoint and `lin_path` the lpips
    package's lin weights, or `backbone_path` alone a saved `lpips.LPIPS(...).state_dict()`.  Read with
    torch.load(weights_only=True, map_location='cpu'); nothing is downloaded."""
    _check_net(net)
    backbone_sd = torch.load(backbone_path, weights_only=True, map_location="cpu")
    lin_sd = None if lin_path is None else torch.load(lin_path, weights_only=True, map_location="cpu")
    for name, sd in (("backbone_path", backbone_sd), ("lin_path", lin_sd)):
        if sd is not None and not isinstance(sd, dict):
            raise ValueError(f"load_lpips_weights: {name} does not hold a state dict but a {type(sd).__name__}")
    return lpips_weights_from_state_dicts(net, backbone_sd, lin_sd)


# --------------------------------------------------------------------------------------------
# launches
# --------------------------------------------------------------------------------------------
def _out_side(side: int, kernel: int, stride: int, pad: int) -> int:
    span = side + 2 * pad - kernel
    return 0 if span < 0 else span // stride + 1


def _check_weights(name, weights, device):
    if not isinstance(weights, LpipsWeights):
        raise ValueError(f"{name}: weights must be an LpipsWeights (losses.load_lpips), got {type(weights).__name__}")
    if weights.device != device:
        raise ValueError(f"{name}: the weights are on {weights.device} and the images on {device} "
                         "(weights.to(device) gives the copy to use)")


def _check_side(name, net, h, w):
    if h < _MIN_SIDE[net] or w < _MIN_SIDE[net]:
        raise ValueError(f"{name}: '{net}' needs H and W of at least {_MIN_SIDE[net]}, got {h} x {w}")


def _check_images(pred, gt, net):
    _check_net(net)
    _check_pair("lpips", pred, gt)
    if pred.shape[1] != 3:
        raise ValueError(f"lpips: images must have 3 channels, got {pred.shape[1]}")
    _check_side("lpips", net, pred.shape[2], pred.shape[3])
    L.require_gpu(pred, gt)
    if pred.device != gt.device:
        raise ValueError(f"lpips: pred is on {pred.device} and gt on {gt.device}")


def lpips_prepare(pred: torch.Tensor, gt: torch.Tensor, net: str) -> torch.Tensor:
    """(2N, 3, H, W) fp32: pred's images, then gt's, each value ((2 v - 1) - shift) / scale (hn_lpips_prepare).  pred / gt:
    (N, 3, H, W) fp32 on the GPU, any element strides."""
    _check_images(pred, gt, net)
    x, y = pred.detach(), gt.detach()
    n, _, h, w = x.shape
    out = torch.empty((2 * n, 3, h, w), dtype=torch.float32, device=x.device)
    L.launch("hn_lpips_prepare", L.ptr(x), (C.c_int64 * 4)(*x.stride()), L.ptr(y), (C.c_int64 * 4)(*y.stride()), n, h, w,
             LPIPS_NETS.index(net), L.ptr(out), L.stream_handle())
    return out


def lpips_conv(x: torch.Tensor, conv, kernel: int, stride: int, pad: int, relu: bool = True, tile: int = 0,
               tag: str = "") -> torch.Tensor:
    """relu(conv2d(x) + bias) of contiguous (B, Cin, H, W) fp32 `x` by hn_lpips_conv; conv = (wt, ktab, bias) of an
    LpipsWeights.  tile: 0 lets the kernel pick its tile shape, 1 / 2 / 3 force one (the bits do not depend on it).
    tag: the launch's name in L.KERNEL_TIMES (tools/lpips_bench.py)."""
    wt, ktab, bias = conv
    L.require_gpu(x, wt)
    b, cin, h, w = x.shape
    cout = bias.shape[0]
    oh, ow = _out_side(h, kernel, stride, pad), _out_side(w, kernel, stride, pad)
    if oh < 1 or ow < 1 or not x.is_contiguous() or x.dtype != torch.float32:
        raise ValueError(f"lpips_conv: a contiguous float32 input with an output of at least 1 x 1, got {tuple(x.shape)}")
    kpad, mpad = -(-cin * kernel * kernel // LPIPS_BK) * LPIPS_BK, -(-cout // LPIPS_MPAD) * LPIPS_MPAD
    if tuple(wt.shape) != (kpad, mpad) or tuple(ktab.shape) != (kpad,) or not wt.is_contiguous() or wt.device != x.device:
        raise ValueError(f"lpips_conv: the packed weights {tuple(wt.shape)} do not belong to a {cin} -> {cout} convolution "
                         f"of kernel {kernel} on {x.device}")
    y = torch.empty((b, cout, oh, ow), dtype=torch.float32, device=x.device)
    L.launch("hn_lpips_conv", L.ptr(x), L.ptr(wt), L.ptr(bias), L.ptr(ktab), L.ptr(y), b, cin, h, w, cout, kernel, stride,
             pad, int(relu), tile, L.stream_handle(), tag=tag)
    return y


def lpips_maxpool(x: torch.Tensor, kernel: int, stride: int, tag: str = "") -> torch.Tensor:
    """Floor-mode max pool without padding of contiguous (B, C, H, W) fp32 `x` (hn_lpips_maxpool)."""
    L.require_gpu(x)
    b, c, h, w = x.shape
    oh, ow = _out_side(h, kernel, stride, 0), _out_side(w, kernel, stride, 0)
    if oh < 1 or ow < 1 or not x.is_contiguous() or x.dtype != torch.float32:
        raise ValueError(f"lpips_maxpool: a contiguous float32 input with an output of at least 1 x 1, got {tuple(x.shape)}")
    y = torch.empty((b, c, oh, ow), dtype=torch.float32, device=x.device)
    L.launch("hn_lpips_maxpool", L.ptr(x), L.ptr(y), b * c, h, w, kernel, stride, L.stream_handle(), tag=tag)
    return y


def _forward(x: torch.Tensor, weights: LpipsWeights, on_tap):
    conv_i = tap_i = 0
    for layer in lpips_net(weights.net):
        if layer[0] == "pool":
            x = lpips_maxpool(x, layer[2], layer[3], tag=str(layer[1]))
            continue
        x = lpips_conv(x, weights.convs[conv_i], layer[4], layer[5], layer[6], tag=str(layer[1]))
        conv_i += 1
        if layer[7]:
            on_tap(tap_i, x)
            tap_i += 1


@torch.no_grad()
def lpips_features(x: torch.Tensor, weights: LpipsWeights) -> List[torch.Tensor]:
    """The five tap tensors (B, C_l, H_l, W_l) of PREPARED images `x` (B, 3, H, W) (lpips_prepare's output, or any
    contiguous fp32 batch in the scaled domain)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError("lpips_features: x must be a float32 (B, 3, H, W) tensor")
    L.require_gpu(x)
    _check_weights("lpips_features", weights, x.device)
    _check_side("lpips_features", weights.net, x.shape[2], x.shape[3])
    taps: List[Optional[torch.Tensor]] = [None] * LPIPS_LAYERS
    _forward(x.detach().contiguous(), weights, lambda l, t: taps.__setitem__(l, t))
    return taps


@torch.no_grad()
def lpips_layers(pred: torch.Tensor, gt: torch.Tensor, weights: LpipsWeights) -> torch.Tensor:
    """(N, 5) fp32: per image pair the five layer terms of LPIPS (their sum is the metric).  pred / gt: (N, 3, H, W) fp32
    in [0, 1] on the GPU, any element strides, sides of at least lpips_min_side.  Both images run through the backbone as
    one batch of 2N; every launch is deterministic, so the result is the same bits run to run, and the same bits for an
    image pair whatever else is in the batch.  A metric: the result carries no gradient."""
    if not isinstance(weights, LpipsWeights):
        raise ValueError(f"lpips: weights must be an LpipsWeights (losses.load_lpips), got {type(weights).__name__}")
    _check_images(pred, gt, weights.net)
    _check_weights("lpips", weights, pred.device)
    x = lpips_prepare(pred, gt, weights.net)
    n = pred.shape[0]
    out = torch.empty((n, LPIPS_LAYERS), dtype=torch.float32, device=x.device)

    def distance(l, feat):
        _, c, h, w = feat.shape
        ws = torch.empty(lpips_workspace_bytes(n, h, w) // 4, dtype=torch.float32, device=x.device)
        L.launch("hn_lpips_distance", L.ptr(feat), L.ptr(weights.lins[l]), n, c, h, w, l, L.ptr(out), L.ptr(ws),
                 L.stream_handle(), tag=str(l))

    _forward(x, weights, distance)
    return out
