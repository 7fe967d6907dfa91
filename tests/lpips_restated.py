"""LPIPS v0.1 restated with torch on the CPU, float64 unless told otherwise, from its own copy of the layer tables:
test infrastructure (tests/test_lpips_host.py, tests/test_gpu_lpips.py), independent of hypernerf_torch_amd.

    x = ((2 img - 1) - shift) / scale;  backbone (conv + bias + ReLU, floor-mode max pools);  five taps after ReLUs;
    fhat = f / (sqrt(sum_c f^2) + 1e-10);  d_l = mean_pixels sum_c w_l[c] (fhat_pred - fhat_gt)^2;  LPIPS = sum_l d_l

and a seeded maker of random weights of the right shapes in both state-dict layouts the loader accepts."""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10

# ('conv', features index, cin, cout, kernel, stride, pad, tap) / ('pool', features index, kernel, stride)
ALEX = (("conv", 0, 3, 64, 11, 4, 2, True), ("pool", 2, 3, 2),
        ("conv", 3, 64, 192, 5, 1, 2, True), ("pool", 5, 3, 2),
        ("conv", 6, 192, 384, 3, 1, 1, True),
        ("conv", 8, 384, 256, 3, 1, 1, True),
        ("conv", 10, 256, 256, 3, 1, 1, True))
VGG = (("conv", 0, 3, 64, 3, 1, 1, False), ("conv", 2, 64, 64, 3, 1, 1, True), ("pool", 4, 2, 2),
       ("conv", 5, 64, 128, 3, 1, 1, False), ("conv", 7, 128, 128, 3, 1, 1, True), ("pool", 9, 2, 2),
       ("conv", 10, 128, 256, 3, 1, 1, False), ("conv", 12, 256, 256, 3, 1, 1, False),
       ("conv", 14, 256, 256, 3, 1, 1, True), ("pool", 16, 2, 2),
       ("conv", 17, 256, 512, 3, 1, 1, False), ("conv", 19, 512, 512, 3, 1, 1, False),
       ("conv", 21, 512, 512, 3, 1, 1, True), ("pool", 23, 2, 2),
       ("conv", 24, 512, 512, 3, 1, 1, False), ("conv", 26, 512, 512, 3, 1, 1, False),
       ("conv", 28, 512, 512, 3, 1, 1, True))
NETS = {"alex": ALEX, "vgg": VGG}
MIN_SIDE = {"alex": 31, "vgg": 16}


def convs_of(net):
    return [l for l in NETS[net] if l[0] == "conv"]


def tap_channels(net):
    return [l[3] for l in convs_of(net) if l[7]]


def random_weights(net, seed):
    """{'convs': [(weight (M, Cin, k, k), bias (M,))], 'lins': [(C_l,)]}, float32: He-scaled normal weights, 0.1 * normal
    biases, uniform [0, 1) lin weights, from one seeded generator."""
    g = torch.Generator().manual_seed(seed)
    convs = []
    for _, _, cin, cout, k, _, _, _ in convs_of(net):
        w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5
        b = 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
        convs.append((w.float(), b.float()))
    lins = [torch.rand(c, generator=g, dtype=torch.float64).float() for c in tap_channels(net)]
    return {"convs": convs, "lins": lins}


def split_state_dicts(net, weights):
    """(torchvision-style backbone state dict with a `classifier.*` entry, the lpips package's lin state dict)."""
    backbone, lin = {}, {}
    for layer, (w, b) in zip(convs_of(net), weights["convs"]):
        backbone[f"features.{layer[1]}.weight"] = w.clone()
        backbone[f"features.{layer[1]}.bias"] = b.clone()
    backbone["classifier.1.weight"] = torch.zeros(4, 4)
    backbone["classifier.1.bias"] = torch.zeros(4)
    for k, v in enumerate(weights["lins"]):
        lin[f"lin{k}.model.1.weight"] = v.clone().view(1, -1, 1, 1)
    return backbone, lin


def full_state_dict(net, weights):
    """A full `lpips.LPIPS(net).state_dict()`: `net.slice<k>.<i>.*`, `lin<k>.*`, their `lins.<k>.*` twins and the
    scaling layer's buffers."""
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    k = 1
    for layer, (w, b) in zip(convs_of(net), weights["convs"]):
        sd[f"net.slice{k}.{layer[1]}.weight"] = w.clone()
        sd[f"net.slice{k}.{layer[1]}.bias"] = b.clone()
        if layer[7]:
            k += 1
    for k, v in enumerate(weights["lins"]):
        sd[f"lin{k}.model.1.weight"] = v.clone().view(1, -1, 1, 1)
        sd[f"lins.{k}.model.1.weight"] = v.clone().view(1, -1, 1, 1)
    return sd


def prepare(img, dtype=torch.float64):
    img = img.to(dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    return ((2 * img - 1) - shift) / scale


def conv_layer(x, layer, w, b, relu=True):
    """One table row on `x`, in x's dtype."""
    y = F.conv2d(x, w.to(x.dtype), b.to(x.dtype), stride=layer[5], padding=layer[6])
    return F.relu(y) if relu else y


def conv_bound(x, layer, w, b):
    """conv(|x|, |w|) + |b|, float64: what the error bound of an fp32 fma chain multiplies."""
    return F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=layer[5], padding=layer[6])


def pool_layer(x, layer):
    return F.max_pool2d(x, layer[2], layer[3])


def features(net, weights, x):
    """The five taps of prepared images `x`, in x's dtype."""
    taps, ci = [], 0
    for layer in NETS[net]:
        if layer[0] == "pool":
            x = pool_layer(x, layer)
            continue
        x = conv_layer(x, layer, *weights["convs"][ci])
        ci += 1
        if layer[7]:
            taps.append(x)
    return taps


def layer_distance(fa, fb, lin):
    """(N,) of one tap: features unit-normalised over channels (epsilon added to the root), weighted squared difference
    summed over channels, mean over pixels."""
    na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    return ((na - nb).pow(2) * lin.to(fa.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_layers(net, weights, pred, gt, dtype=torch.float64):
    """(N, 5) in `dtype`: the layer terms; their sum over the second axis is LPIPS."""
    n = pred.shape[0]
    taps = features(net, weights, prepare(torch.cat([pred, gt]), dtype))
    return torch.stack([layer_distance(t[:n], t[n:], lin) for t, lin in zip(taps, weights["lins"])], dim=1)


def lpips(net, weights, pred, gt, dtype=torch.float64):
    return lpips_layers(net, weights, pred, gt, dtype).sum(1)


def image_pair(n, h, w, seed, noise=0.1):
    """(pred, gt) float32 in [0, 1]: uniform ground truth and a noisy copy."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(n, 3, h, w, generator=g, dtype=torch.float64)
    pred = (gt + noise * torch.randn(gt.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return pred.float(), gt.float()


# (net, N, H, W) of the GPU tests' final-value check; weights from WEIGHT_SEED[net], images from image_pair(seed = H * W)
CASES = (("alex", 1, 31, 31), ("alex", 2, 32, 47), ("alex", 1, 35, 64), ("vgg", 1, 16, 16), ("vgg", 2, 17, 23),
         ("alex", 1, 378, 504))
WEIGHT_SEED = {"alex": 3, "vgg": 4}


def float32_deviation(cases=CASES):
    """The worst relative deviation of this restatement run in float32 from itself in float64, over the layer terms and
    their sum of every case: the yardstick the GPU tests' tolerance is a multiple of."""
    worst = 0.0
    for net, n, h, w in cases:
        weights = random_weights(net, WEIGHT_SEED[net])
        pred, gt = image_pair(n, h, w, h * w)
        v64 = lpips_layers(net, weights, pred, gt)
        v32 = lpips_layers(net, weights, pred, gt, torch.float32).double()
        v64 = torch.cat([v64, v64.sum(1, keepdim=True)], 1)
        v32 = torch.cat([v32, v32.sum(1, keepdim=True)], 1)
        worst = max(worst, float(((v32 - v64).abs() / v64.abs()).max()))
    return worst
