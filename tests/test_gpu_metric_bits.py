"""GPU test (MI355X): the SSIM and MS-SSIM kernels give the bits recorded in tests/golden/metric_bits.json.

The library builds with -ffp-contract=off and neither metric uses a float atomic, so the outputs are a function of the
inputs, the window weights and the ORDER of the kernels' float operations alone; a re-arrangement of the kernels' source
that keeps that order keeps every bit.  The inputs come from tests/hashprng.py (exact on any machine).  The fixture
holds the sha256 of the raw bytes of every output, and under "windows" the sha256 of the fp32 weights the host hands to
the kernels (ssim_window(w), the 5 x 11 MS-SSIM taps of a shape): a host whose exp() rounds differently shows there, by
name, and not as a kernel change.

`python tests/test_gpu_metric_bits.py --record` writes the fixture from the library in use (HN_LIB_PATH selects a
prebuilt one).  Record it from the commit whose bits are to be kept, never from the code under test."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":      # run as a script: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hashprng as H
from gpu_common import DEV
from hypernerf_torch_amd.ops import metrics as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_bits.json")
SEED = 77

# the smallest shapes that reach each path: (1,3,2,2) w3 reflects every tap; (1,3,17,33) is one partial tile in both
# directions (w 9 and 15 are only built for, never the default of any caller); (2,3,63,64) has several tiles, two images
# and more than one slot for the partial-sum launch
SSIM_FORWARD = ([((1, 3, 2, 2), 3, "contiguous")]
                + [((1, 3, 17, 33), w, layout) for w in (3, 9, 11, 15) for layout in ("contiguous", "hwc")]
                + [((2, 3, 63, 64), 7, "contiguous")])
SSIM_BACKWARD = [((1, 3, 17, 33), w) for w in (3, 11, 15)] + [((2, 3, 63, 64), 7)]
# (1,3,5,7): every level below size 11 (the run-time-count build); (2,3,37,53): level 0 on the unrolled size-11 build,
# odd sides at every halving, two images in the final launch
MSSSIM = [((1, 3, 5, 7), "contiguous"), ((2, 3, 37, 53), "contiguous"), ((2, 3, 37, 53), "hwc"),
          ((1, 1, 64, 48), "contiguous")]


def _sid(shape):
    return "x".join(map(str, shape))


def _sha(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def _pair(shape, layout="contiguous"):
    out = []
    for name in ("x", "y"):
        t = H.uniform(SEED, f"metric bits {name} {_sid(shape)}", shape, 0, 1)
        if layout == "hwc":
            out.append(t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2))
        else:
            out.append(t.to(DEV))
    return out


def _ssim_forward(shape, w, layout):
    x, y = _pair(shape, layout)
    return {"map": _sha(M.ssim_dssim(x, y, w, reduction="none")), "sum": _sha(M.ssim_dssim(x, y, w, reduction="sum"))}


def _ssim_backward(shape, w):
    out = {}
    up = H.uniform(SEED, f"metric bits upstream {_sid(shape)}", shape, -0.3, 0.7).to(DEV)
    for reduction in ("sum", "none"):
        x, y = (t.requires_grad_() for t in _pair(shape))
        M.ssim_dssim(x, y, w, reduction=reduction).backward(up if reduction == "none" else None)
        out[f"{reduction} d_pred"], out[f"{reduction} d_gt"] = _sha(x.grad), _sha(y.grad)
    for which in ("pred", "gt"):
        x, y = _pair(shape)
        x.requires_grad_(which == "pred")
        y.requires_grad_(which == "gt")
        M.ssim_dssim(x, y, w, reduction="sum").backward()
        assert (y if which == "pred" else x).grad is None
        out[f"only d_{which}"] = _sha((x if which == "pred" else y).grad)
    return out


def _msssim(shape, layout):
    x, y = _pair(shape, layout)
    return {"levels": _sha(M.msssim_levels(x, y))}


CASES = {}
for _s, _w, _l in SSIM_FORWARD:
    CASES[f"ssim forward {_sid(_s)} w{_w} {_l}"] = (_ssim_forward, (_s, _w, _l))
for _s, _w in SSIM_BACKWARD:
    CASES[f"ssim backward {_sid(_s)} w{_w}"] = (_ssim_backward, (_s, _w))
for _s, _l in MSSSIM:
    CASES[f"msssim {_sid(_s)} {_l}"] = (_msssim, (_s, _l))


def _windows():
    """sha256 of the fp32 weights the host passes to the kernels, by name."""
    out = {f"ssim_window {w}": _sha(M.ssim_window(w).float()) for w in sorted({c[1] for c in SSIM_FORWARD})}
    for shape in sorted({c[0] for c in MSSSIM}):
        taps = M._msssim_plan(*shape)[0]
        out[f"msssim taps {_sid(shape)}"] = _sha(np.ctypeslib.as_array(taps).astype(np.float32))
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_metric_window_bits():
    """The host's window weights are the recorded ones: when this fails, the mismatches below are the host's exp()."""
    assert _windows() == _golden()["windows"]


@pytest.mark.parametrize("name", list(CASES))
def test_metric_bits(name):
    fn, args = CASES[name]
    got, want = fn(*args), _golden()["outputs"][name]
    assert got == want, {k: (got[k], want.get(k)) for k in got if got[k] != want.get(k)}


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_gpu_metric_bits.py --record")
    rec = {"windows": _windows(), "outputs": {name: fn(*args) for name, (fn, args) in CASES.items()}}
    torch.cuda.synchronize()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec['outputs'])} cases and {len(rec['windows'])} windows to {GOLDEN}")
