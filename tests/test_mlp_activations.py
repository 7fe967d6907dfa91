"""LeakyReLU / ELU / Softplus hidden layers and wide outputs of the MLP machine — the CPU side: construction, what
stays refused, the op words the host compiler emits, and a plain torch restatement pinned against the g18 fixture."""
import numpy as np
import pytest
import torch

from act_common import ACTS, golden, load_mlp_weights, mlp_kwargs, mlp_restated
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd.hypernerf import models, modules, warping
from hypernerf_torch_amd.machine import f32_bits

nn = torch.nn
EMB = {"warp": list(range(100)), "camera": [0], "appearance": list(range(100)), "time": list(range(100))}


def test_new_activations_construct():
    for make in ACTS.values():
        modules.MLP(in_ch=16, out_ch=3, hidden_activation=make())
        modules.MLP(in_ch=16, out_ch=40, width=64, depth=2, output_activation=make())
        modules.MLP(in_ch=16, out_ch=2, width=64, depth=2, output_activation=make())     # <= 4 columns: wide route
        modules.NerfMLP(in_ch=63, hidden_activation=make())
        warping.TranslationField(in_ch=3, activation=make())
    m = models.NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, hyper_slice_method="bendy_sheet")
    m.warp_field = warping.TranslationField(in_ch=3, in_ch_embed=m.GLO_dim if hasattr(m, "GLO_dim") else 8,
                                            activation=nn.Softplus())


@pytest.mark.parametrize("act", [nn.SiLU(), nn.GELU()])
def test_silu_gelu_hidden_refused_with_reason(act):
    with pytest.raises(NotImplementedError, match="pre-activation"):
        modules.MLP(in_ch=16, out_ch=3, hidden_activation=act)


@pytest.mark.parametrize("make", list(ACTS.values()))
def test_new_activation_on_narrow_head_refused(make):
    with pytest.raises(NotImplementedError):
        modules.NerfMLP(in_ch=63, rgb_activation=make())


def test_relu_encodings_unchanged_and_new_words():
    """ReLU layers keep zero in every new field; the new activations carry their code, parameters and slots."""
    m = modules.MLP(in_ch=20, out_ch=40, depth=3, width=64, skips=[1], hidden_activation=nn.Softplus(beta=2, threshold=5),
                    output_activation=nn.ELU(0.7))
    prog = m._call(True).program
    fwd, bwd = prog.fwd_ops, prog.bwd_ops
    layers = [w for w in fwd if w[0] == L.HN_OP_LAYER]
    assert len(layers) == 4
    for w in layers[:3]:
        assert (w[1] >> 24) & 15 == L.HN_ACT_SOFTPLUS
        assert w[7] == f32_bits(2.0) and w[4] == f32_bits(5.0)        # p0 = beta, p1 = threshold in the mask word
    out = layers[3]
    assert (out[1] >> 24) & 15 == L.HN_ACT_ELU and out[7] == f32_bits(0.7)
    wide = [w for w in bwd if w[0] == L.HN_BOP_LOAD_WIDE][0]
    assert (wide[3] >> 16) & 15 == L.HN_ACT_ELU and wide[3] & 0xffff == 40 and wide[6] == f32_bits(0.7)
    assert out[5] == wide[7] >= 0                                      # y stashed in the dZ slot, read back in place
    blayers = [w for w in bwd if w[0] == L.HN_BOP_LAYER]
    assert len(blayers) == 3
    for w in blayers:
        assert w[2] == L.HN_ACT_SOFTPLUS and w[3] == f32_bits(2.0) and w[7] == f32_bits(5.0) and w[4] == -1
        assert w[6] >= 0 and prog.slots[w[6]].kind == "stash"
    # the derivative source of each backward layer is the stash slot its forward layer wrote y to
    assert sorted(int(w[6]) for w in blayers) == sorted(int(w[5]) for w in layers[:3])
    # resolved offsets: the parameter words travel untouched, slot words become offsets inside the workspace
    for mode in (L.HN_MODE_BF16, L.HN_MODE_F32):
        f, b = prog.resolved_ops(mode, 1000)
        _, sb, _ = prog.layout(mode, 1000)
        fl = [w for w in f if w[0] == L.HN_OP_LAYER]
        assert fl[0][4] == f32_bits(5.0) and fl[0][7] == f32_bits(2.0)
        for w in (w for w in b if w[0] == L.HN_BOP_LAYER):
            assert w[7] == f32_bits(5.0) and 0 <= w[6] * 1024 < sb

    leaky = modules.MLP(in_ch=20, out_ch=3, depth=2, width=64, hidden_activation=nn.LeakyReLU(0.2))._call(False).program
    relu = modules.MLP(in_ch=20, out_ch=3, depth=2, width=64)._call(False).program
    for wl, wr in zip(leaky.bwd_ops, relu.bwd_ops):
        if wr[0] == L.HN_BOP_LAYER:
            assert list(wr[2:4]) == [0, 0] and wr[6] == 0 and wr[7] == 0 and wr[4] >= 0
            assert wl[2] == L.HN_ACT_LEAKY_RELU and wl[3] == f32_bits(0.2) and wl[4] >= 0     # the mask, as relu
    for wl, wr in zip(leaky.fwd_ops, relu.fwd_ops):
        if wr[0] == L.HN_OP_LAYER and (wr[1] >> 24) & 15 == L.HN_ACT_RELU:
            assert wr[7] == 0
            assert (wl[1] >> 24) & 15 == L.HN_ACT_LEAKY_RELU and wl[7] == f32_bits(0.2) and wl[4] == wr[4]


@pytest.mark.parametrize("kind", ["hidden", "wide"])
@pytest.mark.parametrize("act_name", list(ACTS))
def test_restatement_matches_reference_fixture(kind, act_name):
    """Linear + activation + skip concat in plain torch reproduces the reference's MLP, forward and backward: pins the
    fixture (and the restatement the GPU fuzz compares against) without the reference."""
    g = golden()
    tag = f"{kind}_{act_name}"
    kw = mlp_kwargs(kind, act_name)
    m = modules.MLP(**kw)
    sd = {k: v.double().requires_grad_(True) for k, v in load_mlp_weights(m).items()}
    x = torch.from_numpy(g[f"{tag}/x"]).double().requires_grad_(True)
    y = mlp_restated(sd, x, kw["depth"], kw["skips"], m.hidden_activation,
                     None if isinstance(m.output_activation, nn.Identity) else m.output_activation)
    np.testing.assert_allclose(y.detach().numpy(), g[f"{tag}/y"], rtol=1e-4, atol=1e-4)
    (y * torch.from_numpy(g[f"{tag}/wy"]).double()).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), g[f"{tag}/dx"], rtol=1e-3, atol=1e-4 * float(np.abs(g[f"{tag}/dx"]).max()))
    for name, p in sd.items():
        st = g[f"{tag}/grad/{name}/stats"]
        assert abs(p.grad.norm().item() - st[2]) <= 1e-3 * max(st[2], 1e-12), (name, p.grad.norm().item(), st)
