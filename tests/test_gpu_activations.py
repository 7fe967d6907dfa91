"""LeakyReLU / ELU / Softplus hidden layers and wide outputs on the MI355X: the machine against the reference's own
outputs (tests/golden/g18_activations.npz), against a plain torch restatement on random shapes in both precisions, a
NerfModel whose warp field / template MLPs use them, and the bf16s8 refusal."""
import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
from act_common import ACTS, golden, grad_stats_close, load_mlp_weights, mlp_kwargs, mlp_restated
from gpu_common import DEV, EMB, assert_close, assert_grad_close, assert_rel_close, load_hash, rays_for
from hypernerf_torch_amd.hypernerf import models, modules, warping

pytestmark = pytest.mark.gpu
nn = torch.nn


@pytest.fixture(autouse=True)
def restore_precision():
    old = HN.get_precision()
    yield
    HN.set_precision(old)


def T(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["hidden", "wide"])
@pytest.mark.parametrize("act_name", list(ACTS))
def test_mlp_matches_reference_fixture(precision, kind, act_name):
    """modules.MLP with the activation against the reference: fp32 at test_g03_mlp_hip's tolerances (1e-4 element-wise,
    floor 1e-1), gradients to 5e-3; bf16 at the bf16 model tolerances (3e-2 of the tensor scale, gradients rel L2)."""
    HN.set_precision(precision)
    g = golden()
    tag = f"{kind}_{act_name}"
    m = modules.MLP(**mlp_kwargs(kind, act_name))
    load_mlp_weights(m)
    m = m.to(DEV)
    x = T(g[f"{tag}/x"]).requires_grad_(True)
    y = m(x)
    if precision == "fp32":
        assert_rel_close(y, g[f"{tag}/y"], 1e-4, 1e-1, f"g18 {tag}")
    else:
        assert_close(y, torch.from_numpy(g[f"{tag}/y"]), 3e-2, f"g18 bf16 {tag}", elementwise=False)
    (y * T(g[f"{tag}/wy"])).sum().backward()
    if precision == "fp32":
        assert_grad_close(x.grad, torch.from_numpy(g[f"{tag}/dx"]), 5e-3, f"g18 {tag} dx")
        grad_stats_close({k: v.grad for k, v in m.named_parameters()}, g, f"{tag}/grad/", 5e-3)
    else:
        # the wide cases' hidden layers are ReLU, whose bf16 mask is the sign bit: it keeps the
        # pre-activations that are exactly +0 — the fixture's all-zero rows 80..87 — where the reference drops them
        rows = torch.ones(x.shape[0], dtype=torch.bool)
        if kind == "wide":
            rows[80:88] = False
        assert_grad_close(x.grad.cpu()[rows], torch.from_numpy(g[f"{tag}/dx"])[rows], 0.1, f"g18 bf16 {tag} dx",
                          frobenius=True)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mlp_random_shapes_fuzz_activations(precision):
    """Random widths 24..256, depths 0..8, skips, point counts that are no multiple of 32, every activation as hidden
    and (on wide outputs) output activation, against the plain torch restatement."""
    HN.set_precision(precision)
    rs = np.random.RandomState(4321)
    names = list(ACTS)
    for case in range(24):
        act_name = names[case % len(names)]
        in_ch = int(rs.choice([3, 7, 20, 33, 64]))
        width = int(rs.choice([24, 32, 53, 64, 96, 128, 200, 256]))
        depth = int(rs.randint(0, 9))
        n_hidden = max(depth, 1)
        skips = sorted(set(int(v) for v in rs.randint(0, max(1, n_hidden - 1), size=rs.randint(0, 3)))) if n_hidden > 1 else []
        out_ch = int(rs.choice([3, 8, 40]))
        wide_act = rs.rand() < 0.5
        n = int(rs.choice([5, 31, 33, 100, 257, 700]))
        hid = ACTS[act_name]()
        out_act = ACTS[names[(case + 1) % len(names)]]() if wide_act else None
        what = f"{precision} fuzz {case}: {act_name} in {in_ch} width {width} depth {depth} skips {skips} out {out_ch} " \
               f"out_act {type(out_act).__name__} n {n}"
        m = modules.MLP(in_ch=in_ch, out_ch=out_ch, depth=depth, width=width, skips=skips, hidden_activation=hid,
                        output_activation=out_act)
        sd = load_hash(m, 500 + case)
        m = m.to(DEV)
        x = H.uniform(500 + case, "x", (n, in_ch), -1.5, 1.5)
        xg = x.to(DEV).requires_grad_(in_ch <= 24)
        y = m(xg)
        wy = H.uniform(500 + case, "wy", (n, out_ch), -1, 1)
        (y * wy.to(DEV)).sum().backward()
        p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xr = x.double().requires_grad_(True)
        yr = mlp_restated(p, xr, depth, skips, hid, out_act)
        (yr * wy.double()).sum().backward()
        if precision == "fp32":
            assert_rel_close(y, yr, 1e-4, 1e-1, what)
            for k, prm in m.named_parameters():
                assert_grad_close(prm.grad, p[k].grad, 5e-3, f"{what} d{k}")
            if xg.requires_grad:
                assert_grad_close(xg.grad, xr.grad, 5e-3, what + " dx")
        else:
            assert_close(y, yr.float(), 3e-2, what, elementwise=False)
            assert_grad_close(m.linears[0].weight.grad, p["linears.0.weight"].grad, 0.1, what + " dW0", frobenius=True)
            if xg.requires_grad:
                assert_grad_close(xg.grad, xr.grad, 0.1, what + " dx", frobenius=True)


def test_fields_match_reference_fixture():
    """TranslationField(activation=Softplus()) and NerfMLP(hidden_activation=ELU()) (trunk output ELU included) against
    the reference, fp32."""
    HN.set_precision("fp32")
    g = golden()
    tf = warping.TranslationField(in_ch=3, in_ch_embed=8, activation=nn.Softplus())
    load_hash(tf, 19)
    tf = tf.to(DEV)
    pts, meta = T(g["tf/pts"]).requires_grad_(True), T(g["tf/meta"]).requires_grad_(True)
    out = tf(pts, meta, {"warp_alpha": None})
    y = out["warped_points"] if isinstance(out, dict) else out
    assert_rel_close(y, g["tf/y"], 1e-4, 1e-1, "g18 TranslationField(Softplus)")
    (y * T(g["tf/wy"])).sum().backward()
    assert_grad_close(pts.grad, torch.from_numpy(g["tf/dpts"]), 5e-3, "g18 tf dpts")
    assert_grad_close(meta.grad, torch.from_numpy(g["tf/dmeta"]), 5e-3, "g18 tf dmeta")
    grad_stats_close({k: v.grad for k, v in tf.named_parameters()}, g, "tf/grad/", 5e-3)

    nm = modules.NerfMLP(in_ch=27, trunk_depth=3, trunk_width=256, rgb_branch_depth=1, rgb_branch_width=128,
                         hidden_activation=nn.ELU(), skips=[1], alpha_condition_dim=8, rgb_condition_dim=12,
                         rgb_activation=nn.Sigmoid())
    load_hash(nm, 20)
    nm = nm.to(DEV)
    x = T(g["nm/x"]).requires_grad_(True)
    out = nm(x, T(g["nm/ac"]), T(g["nm/rc"]))
    assert_rel_close(out["rgb"], g["nm/rgb"], 1e-4, 1e-1, "g18 NerfMLP(ELU) rgb")
    assert_rel_close(out["alpha"], g["nm/alpha"], 1e-4, 1e-1, "g18 NerfMLP(ELU) alpha")
    ((out["rgb"] * T(g["nm/wr"])).sum() + (out["alpha"] * T(g["nm/wa"])).sum()).backward()
    assert_grad_close(x.grad, torch.from_numpy(g["nm/dx"]), 5e-3, "g18 nm dx")
    grad_stats_close({k: v.grad for k, v in nm.named_parameters()}, g, "nm/grad/", 5e-3)


def swapped_model(nc=8, nf=8, **kw):
    m = models.NerfModel(EMB, near=0.0, far=1.0, n_samples_coarse=nc, n_samples_fine=nf, view_fourier_dim=6,
                         hyper_slice_method="bendy_sheet", use_nerf_embed=False, use_alpha_cond=False, **kw)
    m.warp_field = warping.TranslationField(in_ch=3, in_ch_embed=m.GLO_dim if hasattr(m, "GLO_dim") else 8,
                                            activation=nn.Softplus())
    for lvl in ("coarse", "fine"):
        old = getattr(m, f"nerf_mlps_{lvl}")
        setattr(m, f"nerf_mlps_{lvl}", modules.NerfMLP(
            in_ch=old.in_ch, trunk_depth=old.trunk_depth, trunk_width=old.trunk_width,
            rgb_branch_depth=old.rgb_branch_depth, rgb_branch_width=old.rgb_branch_width, hidden_activation=nn.ELU(),
            skips=old.skips, alpha_channels=old.alpha_channels, rgb_channels=old.rgb_channels,
            rgb_activation=nn.Sigmoid(), alpha_condition_dim=old.alpha_condition_dim,
            rgb_condition_dim=old.rgb_condition_dim))
    return m


def test_swapped_model_matches_reference_fixture():
    """A bendy-sheet NerfModel (8+8 samples) with TranslationField(Softplus) and NerfMLP(ELU): forward, loss and every
    parameter gradient against the reference, fp32 (test_golden_model_fp32's tolerances)."""
    HN.set_precision("fp32")
    g = golden()
    b, seed = int(g["model/b"]), int(g["model/seed"])
    m = swapped_model(int(g["model/nc"]), int(g["model/nf"]), noise_std=None)
    assert sorted(m.state_dict().keys()) == g["model/keys"].tolist()
    load_hash(m, seed)
    m = m.to(DEV)
    o, d, idx = rays_for(seed, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    rng = {"t_rand": T(g["model/draw0_rand"]), "u": T(g["model/draw1_rand"])}
    out = m(rays, {}, rng=rng)
    for lvl in ("coarse", "fine"):
        for k in ("rgb", "depth", "acc", "weights"):
            assert_close(out[lvl][k], torch.from_numpy(g[f"model/{lvl}/{k}"]), 1e-4, f"g18 model {lvl}/{k}")
    gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0).to(DEV)
    loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
    assert abs(float(loss.detach()) - float(g["model/loss"])) <= 1e-4 * max(1.0, float(g["model/loss"]))
    loss.backward()
    grad_stats_close({k: v.grad for k, v in m.named_parameters()}, g, "model/grad/", 5e-3)


def test_swapped_model_trains_bf16():
    """A few Adam steps of the Softplus / ELU model in bf16: the loss stays finite and goes down."""
    HN.set_precision("bf16")
    torch.manual_seed(0)
    m = swapped_model(16, 16, noise_std=None).to(DEV)
    b, seed = 128, 31
    o, d, idx = rays_for(seed, b)
    rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
            "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
    gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0).to(DEV)
    rng = {"t_rand": H.uniform(seed, "t", (b, 16), 0, 1).to(DEV), "u": H.uniform(seed, "u", (b, 16), 0, 1).to(DEV)}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        out = m(rays, {}, rng=rng)
        loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


def test_swapped_model_captured_train_step():
    """TrainStep with the Softplus / ELU model: the first graphed step equals an eager first step (up to the summation
    order of the weight-gradient atomics, as test_first_graphed_step_applies_exactly_one_update holds ReLU models), and
    a few replays keep the loss finite and decreasing."""
    from hypernerf_torch_amd.training import TrainStep
    HN.set_precision("fp32")
    b, seed = 64, 32
    o, d, idx = rays_for(seed, b)
    rays = torch.cat([o, d, torch.zeros(b, 1), torch.ones(b, 1), idx.float()[:, None]], dim=1).to(DEV)
    rgbs = H.uniform(seed, "rgbs", (b, 3), 0.1, 0.9).to(DEV)
    deltas = {}
    for use_graph in (False, True):
        m = swapped_model(16, 16, noise_std=None)
        load_hash(m, seed)
        m = m.to(DEV)
        m.use_stratified_sampling = False           # no random draws: eager and graph see the same samples
        ts = TrainStep(m, lr=1e-3, use_graph=use_graph)
        before = ts.arena.data.clone()
        first = ts.step(rays, rgbs)
        deltas[use_graph] = ts.arena.data - before
        if use_graph:
            losses = [float(first["train/loss"])] + [float(ts.step(rays, rgbs)["train/loss"]) for _ in range(5)]
    diff = (deltas[True] - deltas[False]).abs()
    assert float((diff > 1e-5).float().mean()) < 1e-3, float((diff > 1e-5).float().mean())
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("act_name", ["elu", "sp"])
def test_bf16s8_refuses_elu_softplus(act_name):
    HN.set_precision("bf16s8")
    m = modules.MLP(**mlp_kwargs("hidden", act_name))
    load_mlp_weights(m)
    m = m.to(DEV)
    x = T(golden()[f"hidden_{act_name}/x"]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="bf16s8"):
        m(x)


def test_bf16s8_runs_leaky_relu():
    HN.set_precision("bf16s8")
    m = modules.MLP(**mlp_kwargs("hidden", "leaky"))
    load_mlp_weights(m)
    m = m.to(DEV)
    g = golden()
    x = T(g["hidden_leaky/x"]).requires_grad_(True)
    y = m(x)
    assert_close(y, torch.from_numpy(g["hidden_leaky/y"]), 3e-2, "g18 bf16s8 leaky", elementwise=False)
    (y * T(g["hidden_leaky/wy"])).sum().backward()
    assert torch.isfinite(x.grad).all()
