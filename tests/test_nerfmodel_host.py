"""NerfModel's host side without a GPU: the plan of one forward pass on each of its paths (which programs run on how many
points, which compositing / sampling calls follow, which of them carries `then_pdf`, which noise tensor reaches which
level), that nothing of a pass stays on the model, and the rules of the program cache.  The model is built on the CPU;
every launch seam is a stub that records its call and returns tensors of the right shapes."""
import copy
import gc
import weakref

import pytest
import torch

from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import machine
from hypernerf_torch_amd.hypernerf import modules, warping
from hypernerf_torch_amd.hypernerf.models import NerfModel

EMB = {"warp": list(range(100)), "camera": [0], "appearance": list(range(100)), "time": list(range(100))}
B, NC, NF, G = 5, 8, 8, 8
BENDY = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True)
SE3_AXIS = dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_nerf_embed=True, use_alpha_cond=True)
# path -> (model arguments, SE(3) warp field, NerfModel.REUSE_COARSE, metadata_encoded)
PATHS = {
    "fused_reuse": (BENDY, False, True, False),
    "fused_noreuse": (BENDY, False, False, False),
    "se3_outside": (SE3_AXIS, True, True, False),
    "networks": (BENDY, False, True, True),
}


class Recorder:
    """The launch seams as stubs.  `plan` is what they were called with; `label` names the tensors the draw stubs made."""

    def __init__(self, monkeypatch, fail_on=None):
        self.plan, self.label, self.keep, self.xyz, self.fail_on = [], {}, [], [], fail_on
        for flag in ("PROLOGUE", "FAST_DRAWS", "COMPOSITE_PDF"):
            monkeypatch.setattr(F, flag, True)
        monkeypatch.setattr(L, "require_gpu", lambda *a, **k: None)
        for name in ("run_program", "composite", "sample_pdf", "random_draws", "render_prologue", "embed_lookup",
                     "se3_warp", "sample_along_rays", "density_activate"):
            monkeypatch.setattr(F, name, getattr(self, name))
        monkeypatch.setattr(machine, "pack_many", self.pack_many)
        monkeypatch.setattr(machine, "collect_pack_jobs", self.collect_pack_jobs)

    def name(self, t, rng):
        if t is None:
            return None
        for k, v in (rng or {}).items():
            if v is t:
                return f"rng:{k}"
        return self.label.get(id(t), f"fresh:{tuple(t.shape)}")

    def draws(self, specs):
        out = []
        for shape, kind in specs:
            t = torch.zeros(shape)
            self.label[id(t)] = f"drawn:{kind}:{tuple(shape)}"
            self.keep.append(t)             # (an id names one tensor only while that tensor lives)
            out.append(t)
        return out

    # ---- functional ----
    def run_program(self, call, srcs, samples_per_ray, precision=None, gather_idx=None):
        points = next(s.shape[0] for s, per_ray in zip(srcs, call.src_per_ray) if s is not None and not per_ray)
        self.plan.append(("program", call.program.name, samples_per_ray, points))
        if self.fail_on == call.program.name:
            raise RuntimeError("stub failure")
        live = call.program.params[0].reshape(-1)[0] * 0.0          # outputs require grad as the real ones do
        return tuple(torch.zeros(points, w) + live for w in call.dst_widths)

    def composite(self, rgb, raw, noise, z, dirs, warped=None, variant=0, white_bg=False, sample_at_infinity=True,
                  want_median=True, dust_threshold=None, keep=None, noise_scale=1.0, rgb1=None, raw1=None, warped1=None,
                  perm=None, then_pdf=None):
        b, s = z.shape
        pdf = None if then_pdf is None else "split" if then_pdf.get("split") else "merged"
        parts = (raw.shape[1],) if perm is None else (raw.shape[1], raw1.shape[1])
        self.plan.append(("composite", s, parts, self.name(noise, self.rng), noise_scale, sample_at_infinity, pdf))
        res = [torch.zeros(b, 3), torch.zeros(b), torch.zeros(b), torch.zeros(b, s), torch.zeros(b), torch.zeros(b)]
        if perm is not None:
            assert rgb.shape == (b, parts[0], 3) and rgb1.shape == (b, parts[1], 3) and sum(parts) == s
            assert warped.shape[:2] == (b, parts[0]) and warped1.shape[:2] == (b, parts[1]) and perm.shape == (b, s)
            res.append(torch.zeros(b, s, warped.shape[-1]))
        else:
            assert rgb.shape == (b, s, 3) and raw.shape == (b, s) and warped.shape[:2] == (b, s)
        assert noise is None or tuple(noise.shape) == (b, s, 1)
        if then_pdf is not None:
            res += self.pdf_results(b, s, then_pdf["u"].shape[1], bool(then_pdf.get("split")))
        return tuple(res)

    @staticmethod
    def pdf_results(b, s, nf, split):
        res = [torch.zeros(b, s + nf), torch.zeros(b, s + nf, 3), torch.zeros(b, nf, dtype=torch.int64), torch.zeros(b, nf)]
        if split:
            res += [torch.zeros(b, s + nf, dtype=torch.int32), torch.zeros(b, nf, 3)]
        return res

    def sample_pdf(self, weights, z, u, origins=None, directions=None, want_points=True, bins=None, merge=True, split=False):
        self.plan.append(("sample_pdf", "split" if split else "merged"))
        return tuple(self.pdf_results(z.shape[0], z.shape[1], u.shape[1], split))

    def random_draws(self, specs, device):
        self.plan.append(("random_draws", [(tuple(s), k) for s, k in specs]))
        return self.draws(specs)

    def render_prologue(self, device, mode, pack_groups, specs, sample=None, ids=None):
        self.plan.append(("render_prologue", len(pack_groups), [(tuple(s), k) for s, k in specs], sample is not None,
                          ids is not None))
        z = pts = None
        if sample is not None:
            b, n = sample["origins"].shape[0], sample["lower"].shape[-1]
            z, pts = torch.zeros(b, n), torch.zeros(b, n, 3)
        return self.draws(specs), z, pts

    def sample_along_rays(self, origins, directions, lower, upper, t_rand):
        self.plan.append(("sample_along_rays", self.name(t_rand, self.rng)))
        b, n = origins.shape[0], lower.shape[-1]
        return torch.zeros(b, n), torch.zeros(b, n, 3)

    def embed_lookup(self, table, idx):
        self.plan.append(("embed_lookup", tuple(idx.shape)))
        return table.index_select(0, idx.reshape(-1))

    def se3_warp(self, wv, points, table=None, idx=None, samples_per_ray=1):
        self.plan.append(("se3_warp", points.shape[0], samples_per_ray, table is not None))
        xyz = wv[:, :3] + points
        self.xyz.append(weakref.ref(xyz))
        if table is None:
            return xyz
        return xyz, torch.zeros(points.shape[0], 3 + table.shape[1])

    def density_activate(self, raw, points, render_opts=None):
        self.plan.append(("density_activate", tuple(raw.shape)))
        return torch.zeros_like(raw)

    # ---- machine ----
    def pack_many(self, runners, device, mode, force=False):
        self.plan.append(("pack_many", [r.prog.name for r in runners], force))

    def collect_pack_jobs(self, runners, device, mode, force=False, min_jobs=2):
        self.plan.append(("collect_pack_jobs", [r.prog.name for r in runners], force, min_jobs))
        return []

    rng = None


def build_model(path, monkeypatch):
    kw, se3, reuse, _ = PATHS[path]
    monkeypatch.setattr(NerfModel, "REUSE_COARSE", reuse)
    monkeypatch.setattr(NerfModel, "FUSE_LEVELS", True)
    monkeypatch.setattr(NerfModel, "PREPACK", True)
    torch.manual_seed(0)
    m = NerfModel(EMB, n_samples_coarse=NC, n_samples_fine=NF, noise_std=0.7, **kw)
    if se3:
        m.warp_field = warping.SE3Field(in_ch=3)
    return m


def inputs(path, supplied):
    idx = torch.arange(B, dtype=torch.int64) * 3
    meta = {k: idx for k in ("warp", "camera", "appearance", "time")}
    if PATHS[path][3]:
        meta = {k: torch.zeros(B, G) for k in ("encoded_warp", "encoded_hyper", "encoded_nerf")}
    rays = {"origins": torch.zeros(B, 3), "directions": torch.ones(B, 3), "viewdirs": None, "metadata": meta}
    rng = None
    if supplied:
        rng = {"t_rand": torch.zeros(B, NC), "u": torch.zeros(B, NF), "noise_coarse": torch.zeros(B, NC, 1),
               "noise_fine": torch.zeros(B, NC + NF, 1)}
    return rays, rng


def run_forward(m, rec, path, supplied):
    rays, rng = inputs(path, supplied)
    rec.rng = rng
    del rec.plan[:]
    out = m(rays, {}, rng=rng, metadata_encoded=PATHS[path][3])
    return out, list(rec.plan)


P = B * NC            # the points of a level over Nc (= Nf) samples per ray
DRAWS = [((B, NC), "uniform"), ((B, NC, 1), "normal"), ((B, NF), "uniform"), ((B, NC + NF, 1), "normal")]
N_COARSE, N_FINE = f"drawn:normal:{(B, NC, 1)}", f"drawn:normal:{(B, NC + NF, 1)}"
LEVELS = ["level_coarse", "level_fine", "template_fine_reuse"]
# what every path does around its programs when the model draws (one prologue launch) / the caller supplies the draws
HEAD = {False: lambda packs, force: ([("collect_pack_jobs", packs, force, 1)] if packs else [])
        + [("render_prologue", 0, DRAWS, True, False)],
        True: lambda packs, force: [("pack_many", packs, force)] * bool(packs) + [("sample_along_rays", "rng:t_rand")]}


def composites(supplied, fine_parts, pdf):
    """The two compositing calls: the coarse level's carries then_pdf, each level gets its own noise."""
    nz = ("rng:noise_coarse", 1.0, "rng:noise_fine", 1.0) if supplied else (N_COARSE, 0.7, N_FINE, 0.7)
    return (("composite", NC, (NC,), nz[0], nz[1], True, pdf),
            ("composite", NC + NF, fine_parts, nz[2], nz[3], True, None))


def expected_plan(path, supplied):
    if path == "fused_reuse":
        c, f = composites(supplied, (NC, NF), "split")
        return HEAD[supplied](LEVELS, True) + [("program", "level_coarse", NC, P), c,
                                               ("program", "template_fine_reuse", NC, P),
                                               ("program", "level_fine", NF, B * NF), f]
    if path == "fused_noreuse":
        c, f = composites(supplied, (NC + NF,), "merged")
        return HEAD[supplied](LEVELS[:2], True) + [("program", "level_coarse", NC, P), c,
                                                   ("program", "level_fine", NC + NF, B * (NC + NF)), f]
    if path == "se3_outside":
        c, f = composites(supplied, (NC, NF), "split")
        return HEAD[supplied]([], False) + [("program", "SE3Field", 1, P), ("se3_warp", P, NC, True),
                                            ("program", "template_coarse", NC, P), c,
                                            ("program", "template_fine", NC, P),
                                            ("program", "SE3Field", 1, B * NF), ("se3_warp", B * NF, NF, True),
                                            ("program", "template_fine", NF, B * NF), f]
    c, f = composites(supplied, (NC + NF,), "split")
    return HEAD[supplied]([], False) + [("program", "TranslationField", NC, P), ("program", "HyperSheetMLP", NC, P),
                                        ("program", "template_coarse", NC, P), c,
                                        ("program", "TranslationField", NC + NF, B * (NC + NF)),
                                        ("program", "HyperSheetMLP", NC + NF, B * (NC + NF)),
                                        ("program", "template_fine", NC + NF, B * (NC + NF)), f]


@pytest.mark.parametrize("supplied", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_plan_of_one_forward(monkeypatch, path, supplied):
    rec = Recorder(monkeypatch)
    m = build_model(path, monkeypatch)
    out, plan = run_forward(m, rec, path, supplied)
    assert plan == expected_plan(path, supplied)
    assert m._reused_coarse == {"fused_reuse": "fused", "se3_outside": "outside"}.get(path)
    assert set(out) == {"coarse", "fine"} and set(m.last_sampling) == {"z_coarse", "z_fine", "inds", "u"}
    hyper = 8 if path == "se3_outside" else 4
    for level, s in (("coarse", NC), ("fine", NC + NF)):
        r = out[level]
        assert list(r) == ["points", "warped_points", "rgb", "depth", "acc", "weights", "med_depth", "med_points"]
        assert r["points"].shape == (B, s, 3) and r["warped_points"].shape == (B, s, 3 + hyper)
        assert r["weights"].shape == (B, s) and r["med_points"].shape == (B, 1, 1)
    _, again = run_forward(m, rec, path, supplied)       # and the second pass, programs cached, runs the same plan
    assert again == plan


def test_torch_draws_fall_back_in_the_reference_order(monkeypatch):
    """Without the fused draws: t_rand, u, then each level's density noise where that level composites."""
    rec = Recorder(monkeypatch)
    monkeypatch.setattr(F, "FAST_DRAWS", False)
    m = build_model("fused_reuse", monkeypatch)
    seen = []
    for fn in ("rand", "randn"):
        real = getattr(torch, fn)
        monkeypatch.setattr(torch, fn, lambda *a, _fn=fn, _real=real, **k: (seen.append((_fn, len(rec.plan))), _real(*a, **k))[1])
    _, plan = run_forward(m, rec, "fused_reuse", False)
    comps = [i for i, e in enumerate(plan) if e[0] == "composite"]
    assert [plan[i][3:5] for i in comps] == [(f"fresh:{(B, NC, 1)}", 0.7), (f"fresh:{(B, NC + NF, 1)}", 0.7)]
    # rand (t_rand) behind the pack launch, rand (u) behind the coarse samples, randn right in front of each compositing call
    assert plan[:2] == [("pack_many", LEVELS, True), ("sample_along_rays", f"fresh:{(B, NC)}")]
    assert seen == [("rand", 1), ("rand", 2), ("randn", comps[0]), ("randn", comps[1])]


def test_nothing_of_a_pass_stays_on_the_model(monkeypatch):
    gone = ("_then_pdf", "_auto_noise", "_level_state")
    for path in sorted(PATHS):
        rec = Recorder(monkeypatch)
        m = build_model(path, monkeypatch)
        out, _ = run_forward(m, rec, path, False)
        assert not any(k in vars(m) for k in gone), path
        meta = {k: torch.arange(B) for k in ("warp", "camera", "appearance", "time")}
        for level in ("coarse", "fine"):
            q = m.query_points(torch.zeros(B, 4, 3), meta, level=level)
            assert q["sigma"].shape == (B, 4) and q["rgb"].shape == (B, 4, 3)
        assert not any(k in vars(m) for k in gone), path
        if path == "se3_outside":
            # the warped xyz of every level (the coarse level's is what the fine level re-used) dies with the results
            assert len(rec.xyz) == 4
            del out, q
            gc.collect()
            assert all(r() is None for r in rec.xyz)


@pytest.mark.parametrize("path,fail_on", [("fused_reuse", "template_fine_reuse"), ("fused_reuse", "level_fine"),
                                          ("se3_outside", "template_fine"), ("networks", "template_fine")])
def test_a_failed_fine_level_leaves_nothing_behind(monkeypatch, path, fail_on):
    fresh = run_forward(build_model(path, monkeypatch), Recorder(monkeypatch), path, False)[1]
    rec = Recorder(monkeypatch, fail_on=fail_on)
    m = build_model(path, monkeypatch)
    with pytest.raises(RuntimeError, match="stub failure"):
        run_forward(m, rec, path, False)
    assert not any(k in vars(m) for k in ("_then_pdf", "_auto_noise", "_level_state"))
    rec.fail_on = None
    assert run_forward(m, rec, path, False)[1] == fresh
    if path == "se3_outside":
        gc.collect()
        assert all(r() is None for r in rec.xyz)


# ---- the program cache ------------------------------------------------------------------------------------------------
GLO24 = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, GLO_dim=24)


def unfit_model():
    """37 source components: more than ONE level program stages, so the level is marked as not fitting."""
    torch.manual_seed(0)
    m = NerfModel(EMB, n_samples_coarse=NC, n_samples_fine=NF, **GLO24)
    assert not m._can_fuse_level(True, False, {})
    m._template_call("coarse", 7, False, False)
    assert m._no_fit == {"fuse"} and list(m._template_calls) == [("coarse", 7, False, False)]
    return m


def test_markers_and_programs_are_dropped_together():
    m = unfit_model()
    m.use_viewdirs = False                                       # a structural attribute
    assert not m._no_fit and not m._template_calls
    m = unfit_model()
    m.warp_field = warping.TranslationField(in_ch=3, in_ch_embed=24)      # a sub-module
    assert not m._no_fit and not m._template_calls
    m = unfit_model()
    m.nerf_mlps_coarse.trunk_mlp = copy.deepcopy(m.nerf_mlps_coarse.trunk_mlp)      # a nested module, seen on the next look-up
    assert m._no_fit and m._template_calls
    old = m._template_calls[("coarse", 7, False, False)]
    call = m._template_call("coarse", 7, False, False)
    assert call is not old and not m._no_fit and list(m._template_calls.values()) == [call]
    assert not m._can_fuse_level(True, False, {}) and m._no_fit == {"fuse"}      # and the marker is found again


def test_nested_warp_mlp_swap_rebuilds_the_level_programs():
    torch.manual_seed(0)
    m = NerfModel(EMB, n_samples_coarse=NC, n_samples_fine=NF, **BENDY)
    old = m._level_call("coarse")
    m._no_fit.add("gather")
    m.warp_field.mlp = modules.MLP(in_ch=m.warp_field.mlp.in_ch, out_ch=3, depth=6, width=128)
    new = m._level_call("coarse")
    assert new is not old and not m._no_fit and list(m._template_calls) == [("level", "coarse")]
    assert {id(q) for q in m.warp_field.mlp.parameters()} <= {id(q) for q in new.program.params}


def test_program_cache_holds_programs_only(monkeypatch):
    for path in sorted(PATHS):
        rec = Recorder(monkeypatch)
        m = build_model(path, monkeypatch)
        run_forward(m, rec, path, False)
        assert m._template_calls and all(isinstance(c, F.ProgramCall) for c in m._template_calls.values())
    m = unfit_model()
    assert all(isinstance(c, F.ProgramCall) for c in m._template_calls.values())
    names = [(n, pts) for n, _, pts in m.compiled_programs(B)]
    assert names == [("template_coarse", B * NC)]


def test_can_fuse_level_answers():
    """The configurations of tools/op_lists.py."""
    models = {
        "bendy_warp": (dict(hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True), True),
        "bendy": (dict(hyper_slice_method="bendy_sheet"), True),
        "axis_se3": (dict(hyper_slice_method="axis_aligned_plane", hyper_slice_out_dim=8, use_warp=True,
                          use_nerf_embed=True, use_alpha_cond=True), False),
        # a warp without a hyper slice: the template is sized for hyper channels nothing supplies, and the level program
        # shape-errors as the reference's forward does
        "nowarp_cond": (dict(hyper_slice_method="none", use_nerf_embed=True, use_alpha_cond=True), RuntimeError),
    }
    for name, (kw, want) in models.items():
        m = NerfModel(EMB, n_samples_coarse=8, n_samples_fine=8, view_fourier_dim=6, **kw)
        if name == "axis_se3":
            m.warp_field = warping.SE3Field(in_ch=3)
        if want is RuntimeError:
            with pytest.raises(RuntimeError, match="template input has 63 channels, the MLP expects 115"):
                m._can_fuse_level(True, False, {})
        else:
            assert m._can_fuse_level(True, False, {}) is want, name
        assert m._can_fuse_level(True, True, {}) is False and m._can_fuse_level(False, False, {}) is False
