"""The surface of `functional` after its eval, data and mesh ops moved to ops/: every public name it had before the split
still resolves on it, every moved name IS the object its ops module defines (one definition, no copies), the ops modules
stay below functional / machine / arena in the import order, and geometry.py no longer reaches private validators or the
binding through the umbrella.  No GPU."""
import ast
import functools
import importlib
import pathlib

import pytest

import hypernerf_torch_amd as HN
from hypernerf_torch_amd import functional as F

PKG = pathlib.Path(HN.geometry.__file__).parent

# what functional.py defined at module level, without a leading underscore, before the split; None = still defined there,
# otherwise the ops module that owns the name now
PUBLIC = {
    "set_precision": None, "get_precision": None, "mode_of": None, "ProgramCall": None, "BATCH_WGRADS": None,
    "WGRAD_OVERLAP": None, "set_wgrad_overlap": None, "drop_pending_wgrads": None, "held_wgrads": None,
    "flush_held_wgrads": None, "run_program": None, "sum_samples": None, "embed_lookup": None,
    "sample_along_rays": None, "MAX_SAMPLES": None, "MAX_PDF_COARSE": None, "check_sample_counts": None,
    "sample_pdf": None, "FAST_DRAWS": None, "seed_draws": None, "random_draws": None, "PROLOGUE": None,
    "render_prologue": None, "COMPOSITE_PDF": None, "composite": None, "backward": None, "mse_loss": None,
    "BG_MAX_ROWS": None, "bg_sample": None, "bg_loss": None,
    "SSIM_MAX_WINDOW": "metrics", "ssim_window": "metrics", "ssim_dssim": "metrics", "MSSSIM_LEVELS": "metrics",
    "MSSSIM_MAX_SIZE": "metrics", "MSSSIM_WEIGHTS": "metrics", "msssim_window": "metrics", "msssim_pyramid": "metrics",
    "msssim_workspace_bytes": "metrics", "msssim_levels": "metrics",
    "ISO_BLOCK": "mesh", "INT32_MAX": "checks", "check_lattice": "mesh", "grid_points": "mesh",
    "density_activate": "mesh", "extract_isosurface": "mesh", "mesh_components": "mesh", "component_sizes": "mesh",
    "gather_rows": "mesh", "compact_mesh": "mesh", "vertex_viewdirs": "mesh",
    "CELL_BITS": "simplify", "check_cells": "simplify", "EXTENT_TILE": "simplify", "vertex_extent": "simplify",
    "cluster_vertices": "simplify", "reduce_clusters": "simplify", "cluster_faces": "simplify",
    "relabel_vertices": "simplify",
    "MESH_TILE": "mesh_render", "MESH_MAX_SIDE": "mesh_render", "check_image_wh": "mesh_render",
    "mesh_project": "mesh_render", "mesh_tile_pairs": "mesh_render", "group_tile_pairs": "mesh_render",
    "mesh_bins": "mesh_render", "mesh_trace": "mesh_render", "SHADINGS": "mesh_render", "check_shading": "mesh_render",
    "mesh_shade": "mesh_render",
    "generate_rays": "data", "ray_batch": "data", "ray_batch_rgba": "data", "NERFIES_CAM_FLOATS": "data",
    "generate_rays_nerfies": "data", "ray_batch_nerfies": "data", "blend_white_u8": "data", "resize_lanczos_u8": "data",
    "premultiply_u8": "data", "resize_lanczos_rgba8": "data",
    "HIST_BINS": "gif", "color_histogram": "gif", "palette_map": "gif", "gif_lzw": "gif", "depth_colormap": "gif",
    "se3_apply": None, "se3_warp": None, "posenc": None, "sample_legacy": None,
}
OPS = ("checks", "data", "gif", "mesh", "mesh_render", "metrics", "simplify")
# the training step's switches and queues: tests and bench.py rebind or read them on `functional`, so a second
# definition anywhere would go stale silently
REBINDABLE = ("_PRECISION", "BATCH_WGRADS", "WGRAD_OVERLAP", "FAST_DRAWS", "PROLOGUE", "COMPOSITE_PDF", "_PENDING",
              "_FORKED", "_PENDING_TASK")


@functools.lru_cache(maxsize=None)
def _module_level_names(path):
    """Names a module binds at top level by def, class or assignment (imports are not definitions)."""
    names = set()
    for node in ast.parse(path.read_text()).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign)):
            for t in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                names.update(n.id for n in ast.walk(t) if isinstance(n, ast.Name))
    return names


def _ops(name):
    return importlib.import_module(f"hypernerf_torch_amd.ops.{name}")


@pytest.mark.parametrize("name", sorted(PUBLIC))
def test_public_name_still_resolves(name):
    assert hasattr(F, name), f"functional lost {name}"


@pytest.mark.parametrize("name", sorted(n for n, owner in PUBLIC.items() if owner))
def test_moved_name_has_one_definition(name):
    owner = _ops(PUBLIC[name])
    assert getattr(F, name) is getattr(owner, name)
    assert name in owner.__all__
    assert name in _module_level_names(PKG / "ops" / f"{PUBLIC[name]}.py")
    assert name not in _module_level_names(PKG / "functional.py")
    others = [m for m in OPS if m != PUBLIC[name] and name in _module_level_names(PKG / "ops" / f"{m}.py")]
    assert not others, f"{name} is also defined in ops.{others}"


@pytest.mark.parametrize("name", sorted(n for n, owner in PUBLIC.items() if owner is None))
def test_kept_name_is_defined_in_functional(name):
    assert name in _module_level_names(PKG / "functional.py")


def test_rebindable_globals_live_in_functional_only():
    here = _module_level_names(PKG / "functional.py")
    for name in REBINDABLE:
        assert name in here, name
        for m in OPS:
            assert name not in _module_level_names(PKG / "ops" / f"{m}.py"), f"{name} is defined in ops.{m}"
            assert not hasattr(_ops(m), name), f"ops.{m} exposes {name}"


def test_ops_modules_are_all_there_and_declare_all():
    found = sorted(p.stem for p in (PKG / "ops").glob("*.py") if p.stem != "__init__")
    assert found == sorted(OPS)
    for m in OPS:
        mod = _ops(m)
        assert mod.__all__ and all(hasattr(mod, n) for n in mod.__all__), m
        assert not [n for n in mod.__all__ if n.startswith("_")], m


def test_ops_never_import_the_training_step():
    """functional imports ops, not the other way round: no import statement of an ops module, lazy ones inside
    functions included, names functional, machine or arena."""
    banned = {"functional", "machine", "arena"}
    for path in sorted((PKG / "ops").glob("*.py")):
        for node in ast.walk(ast.parse(path.read_text())):
            if isinstance(node, ast.Import):
                named = [part for a in node.names for part in a.name.split(".")]
            elif isinstance(node, ast.ImportFrom):
                named = (node.module or "").split(".") + [a.name for a in node.names]
            else:
                continue
            assert not banned & set(named), f"{path.name}:{node.lineno} imports {sorted(banned & set(named))}"


def test_geometry_does_not_go_through_the_umbrella():
    src = (PKG / "geometry.py").read_text()
    assert "F._" not in src
    assert "F.L." not in src
