"""hypernerf_torch_amd — MI355X-native (gfx950) render hot path of songrise/HyperNeRF-torch.

Drop-in module layout (same import paths as the reference, under this package):
    hypernerf_torch_amd.hypernerf.models.NerfModel          <- hypernerf/models.py
    hypernerf_torch_amd.hypernerf.modules.{MLP,GLOEmbed,NerfMLP,HyperSheetMLP}
    hypernerf_torch_amd.hypernerf.warping.{TranslationField,SE3Field}
    hypernerf_torch_amd.hypernerf.model_utils.*
    hypernerf_torch_amd.models.rendering.render_rays        <- models/rendering.py (nerf_pl signature)
    hypernerf_torch_amd.models.nerf.{Embedding,NeRF}        <- models/nerf.py
Beside the reference's surface: hypernerf_torch_amd.geometry (density lattice of a frame, isosurface mesh, PLY files,
mesh images by ray casting, depth fusion, texture atlases and textured OBJ files, occupancy grids that let the renderer
skip empty space) and hypernerf_torch_amd.ops (metrics, data path, mesh and GIF ops, one module per kernel file).

All device arithmetic runs in hand-written HIP kernels behind the C ABI in include/hn_kernels.h
(csrc/libhn_hip.so).  There is no CPU execution path: ops raise on CPU tensors or a missing library.
"""
from . import _lib
from .arena import ParamArena
from .optim import ArenaAdam, ArenaRAdam, ArenaRanger, ArenaSGD, GradClip
from .functional import get_precision, set_precision
from . import geometry
from .geometry import (camera_from_c2w, camera_rays, component_sizes, density_grid, depth_agreement,
                       depth_images_from_field, extract_isosurface, extract_mesh, extract_mesh_fused, filter_mesh, fuse_depth,
                       mesh_components, mesh_depth_error, mesh_turntable, orbit_cameras, read_ply, render_mesh, simplify_mesh,
                       tsdf_isosurface, vertex_colors, write_ply)
from .geometry import (OccupancyCache, clip_rays, occupancy_fraction, occupancy_from_density, occupancy_grid, occupancy_union,
                       unclip)
from .ops.occupancy import OccupancyStack, clip_batch
from .geometry import (atlas_texel_for_size, bake_field_texture, bake_texture, rasterize_atlas, read_obj,
                       render_textured_mesh, texture_atlas, write_obj)

__version__ = "0.1.0"


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP extension for gfx950 (hipcc cross-compiles without a GPU)."""
    return _lib.build(force=force, verbose=verbose)
