"""The host halves of the kernels outside the training step, one module per kernel source file:

    metrics      csrc/hn_metrics.hip, csrc/hn_msssim.hip    SSIM (differentiable) and multi-scale SSIM
    lpips        csrc/hn_lpips.hip                           LPIPS: the backbones' layers on the fp32 MFMA, the weight loader
    mesh         csrc/hn_geometry.hip, csrc/hn_fusion.hip    lattice points, isosurface, components, compaction; depth
                                                             fusion into a TSDF volume, its observed faces
                 csrc/hn_mesh_distance.hip                   surface samples, the distance grid, nearest points of a mesh
    registration csrc/hn_registration.hip                    similarity transform of points, the sums an ICP iteration
                                                             solves from, both solves
    simplify     csrc/hn_simplify.hip                        vertex clustering
    texture      csrc/hn_texture.hip                         texture atlas: face classes, cell layout, texel rasteriser,
                                                             textured shading
    mesh_render  csrc/hn_mesh_render.hip                     projection, binning, ray casting, shading
    occupancy    csrc/hn_occupancy.hip                       occupancy bits of a density lattice, dilation, ray clipping
    data         csrc/hn_data.hip                            ray generation, batch gathers, blend, Pillow-exact resize
    gif          csrc/hn_gif.hip                             colour histogram, palette map, LZW, depth colour map
    checks       —                                           argument validators more than one of them uses

They import the binding (_lib), torch, numpy and each other, never functional, machine or arena: functional imports
them and re-exports their public names.
"""
from . import checks, data, gif, lpips, mesh, mesh_render, metrics, occupancy, registration, simplify, texture

__all__ = ["checks", "data", "gif", "lpips", "mesh", "mesh_render", "metrics", "occupancy", "registration", "simplify", "texture"]
