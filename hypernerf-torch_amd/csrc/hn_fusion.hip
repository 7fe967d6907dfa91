// Depth fusion for gfx950: depth images seen through the cameras of the field are folded into a truncated signed
// distance volume (TSDF) on the lattice of hn_geometry.hip, whose zero level set hn_iso_* then meshes.
//
// Definition (DESIGN.md 3.12 holds it in full; tests/tsdf_restated.py restates it in NumPy float32, bit for bit).  tsdf and
// weight are (nx, ny, nz) fp32 volumes, z fastest, zeroed by the caller before the first batch; cams (n_views, 24) camera
// records, depths (n_views, H, W) fp32: the distance along the unit ray from the camera position, +inf where the ray hit
// nothing, anything not > 0 (zero, negative, NaN) where nothing is known.  Every operation is one fp32 operation rounded
// on its own (the library is built with contraction off), in the order written.  One work-item owns one lattice point x
// (hn_lattice_pos: the bits of hn_grid_points) and walks the views 0 .. n_views - 1 in order:
//   q = x - cam[9:12];  (u, v, flag) = hn_mr_project(cam, x);  flag != 0 skips the view
//   skip unless 0 <= u < W and 0 <= v < H (compared as floats);  col = (int)floorf(u), row = (int)floorf(v)
//   D = depths[view, row, col];  skip unless D > 0
//   r = sqrt((qx*qx + qy*qy) + qz*qz);  s = D - r;  skip if s < -trunc
//   t = fminf(1, s / trunc);  tsdf = (weight * tsdf + t) / (weight + 1);  weight = weight + 1
// No atomics, no reductions: two runs give the same bits, and so do the same views in several batches.
//
// Mapping: a wave owns a 4 x 4 x 4 brick of lattice points (lane = (di*4 + dj)*4 + dk), the four waves of a workgroup four
// bricks that follow each other along z.  A brick projects to a compact patch of the depth image; a wave of 64
// consecutive k projects to a line across it, touches more cache lines per view and measured 2 % slower at 128^3 and
// 0.2 % slower at 256^3 (DESIGN.md 3.12 has both sets of numbers; that mapping is gone).  The launch is bound by its
// arithmetic — a projection, four correctly rounded divisions and a root per voxel-view — at 32 VGPRs and full
// occupancy; the camera record is read through a wave-uniform index and stays in scalar registers.
#include "hn_camera.h"

#define HN_TSDF_BRICK 4      // lattice points per brick side: 4^3 = one wave

__global__ __launch_bounds__(256) void hn_tsdf_integrate_kernel(HnLattice g, float* __restrict__ tsdf,
                                                                float* __restrict__ weight,
                                                                const float* __restrict__ cams,
                                                                const float* __restrict__ depths, int n_views, int H, int W,
                                                                float trunc, int bricks_y, int bricks_z) {
  // brick of this wave: bricks run z fastest, as lattice points do
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int bk = (int)(b % bricks_z), bj = (int)((b / bricks_z) % bricks_y), bi = (int)(b / ((long long)bricks_y * bricks_z));
  const int i = bi * HN_TSDF_BRICK + (lane >> 4), j = bj * HN_TSDF_BRICK + ((lane >> 2) & 3), k = bk * HN_TSDF_BRICK + (lane & 3);
  if (i >= g.nx || j >= g.ny || k >= g.nz) return;      // bricks past the lattice, and the part of an edge brick outside it
  const size_t p = ((size_t)i * g.ny + j) * g.nz + k;
  const float x = hn_lattice_pos(g, 0, i), y = hn_lattice_pos(g, 1, j), z = hn_lattice_pos(g, 2, k);
  float d = tsdf[p], w = weight[p];
  const float fw = (float)W, fh = (float)H, neg_trunc = -trunc;
  const size_t image = (size_t)H * W;
  for (int view = 0; view < n_views; ++view) {
    const float* __restrict__ cam = cams + 24 * (size_t)view;      // uniform over the wave
    float u, v;
    if (hn_mr_project(cam, x, y, z, &u, &v) != 0) continue;
    if (!(u >= 0.0f && u < fw && v >= 0.0f && v < fh)) continue;
    const int col = (int)floorf(u), row = (int)floorf(v);
    const float D = depths[(size_t)view * image + (size_t)row * W + col];
    if (!(D > 0.0f)) continue;
    const float qx = x - cam[9], qy = y - cam[10], qz = z - cam[11];
    // sqrtf, not __fsqrt_rn: the correctly rounded root (see hn_simplify.hip)
    const float r = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz)));
    const float s = __fsub_rn(D, r);
    if (s < neg_trunc) continue;
    const float t = fminf(1.0f, __fdiv_rn(s, trunc));
    d = __fdiv_rn(__fadd_rn(__fmul_rn(w, d), t), __fadd_rn(w, 1.0f));
    w = __fadd_rn(w, 1.0f);
  }
  tsdf[p] = d;
  weight[p] = w;
}

extern "C" int hn_tsdf_integrate(float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const float* bounds_host,
                                 const float* cams_dev, const float* depths_dev, int n_views, int H, int W, float trunc,
                                 hnStream_t stream) {
  HnLattice g;
  if (bounds_host == nullptr || !hn_lattice(nx, ny, nz, bounds_host, &g)) return -2;
  if (n_views < 1 || H < 1 || W < 1 || H > HN_MESH_MAX_SIDE || W > HN_MESH_MAX_SIDE) return -2;
  if (!(trunc > 0.0f && trunc <= 3.402823466e38f)) return -2;
  if (tsdf_dev == nullptr || weight_dev == nullptr || cams_dev == nullptr || depths_dev == nullptr) return -3;
  const int bx = (nx + HN_TSDF_BRICK - 1) / HN_TSDF_BRICK, by = (ny + HN_TSDF_BRICK - 1) / HN_TSDF_BRICK,
            bz = (nz + HN_TSDF_BRICK - 1) / HN_TSDF_BRICK;
  const long long bricks = (long long)bx * by * bz;      // at most the lattice's points: below 2^31 / 7
  hipLaunchKernelGGL(hn_tsdf_integrate_kernel, dim3((unsigned)((bricks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g,
                     tsdf_dev, weight_dev, cams_dev, depths_dev, n_views, H, W, trunc, by, bz);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_tsdf_face_keep: which faces of a mesh extracted on the lattice lie in cells that were observed.  One work-item per
// face: centroid = ((a + b) + c) / 3 per axis, cell index per axis = min(n - 2, max(0, (int)floorf((centroid - lo) / step)))
// — clamped in fp32 before the conversion, so that no value overflows it; a NaN gives cell 0 —, and fkeep[f] = 1 iff all
// eight lattice points of that cell have weight > 0.  vkeep[v] = 1 iff a kept face references v: whoever gets there
// stores the same 1 (vkeep is zeroed by the caller).  A face with an id outside [0, V) is dropped.
// ------------------------------------------------------------------------------------------------
HN_DEV int hn_tsdf_cell(const HnLattice& g, int c, int n, float centroid) {
  const float fl = floorf(__fdiv_rn(__fsub_rn(centroid, g.lo[c]), g.step[c]));
  if (!(fl > 0.0f)) return 0;
  return fl > (float)(n - 2) ? n - 2 : (int)fl;
}

__global__ __launch_bounds__(256) void hn_tsdf_face_keep_kernel(const int32_t* __restrict__ faces, long long n_faces,
                                                                const float* __restrict__ vertices, long long n_vertices,
                                                                const float* __restrict__ weight, HnLattice g,
                                                                int32_t* __restrict__ fkeep, int32_t* __restrict__ vkeep) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  const int32_t id[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
  bool keep = true;
  for (int c = 0; c < 3; ++c) keep = keep && id[c] >= 0 && id[c] < n_vertices;
  if (keep) {
    int cell[3];
    const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sum = __fadd_rn(__fadd_rn(vertices[3 * (size_t)id[0] + c], vertices[3 * (size_t)id[1] + c]),
                                  vertices[3 * (size_t)id[2] + c]);
      cell[c] = hn_tsdf_cell(g, c, n[c], __fdiv_rn(sum, 3.0f));
    }
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const size_t p = ((size_t)(cell[0] + (corner >> 2)) * g.ny + (cell[1] + ((corner >> 1) & 1))) * g.nz +
                       (cell[2] + (corner & 1));
      keep = keep && weight[p] > 0.0f;
    }
  }
  fkeep[f] = keep ? 1 : 0;
  if (keep)
    for (int c = 0; c < 3; ++c) vkeep[id[c]] = 1;
}

extern "C" int hn_tsdf_face_keep(const int32_t* faces_dev, long long n_faces, const float* vertices_dev, long long n_vertices,
                                 const float* weight_dev, int nx, int ny, int nz, const float* bounds_host,
                                 int32_t* fkeep_dev, int32_t* vkeep_dev, hnStream_t stream) {
  HnLattice g;
  if (bounds_host == nullptr || !hn_lattice(nx, ny, nz, bounds_host, &g)) return -2;
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll) return -2;
  if (faces_dev == nullptr || vertices_dev == nullptr || weight_dev == nullptr || fkeep_dev == nullptr || vkeep_dev == nullptr)
    return -3;
  hipLaunchKernelGGL(hn_tsdf_face_keep_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     faces_dev, n_faces, vertices_dev, n_vertices, weight_dev, g, fkeep_dev, vkeep_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
