// Geometry out of a trained field, for gfx950: lattice points for density queries, the density activation of a point
// query, an indexed triangle mesh of an isosurface by marching tetrahedra, and what follows on that mesh: connected
// components, filtering by component, view directions for vertex colours (further down, each with its own header).
//
// Lattice: (nx, ny, nz) points over bounds (xmin, xmax, ymin, ymax, zmin, zmax), point index p = (i*ny + j)*nz + k at
// lo + (i, j, k) * step, step = (hi - lo) / (n - 1) taken once on the host; product and sum are rounded on their own
// (no contraction), so a float32 NumPy restatement gives the same bits.
//
// Isosurface of a C-contiguous fp32 grid f[nx][ny][nz] at `iso`, inside = f >= iso (NaN is outside).  Every cell is split
// into the six Kuhn tetrahedra around its main diagonal: for the q-th permutation pi of the axes (lexicographic order)
// v0 = cell origin, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = v0 + (1,1,1).  Neighbouring cells cut their shared face along
// the same diagonal, so the surface is watertight by construction.  Every tetrahedron edge leaves its LOWER lattice
// point in one of seven directions (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1): lattice point p owns the
// edge slots e = 7*p + d, and a vertex is named by its slot — an indexed mesh without a sort and without atomics.
//   pass A  hn_iso_mark      per lattice point the 7-bit mask of owned edges whose ends differ in `inside`; count per block
//   (scan)                   exclusive scan of the block counts (the caller's: torch.cumsum)
//   pass B  hn_iso_vertices  vertex id = block offset + rank inside the block (ascending slot); position, normal, slot
//   pass C  hn_iso_faces     per cell 0 .. 12 triangles (count launch, scan, emit launch): faces by cell, tetrahedron,
//                            triangle, vertex ids looked up through the slots
// Ranks inside a block come from wave64 ballots (one per bit plane) and four wave totals in LDS: the same input gives the
// same arrays on every run.  All four kernels stream the grid once (neighbours come out of L2) and are HBM bound:
// 28 bytes of slots per lattice point are the largest term.
#include "hn_camera.h"

// HnLattice, hn_lattice (host) and hn_lattice_pos (device) live in hn_camera.h, shared with hn_fusion.hip

// ------------------------------------------------------------------------------------------------
// hn_grid_points: out[r] = position of lattice point min(start + r, N - 1), r < count — a chunk of the lattice as the
// (rows, S, 3) points of a point query; the padding of the last chunk repeats the last lattice point.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_grid_points_kernel(HnLattice g, long long start, long long count,
                                                             float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= count) return;
  const long long n = (long long)g.nx * g.ny * g.nz;
  long long p = start + r;
  if (p > n - 1) p = n - 1;
  const int k = (int)(p % g.nz), j = (int)((p / g.nz) % g.ny), i = (int)(p / ((long long)g.ny * g.nz));
  float* o = out + 3 * (size_t)r;
  o[0] = hn_lattice_pos(g, 0, i);
  o[1] = hn_lattice_pos(g, 1, j);
  o[2] = hn_lattice_pos(g, 2, k);
}

extern "C" int hn_grid_points(int nx, int ny, int nz, const float* bounds_host, long long start, long long count,
                              float* out_dev, hnStream_t stream) {
  HnLattice g;
  if (bounds_host == nullptr || out_dev == nullptr || !hn_lattice(nx, ny, nz, bounds_host, &g)) return -2;
  if (start < 0 || count <= 0 || start >= (long long)nx * ny * nz || count > 2147483647ll) return -2;
  hipLaunchKernelGGL(hn_grid_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g,
                     start, count, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_density_activate: what the compositing kernel does to a raw density before it integrates it (hn_composite_*):
// Softplus (beta 1, threshold 20), then filter_sigma — below the dust threshold or outside the bounding box gives 0.
// ------------------------------------------------------------------------------------------------
struct HnBox { float v[6]; };

__global__ __launch_bounds__(256) void hn_density_activate_kernel(const float* __restrict__ raw,
                                                                  const float* __restrict__ points, long long n,
                                                                  int has_dust, float dust, int has_box, HnBox box,
                                                                  float* __restrict__ sigma_out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float x = raw[r];
  float sigma = x > 20.0f ? x : log1pf(expf(x));
  float keep = 1.0f;
  if (has_dust != 0 && !(sigma >= dust)) keep = 0.0f;
  if (has_box != 0) {
    const float* p = points + 3 * (size_t)r;
    const bool in = p[0] >= box.v[0] && p[0] <= box.v[1] && p[1] >= box.v[2] && p[1] <= box.v[3] && p[2] >= box.v[4] &&
                    p[2] <= box.v[5];
    if (!in) keep = 0.0f;
  }
  sigma_out[r] = sigma * keep;
}

extern "C" int hn_density_activate(const float* raw_dev, const float* points_dev, long long n, int has_dust,
                                   float dust_threshold, const float* box_host, float* sigma_dev, hnStream_t stream) {
  if (raw_dev == nullptr || sigma_dev == nullptr || n <= 0 || n > 2147483647ll * 256) return -2;
  if (box_host != nullptr && points_dev == nullptr) return -2;
  HnBox box = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
  if (box_host != nullptr)
    for (int c = 0; c < 6; ++c) box.v[c] = box_host[c];
  hipLaunchKernelGGL(hn_density_activate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     raw_dev, points_dev, n, has_dust, dust_threshold, box_host != nullptr ? 1 : 0, box, sigma_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// ranks inside a workgroup of HN_ISO_BLOCK threads.  `v` holds NB bits per thread; WEIGHTED = false: every set bit is one
// item (the 7 edge bits of a lattice point), true: v is a binary count (triangles of a cell).  Returns the number of
// items of the threads in front of this one; `total` = the items of the whole workgroup.  One ballot per bit plane, the
// lanes in front counted with a mask; four wave totals through LDS.  Every thread of the workgroup must call it.
// ------------------------------------------------------------------------------------------------
template <int NB, bool WEIGHTED>
HN_DEV int hn_iso_block_rank(unsigned v, int* wave_sums, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long front = (1ull << lane) - 1ull;
  int ex = 0, wave_total = 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const unsigned long long m = __ballot((v >> b) & 1u);
    const int w = WEIGHTED ? (1 << b) : 1;
    ex += w * __popcll(m & front);
    wave_total += w * __popcll(m);
  }
  if (lane == 0) wave_sums[wave] = wave_total;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < HN_ISO_BLOCK / 64; ++w) {
    const int s = wave_sums[w];
    if (w < wave) ex += s;
    total += s;
  }
  return ex;
}

// direction class d -> lattice offset (dx, dy, dz) as the bits 4, 2, 1 of a corner code
__constant__ int hn_iso_dir_code[7] = {4, 2, 1, 6, 5, 3, 7};

HN_DEV bool hn_iso_inside(float f, float iso) { return f >= iso; }      // false for NaN

// ------------------------------------------------------------------------------------------------
// pass A
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HN_ISO_BLOCK) void hn_iso_mark_kernel(const float* __restrict__ f, int nx, int ny, int nz,
                                                                   float iso, uint8_t* __restrict__ mask,
                                                                   int32_t* __restrict__ block_counts) {
  __shared__ int wave_sums[HN_ISO_BLOCK / 64];
  const long long n = (long long)nx * ny * nz;
  const long long p = (long long)blockIdx.x * HN_ISO_BLOCK + threadIdx.x;
  unsigned m = 0;
  if (p < n) {
    const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / ((long long)ny * nz));
    const bool ia = hn_iso_inside(f[p], iso);
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int code = hn_iso_dir_code[d];
      const int dx = code >> 2, dy = (code >> 1) & 1, dz = code & 1;
      if (i + dx < nx && j + dy < ny && k + dz < nz) {
        const bool ib = hn_iso_inside(f[p + ((long long)dx * ny + dy) * nz + dz], iso);
        if (ia != ib) m |= 1u << d;
      }
    }
    mask[p] = (uint8_t)m;
  }
  int total;
  hn_iso_block_rank<7, false>(m, wave_sums, total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

extern "C" int hn_iso_mark(const float* grid_dev, int nx, int ny, int nz, float iso, uint8_t* mask_dev,
                           int32_t* block_counts_dev, hnStream_t stream) {
  HnLattice g;
  if (grid_dev == nullptr || mask_dev == nullptr || block_counts_dev == nullptr || !hn_lattice(nx, ny, nz, nullptr, &g))
    return -2;
  const long long n = (long long)nx * ny * nz;
  hipLaunchKernelGGL(hn_iso_mark_kernel, dim3((unsigned)((n + HN_ISO_BLOCK - 1) / HN_ISO_BLOCK)), dim3(HN_ISO_BLOCK), 0,
                     (hipStream_t)stream, grid_dev, nx, ny, nz, iso, mask_dev, block_counts_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// pass B.  Vertex on the edge a -> b (a the owning lattice point): t = (iso - fa) / (fb - fa),
// position = pos(a) + t * (pos(b) - pos(a)), normal = -g / |g| with g = ga + t * (gb - ga), ga / gb the central
// differences of f at the two ends (one-sided on the boundary of the lattice); |g| = 0 (or NaN) gives (0, 0, 0).
// ------------------------------------------------------------------------------------------------
HN_DEV void hn_iso_gradient(const float* __restrict__ f, const HnLattice& g, int i, int j, int k, float* out) {
  const int idx[3] = {i, j, k}, n[3] = {g.nx, g.ny, g.nz};
  const long long stride[3] = {(long long)g.ny * g.nz, (long long)g.nz, 1ll};
  const long long p = ((long long)i * g.ny + j) * g.nz + k;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int hi = idx[c] + 1 < n[c] ? idx[c] + 1 : n[c] - 1, lo = idx[c] > 0 ? idx[c] - 1 : 0;
    const float width = __fmul_rn((float)(hi - lo), g.step[c]);
    out[c] = __fdiv_rn(__fsub_rn(f[p + (hi - idx[c]) * stride[c]], f[p + (lo - idx[c]) * stride[c]]), width);
  }
}

__global__ __launch_bounds__(HN_ISO_BLOCK) void hn_iso_vertices_kernel(const float* __restrict__ f, HnLattice g, float iso,
                                                                       const uint8_t* __restrict__ mask,
                                                                       const int64_t* __restrict__ block_offsets,
                                                                       float* __restrict__ vertices,
                                                                       float* __restrict__ normals,
                                                                       int32_t* __restrict__ slots) {
  __shared__ int wave_sums[HN_ISO_BLOCK / 64];
  const long long n = (long long)g.nx * g.ny * g.nz;
  const long long p = (long long)blockIdx.x * HN_ISO_BLOCK + threadIdx.x;
  const unsigned m = p < n ? mask[p] : 0u;
  int total;
  const int rank = hn_iso_block_rank<7, false>(m, wave_sums, total);
  if (p >= n) return;
  long long vid = block_offsets[blockIdx.x] + rank;
  const int k = (int)(p % g.nz), j = (int)((p / g.nz) % g.ny), i = (int)(p / ((long long)g.ny * g.nz));
  float fa = 0.f, ga[3] = {0.f, 0.f, 0.f}, pa[3] = {0.f, 0.f, 0.f};
  if (m != 0u) {
    fa = f[p];
    hn_iso_gradient(f, g, i, j, k, ga);
    pa[0] = hn_lattice_pos(g, 0, i); pa[1] = hn_lattice_pos(g, 1, j); pa[2] = hn_lattice_pos(g, 2, k);
  }
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    int slot = -1;
    if ((m >> d) & 1u) {
      const int code = hn_iso_dir_code[d];
      const int ib[3] = {i + (code >> 2), j + ((code >> 1) & 1), k + (code & 1)};
      const float fb = f[((long long)ib[0] * g.ny + ib[1]) * g.nz + ib[2]];
      const float t = __fdiv_rn(__fsub_rn(iso, fa), __fsub_rn(fb, fa));
      float gb[3], gv[3];
      hn_iso_gradient(f, g, ib[0], ib[1], ib[2], gb);
      float* vo = vertices + 3 * (size_t)vid;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float pb = hn_lattice_pos(g, c, ib[c]);
        vo[c] = __fadd_rn(pa[c], __fmul_rn(t, __fsub_rn(pb, pa[c])));
        gv[c] = __fadd_rn(ga[c], __fmul_rn(t, __fsub_rn(gb[c], ga[c])));
      }
      const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(gv[0], gv[0]), __fmul_rn(gv[1], gv[1])), __fmul_rn(gv[2], gv[2])));
      float* no = normals + 3 * (size_t)vid;
      const bool ok = len > 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) no[c] = ok ? __fdiv_rn(-gv[c], len) : 0.0f;
      slot = (int)vid;
      ++vid;
    }
    slots[7 * (size_t)p + d] = slot;
  }
}

extern "C" int hn_iso_vertices(const float* grid_dev, int nx, int ny, int nz, const float* bounds_host, float iso,
                               const uint8_t* mask_dev, const int64_t* block_offsets_dev, float* vertices_dev,
                               float* normals_dev, int32_t* slots_dev, hnStream_t stream) {
  HnLattice g;
  if (grid_dev == nullptr || bounds_host == nullptr || mask_dev == nullptr || block_offsets_dev == nullptr ||
      vertices_dev == nullptr || normals_dev == nullptr || slots_dev == nullptr || !hn_lattice(nx, ny, nz, bounds_host, &g))
    return -2;
  const long long n = (long long)nx * ny * nz;
  hipLaunchKernelGGL(hn_iso_vertices_kernel, dim3((unsigned)((n + HN_ISO_BLOCK - 1) / HN_ISO_BLOCK)), dim3(HN_ISO_BLOCK), 0,
                     (hipStream_t)stream, grid_dev, g, iso, mask_dev, block_offsets_dev, vertices_dev, normals_dev,
                     slots_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// pass C.  The 6 x 16 table of triangles per (tetrahedron, inside mask) is worked out at compile time from the rule:
//   one corner L alone on its side, the others R0 < R1 < R2: triangle on the edges (L,R0) (L,R1) (L,R2); with
//     s = det(R0 - L, R1 - L, R2 - L) that order winds with its normal away from L when s > 0 — kept when L is the
//     inside corner and s > 0 or L is the outside corner and s < 0, otherwise the last two are swapped;
//   two inside I0 < I1, two outside O0 < O1: the quad (I0,O0) (I0,O1) (I1,O1) (I1,O0), reversed when
//     det(O1 - O0, I1 - I0, O0 + O1 - I0 - I1) < 0, cut along its first diagonal.
// Integer determinants of lattice vectors only: normals point from inside to outside (towards lower f) whatever the
// emitted triangle's shape, degenerate ones (a lattice value equal to iso) included.
// Entry: bits 0-1 triangles; vertex s of triangle r at bits 2 + 4*(3r + s): corner a (2 bits), corner b (2 bits), a < b.
// ------------------------------------------------------------------------------------------------
struct HnTetTable {
  unsigned entry[6][16];
  int corner[6][4];      // corner code of v_t: bits 4, 2, 1 = offset along x, y, z
  int dir_class[8];      // corner code of (b - a) -> direction class
};

constexpr int hn_tet_det(const int* a, const int* b, const int* c) {
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

constexpr unsigned hn_tet_edge(int a, int b) { return a < b ? (unsigned)(a | b << 2) : (unsigned)(b | a << 2); }

constexpr HnTetTable hn_make_tet_table() {
  HnTetTable t = {};
  const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const int classes[7] = {4, 2, 1, 6, 5, 3, 7};
  for (int d = 0; d < 7; ++d) t.dir_class[classes[d]] = d;
  for (int q = 0; q < 6; ++q) {
    int v[4][3] = {};
    v[1][perms[q][0]] = 1;
    v[2][perms[q][0]] = 1;
    v[2][perms[q][1]] = 1;
    v[3][0] = v[3][1] = v[3][2] = 1;
    for (int c = 0; c < 4; ++c) t.corner[q][c] = v[c][0] * 4 + v[c][1] * 2 + v[c][2];
    for (int mask = 0; mask < 16; ++mask) {
      int ins[4] = {}, outs[4] = {}, ni = 0, no = 0;
      for (int c = 0; c < 4; ++c) {
        if ((mask >> c) & 1) ins[ni++] = c;
        else outs[no++] = c;
      }
      unsigned e = 0;
      if (ni == 1 || no == 1) {
        const int lone = ni == 1 ? ins[0] : outs[0];
        const int* rest = ni == 1 ? outs : ins;
        int d[3][3] = {};
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) d[r][c] = v[rest[r]][c] - v[lone][c];
        const bool away = hn_tet_det(d[0], d[1], d[2]) > 0;
        const bool keep = ni == 1 ? away : !away;
        const unsigned tri[3] = {hn_tet_edge(lone, rest[0]), hn_tet_edge(lone, rest[keep ? 1 : 2]),
                                 hn_tet_edge(lone, rest[keep ? 2 : 1])};
        e = 1u | tri[0] << 2 | tri[1] << 6 | tri[2] << 10;
      } else if (ni == 2) {
        int a[3] = {}, b[3] = {}, c3[3] = {};
        for (int c = 0; c < 3; ++c) {
          a[c] = v[outs[1]][c] - v[outs[0]][c];
          b[c] = v[ins[1]][c] - v[ins[0]][c];
          c3[c] = v[outs[0]][c] + v[outs[1]][c] - v[ins[0]][c] - v[ins[1]][c];
        }
        const bool flip = hn_tet_det(a, b, c3) < 0;
        const unsigned q0 = hn_tet_edge(ins[0], outs[0]), q1 = hn_tet_edge(ins[0], outs[1]),
                       q2 = hn_tet_edge(ins[1], outs[1]), q3 = hn_tet_edge(ins[1], outs[0]);
        const unsigned quad[4] = {q0, flip ? q3 : q1, q2, flip ? q1 : q3};
        e = 2u | quad[0] << 2 | quad[1] << 6 | quad[2] << 10 | quad[0] << 14 | quad[2] << 18 | quad[3] << 22;
      }
      t.entry[q][mask] = e;
    }
  }
  return t;
}

__constant__ HnTetTable hn_tet_table = hn_make_tet_table();

template <bool EMIT>
__global__ __launch_bounds__(HN_ISO_BLOCK) void hn_iso_faces_kernel(const float* __restrict__ f, int nx, int ny, int nz,
                                                                    float iso, const int32_t* __restrict__ slots,
                                                                    const int64_t* __restrict__ block_offsets,
                                                                    int32_t* __restrict__ block_counts,
                                                                    int32_t* __restrict__ faces) {
  __shared__ int wave_sums[HN_ISO_BLOCK / 64];
  const long long n_cells = (long long)(nx - 1) * (ny - 1) * (nz - 1);
  const long long c = (long long)blockIdx.x * HN_ISO_BLOCK + threadIdx.x;
  unsigned inside = 0, count = 0;
  long long p = 0;
  if (c < n_cells) {
    const int k = (int)(c % (nz - 1)), j = (int)((c / (nz - 1)) % (ny - 1)), i = (int)(c / ((long long)(ny - 1) * (nz - 1)));
    p = ((long long)i * ny + j) * nz + k;
#pragma unroll
    for (int code = 0; code < 8; ++code) {
      const float v = f[p + ((long long)(code >> 2) * ny + ((code >> 1) & 1)) * nz + (code & 1)];
      if (hn_iso_inside(v, iso)) inside |= 1u << code;
    }
    if (inside != 0u && inside != 255u) {
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        unsigned m4 = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) m4 |= ((inside >> hn_tet_table.corner[q][t]) & 1u) << t;
        count += hn_tet_table.entry[q][m4] & 3u;
      }
    }
  }
  int total;
  const int rank = hn_iso_block_rank<4, true>(count, wave_sums, total);
  if (!EMIT) {
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
    return;
  }
  if (count == 0u) return;
  long long fid = block_offsets[blockIdx.x] + rank;
  for (int q = 0; q < 6; ++q) {
    unsigned m4 = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) m4 |= ((inside >> hn_tet_table.corner[q][t]) & 1u) << t;
    const unsigned e = hn_tet_table.entry[q][m4];
    const int n_tri = (int)(e & 3u);
    for (int r = 0; r < n_tri; ++r) {
      int32_t* o = faces + 3 * (size_t)fid;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const unsigned ab = (e >> (2 + 4 * (3 * r + s))) & 15u;
        const int ca = hn_tet_table.corner[q][ab & 3u], cb = hn_tet_table.corner[q][ab >> 2];
        const long long owner = p + ((long long)(ca >> 2) * ny + ((ca >> 1) & 1)) * nz + (ca & 1);
        o[s] = slots[7 * (size_t)owner + hn_tet_table.dir_class[cb ^ ca]];
      }
      ++fid;
    }
  }
}

extern "C" int hn_iso_faces(const float* grid_dev, int nx, int ny, int nz, float iso, const int32_t* slots_dev,
                            const int64_t* block_offsets_dev, int32_t* block_counts_dev, int32_t* faces_dev,
                            hnStream_t stream) {
  HnLattice g;
  if (grid_dev == nullptr || !hn_lattice(nx, ny, nz, nullptr, &g)) return -2;
  const bool emit = faces_dev != nullptr;
  if (emit ? (slots_dev == nullptr || block_offsets_dev == nullptr) : block_counts_dev == nullptr) return -2;
  const long long n_cells = (long long)(nx - 1) * (ny - 1) * (nz - 1);
  const dim3 grid((unsigned)((n_cells + HN_ISO_BLOCK - 1) / HN_ISO_BLOCK));
  if (emit)
    hipLaunchKernelGGL(hn_iso_faces_kernel<true>, grid, dim3(HN_ISO_BLOCK), 0, (hipStream_t)stream, grid_dev, nx, ny, nz,
                       iso, slots_dev, block_offsets_dev, block_counts_dev, faces_dev);
  else
    hipLaunchKernelGGL(hn_iso_faces_kernel<false>, grid, dim3(HN_ISO_BLOCK), 0, (hipStream_t)stream, grid_dev, nx, ny, nz,
                       iso, slots_dev, block_offsets_dev, block_counts_dev, faces_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Connected components of an indexed mesh.  Two vertices are connected when a face holds both; the label of a vertex is
// the SMALLEST vertex id of its component.  parent[] (int32, V entries) starts as the identity and only ever goes down:
//   invariant  parent[v] <= v, and parent[v] is a vertex of v's component.
// One round = two launches:
//   hook   per face (a, b, c): m = min(parent[a], parent[b], parent[c]); atomicMin(parent[x], m) for x in a, b, c and for
//          their three parents — a round of min-label propagation over the faces plus the hooking of the old roots;
//   jump   per vertex: follow parent at most HN_CC_HOPS times (ids strictly decrease along the way, nobody is waited
//          for) and store where it got to.
// A launch that lowers an entry stores the round number into flags[1]; the host stops after the first round that leaves
// it untouched.  At that point every face sees one value and parent[parent[v]] == parent[v]: every component is a star
// around one root r <= all its members that is itself a member, hence its smallest id.
// Rounds needed: plain min-label propagation L[v] <- min over the faces of v reaches the fixed point in at most V - 1
// rounds (the smallest id travels one face per round, a path has at most V - 1 edges) and every parent[v] here is, by
// induction over the rounds, <= that L[v] (the hook does at least that step on values that are already lower, the jump
// only lowers) and >= the component's smallest id: V - 1 rounds that change something at most, one more that does not.
// The caller's cap is V + 1.  In practice the jump makes it logarithmic (DESIGN.md 3.9 has the measured counts).
// Out-of-range ids: hn_cc_init reports them in flags[0]; hook and size launches skip such faces, so nothing is ever
// written outside parent[0 .. V).
// ------------------------------------------------------------------------------------------------
#define HN_CC_HOPS 16

__global__ __launch_bounds__(256) void hn_cc_init_kernel(const int32_t* __restrict__ faces, long long n_faces,
                                                         int32_t* __restrict__ parent, long long n_vertices,
                                                         int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) flags[1] = 0;
  if (i < n_vertices) parent[i] = (int32_t)i;
  if (i < n_faces) {
    const int32_t a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
    // every thread that sees a bad id stores the same 1: no ordering to depend on
    if (a < 0 || b < 0 || c < 0 || a >= n_vertices || b >= n_vertices || c >= n_vertices) flags[0] = 1;
  }
}

__global__ __launch_bounds__(256) void hn_cc_hook_kernel(const int32_t* __restrict__ faces, long long n_faces,
                                                         int32_t* parent, long long n_vertices, int round,
                                                         int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_faces) return;
  const int32_t v[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
  if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[0] >= n_vertices || v[1] >= n_vertices || v[2] >= n_vertices) return;
  // relaxed loads of words that other threads lower meanwhile: any value read is a member of the component that is <= the
  // value at the start of the round, which is all the argument above needs
  const int32_t p[3] = {__hip_atomic_load(parent + v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                        __hip_atomic_load(parent + v[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                        __hip_atomic_load(parent + v[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
  const int32_t m = min(p[0], min(p[1], p[2]));
  bool lowered = false;
  // integer atomicMin: the entry ends up as the minimum of everything offered to it, whatever the order of arrival, and
  // the fixed point (the smallest id of the component) does not depend on scheduling at all — only the number of rounds may
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (p[s] > m) {
      lowered |= atomicMin(parent + v[s], m) > m;
      lowered |= atomicMin(parent + p[s], m) > m;       // p[s] is a vertex id in [0, V): the invariant
    }
  }
  if (lowered) flags[1] = round;
}

__global__ __launch_bounds__(256) void hn_cc_jump_kernel(int32_t* parent, long long n_vertices, int round,
                                                         int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_vertices) return;
  const int32_t first = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int32_t p = first;
  for (int hop = 0; hop < HN_CC_HOPS; ++hop) {
    const int32_t q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == p) break;
    p = q;                                              // q < p: the walk ends, with or without the hop limit
  }
  if (p < first) {
    atomicMin(parent + i, p);                           // never raises what a concurrent walk already stored
    flags[1] = round;
  }
}

extern "C" int hn_cc_init(const int32_t* faces_dev, long long n_faces, int32_t* parent_dev, long long n_vertices,
                          int32_t* flags_dev, hnStream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_faces > 2147483647ll || n_vertices > 2147483647ll) return -2;
  if (flags_dev == nullptr || (n_faces > 0 && faces_dev == nullptr) || (n_vertices > 0 && parent_dev == nullptr)) return -2;
  const long long n = n_faces > n_vertices ? n_faces : n_vertices;
  hipLaunchKernelGGL(hn_cc_init_kernel, dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)), dim3(256), 0,
                     (hipStream_t)stream, faces_dev, n_faces, parent_dev, n_vertices, flags_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_cc_round(const int32_t* faces_dev, long long n_faces, int32_t* parent_dev, long long n_vertices,
                           int round, int32_t* flags_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_vertices <= 0 || n_faces > 2147483647ll || n_vertices > 2147483647ll || round < 1) return -2;
  if (faces_dev == nullptr || parent_dev == nullptr || flags_dev == nullptr) return -2;
  hipLaunchKernelGGL(hn_cc_hook_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     faces_dev, n_faces, parent_dev, n_vertices, round, flags_dev);
  HN_CHECK_LAUNCH();
  hipLaunchKernelGGL(hn_cc_jump_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     parent_dev, n_vertices, round, flags_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_cc_sizes: sizes[label] += 1 per face, label = labels[first vertex of the face]; sizes (V) zeroed by the caller.
// Integer sums do not depend on the order of arrival.  Nearly every face of an extracted mesh carries the label of the one
// large component, so the adds are folded before they reach memory: a workgroup takes HN_CC_SIZES_TILE faces, counts those
// that carry the label of its first face in registers, then LDS, and sends ONE add for them; the lanes of a wave that
// hold any other label send one add per distinct label.  A face with an id, or a label, outside [0, V) is skipped and
// reported in flags[0].
// ------------------------------------------------------------------------------------------------
#define HN_CC_SIZES_PER_THREAD 8
#define HN_CC_SIZES_TILE (256 * HN_CC_SIZES_PER_THREAD)

HN_DEV int32_t hn_cc_face_label(const int32_t* __restrict__ labels, const int32_t* __restrict__ faces, long long i,
                                long long n_vertices, int32_t* __restrict__ flags) {
  const int32_t a = faces[3 * i];
  int32_t label = -1;
  if (a >= 0 && a < n_vertices) label = labels[a];
  if (label < 0 || label >= n_vertices) {
    label = -1;
    flags[0] = 1;
  }
  return label;
}

__global__ __launch_bounds__(256) void hn_cc_sizes_kernel(const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ faces, long long n_faces,
                                                          long long n_vertices, int32_t* __restrict__ sizes,
                                                          int32_t* __restrict__ flags) {
  __shared__ int block_count;
  const long long base = (long long)blockIdx.x * HN_CC_SIZES_TILE;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) block_count = 0;
  __syncthreads();
  const int32_t common = hn_cc_face_label(labels, faces, base, n_vertices, flags);     // base < n_faces: the grid's size
  int mine = 0;
  for (int j = 0; j < HN_CC_SIZES_PER_THREAD; ++j) {
    const long long i = base + (long long)j * 256 + threadIdx.x;
    int32_t label = i < n_faces ? hn_cc_face_label(labels, faces, i, n_vertices, flags) : -1;
    if (label >= 0 && label == common) {
      ++mine;
      label = -1;
    }
    unsigned long long todo = __ballot(label >= 0);
    while (todo != 0ull) {                               // wave-uniform: `todo` is the same in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int32_t lead = __shfl(label, leader, 64);
      const unsigned long long same = __ballot(label == lead) & todo;
      if (lane == leader) atomicAdd(sizes + lead, (int32_t)__popcll(same));
      todo &= ~same;
    }
  }
  if (mine != 0) atomicAdd(&block_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && block_count != 0) atomicAdd(sizes + common, (int32_t)block_count);
}

extern "C" int hn_cc_sizes(const int32_t* labels_dev, const int32_t* faces_dev, long long n_faces, long long n_vertices,
                           int32_t* sizes_dev, int32_t* flags_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_vertices <= 0 || n_faces > 2147483647ll || n_vertices > 2147483647ll) return -2;
  if (labels_dev == nullptr || faces_dev == nullptr || sizes_dev == nullptr || flags_dev == nullptr) return -2;
  hipLaunchKernelGGL(hn_cc_sizes_kernel, dim3((unsigned)((n_faces + HN_CC_SIZES_TILE - 1) / HN_CC_SIZES_TILE)), dim3(256), 0,
                     (hipStream_t)stream, labels_dev, faces_dev, n_faces, n_vertices, sizes_dev, flags_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Filtering.  keep_comp[label] (one byte per vertex id, non-zero = the component stays) ->
//   hn_mesh_keep     vkeep[v] = keep_comp[labels[v]], fkeep[f] = keep_comp[labels[first vertex of f]] (int32 0 / 1, ready
//                    for an inclusive scan; a face with an id outside [0, V) is dropped)
//   hn_mesh_compact  vscan / fscan = the inclusive scans: vertex_index[vscan[v] - 1] = v for a kept v, and a kept face goes
//                    to row fscan[f] - 1 with every id replaced by vscan[id] - 1 — relative orders kept, no atomics
//   hn_gather_rows   dst[r] = src[index[r]] for rows of row_bytes bytes (words when everything is 4-byte aligned)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_mesh_keep_kernel(const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ faces,
                                                           const uint8_t* __restrict__ keep_comp, long long n_vertices,
                                                           long long n_faces, int32_t* __restrict__ vkeep,
                                                           int32_t* __restrict__ fkeep) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_vertices) {
    const int32_t l = labels[i];
    vkeep[i] = (l >= 0 && l < n_vertices && keep_comp[l] != 0) ? 1 : 0;
  }
  if (i < n_faces) {
    const int32_t a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
    int32_t k = 0;
    if (a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices) {
      const int32_t l = labels[a];
      k = (l >= 0 && l < n_vertices && keep_comp[l] != 0) ? 1 : 0;
    }
    fkeep[i] = k;
  }
}

extern "C" int hn_mesh_keep(const int32_t* labels_dev, const int32_t* faces_dev, const uint8_t* keep_comp_dev,
                            long long n_vertices, long long n_faces, int32_t* vkeep_dev, int32_t* fkeep_dev,
                            hnStream_t stream) {
  if (n_vertices <= 0 || n_faces < 0 || n_faces > 2147483647ll || n_vertices > 2147483647ll) return -2;
  if (labels_dev == nullptr || keep_comp_dev == nullptr || vkeep_dev == nullptr) return -2;
  if (n_faces > 0 && (faces_dev == nullptr || fkeep_dev == nullptr)) return -2;
  const long long n = n_faces > n_vertices ? n_faces : n_vertices;
  hipLaunchKernelGGL(hn_mesh_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, labels_dev,
                     faces_dev, keep_comp_dev, n_vertices, n_faces, vkeep_dev, fkeep_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

__global__ __launch_bounds__(256) void hn_mesh_compact_kernel(const int32_t* __restrict__ faces,
                                                              const int32_t* __restrict__ vscan,
                                                              const int32_t* __restrict__ fscan, long long n_vertices,
                                                              long long n_faces, long long n_vertices_out,
                                                              long long n_faces_out, int32_t* __restrict__ vertex_index,
                                                              int32_t* __restrict__ faces_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_vertices) {
    const int32_t s = vscan[i], before = i > 0 ? vscan[i - 1] : 0;
    if (s != before && s >= 1 && s <= n_vertices_out) vertex_index[s - 1] = (int32_t)i;
  }
  if (i < n_faces) {
    const int32_t s = fscan[i], before = i > 0 ? fscan[i - 1] : 0;
    if (s != before && s >= 1 && s <= n_faces_out) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int32_t id = faces[3 * i + c];                // a kept face has its ids in range (hn_mesh_keep)
        faces_out[3 * (size_t)(s - 1) + c] = (id >= 0 && id < n_vertices) ? vscan[id] - 1 : -1;
      }
    }
  }
}

extern "C" int hn_mesh_compact(const int32_t* faces_dev, const int32_t* vscan_dev, const int32_t* fscan_dev,
                               long long n_vertices, long long n_faces, long long n_vertices_out, long long n_faces_out,
                               int32_t* vertex_index_dev, int32_t* faces_out_dev, hnStream_t stream) {
  if (n_vertices <= 0 || n_faces < 0 || n_faces > 2147483647ll || n_vertices > 2147483647ll) return -2;
  if (n_vertices_out < 0 || n_vertices_out > n_vertices || n_faces_out < 0 || n_faces_out > n_faces) return -2;
  if (vscan_dev == nullptr || (n_vertices_out > 0 && vertex_index_dev == nullptr)) return -2;
  if (n_faces > 0 && (faces_dev == nullptr || fscan_dev == nullptr)) return -2;
  if (n_faces_out > 0 && faces_out_dev == nullptr) return -2;
  const long long n = n_faces > n_vertices ? n_faces : n_vertices;
  hipLaunchKernelGGL(hn_mesh_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces_dev,
                     vscan_dev, fscan_dev, n_vertices, n_faces, n_vertices_out, n_faces_out, vertex_index_dev,
                     faces_out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void hn_gather_rows_kernel(const T* __restrict__ src, long long n_src,
                                                             const int32_t* __restrict__ index, long long n_rows,
                                                             int row_items, T* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows * row_items) return;
  const long long r = i / row_items;
  const int c = (int)(i - r * row_items);
  const int32_t s = index[r];
  dst[i] = (s >= 0 && s < n_src) ? src[(size_t)s * row_items + c] : T(0);
}

extern "C" int hn_gather_rows(const void* src_dev, long long n_src, const int32_t* index_dev, long long n_rows,
                              long long row_bytes, void* dst_dev, hnStream_t stream) {
  if (n_src <= 0 || n_rows <= 0 || row_bytes <= 0 || n_src > 2147483647ll || n_rows > 2147483647ll || row_bytes > 65536) return -2;
  if (src_dev == nullptr || index_dev == nullptr || dst_dev == nullptr) return -2;
  const bool words = row_bytes % 4 == 0 && (uintptr_t)src_dev % 4 == 0 && (uintptr_t)dst_dev % 4 == 0;
  const long long items = words ? row_bytes / 4 : row_bytes;
  const long long blocks = (n_rows * items + 255) / 256;
  if (blocks > 2147483647ll) return -2;
  if (words)
    hipLaunchKernelGGL(hn_gather_rows_kernel<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)src_dev, n_src, index_dev, n_rows, (int)items, (uint32_t*)dst_dev);
  else
    hipLaunchKernelGGL(hn_gather_rows_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src_dev, n_src, index_dev, n_rows, (int)items, (uint8_t*)dst_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_vertex_viewdirs: out[r] = the direction a colour query looks along at vertex i = min(start + r, V - 1), r < count
// (rows past the mesh, the padding of a last chunk, repeat the last vertex).  u = -normal[i] (cam_host == NULL: head-on
// from outside) or vertex[i] - c; out = u / |u| with |u| = sqrt((ux*ux + uy*uy) + uz*uz), every operation fp32 and
// rounded on its own; |u| = 0 (or NaN) gives (0, 0, 1), the direction query_points itself defaults to.
// ------------------------------------------------------------------------------------------------
struct HnVec3 { float v[3]; };

__global__ __launch_bounds__(256) void hn_vertex_viewdirs_kernel(const float* __restrict__ vertices,
                                                                 const float* __restrict__ normals, long long n_vertices,
                                                                 long long start, long long count, int has_cam,
                                                                 HnVec3 cam, float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= count) return;
  long long i = start + r;
  if (i > n_vertices - 1) i = n_vertices - 1;
  float u[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    u[c] = has_cam != 0 ? __fsub_rn(vertices[3 * (size_t)i + c], cam.v[c]) : -normals[3 * (size_t)i + c];
  const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(u[0], u[0]), __fmul_rn(u[1], u[1])), __fmul_rn(u[2], u[2])));
  const bool ok = len > 0.0f;
  float* o = out + 3 * (size_t)r;
  o[0] = ok ? __fdiv_rn(u[0], len) : 0.0f;
  o[1] = ok ? __fdiv_rn(u[1], len) : 0.0f;
  o[2] = ok ? __fdiv_rn(u[2], len) : 1.0f;
}

extern "C" int hn_vertex_viewdirs(const float* vertices_dev, const float* normals_dev, long long n_vertices,
                                  long long start, long long count, const float* cam_host, float* out_dev,
                                  hnStream_t stream) {
  if (n_vertices <= 0 || n_vertices > 2147483647ll || start < 0 || start >= n_vertices || count <= 0 ||
      count > 2147483647ll)
    return -2;
  if (out_dev == nullptr || (cam_host != nullptr ? vertices_dev == nullptr : normals_dev == nullptr)) return -2;
  HnVec3 cam = {{0.f, 0.f, 0.f}};
  if (cam_host != nullptr)
    for (int c = 0; c < 3; ++c) cam.v[c] = cam_host[c];
  hipLaunchKernelGGL(hn_vertex_viewdirs_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, normals_dev, n_vertices, start, count, cam_host != nullptr ? 1 : 0, cam, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
