// Mesh-to-mesh distance for gfx950: area-weighted surface samples and the exact nearest point of a triangle mesh.
//
// Definition (DESIGN.md 3.13 holds it in full; tests/mesh_distance_restated.py restates it in NumPy float32, bit for bit).
// Every fp32 operation that decides a result is rounded on its own (__f*_rn; the library is built with contraction off);
// dot(u, v) = (ux*vx + uy*vy) + uz*vz.
//   weights   a2_f = sqrt(dot(n, n)), n = (B - A) x (C - A), each component one product minus another; 0 unless finite.
//             The caller turns them into integers w_f = (int64)((a2_f / max a2) * 2^24) and their inclusive scan cdf.
//   sample k  h_j = splitmix64(key + 3 k + j), key = splitmix64(seed); t = mulhi64(h_0, W), W = cdf[F - 1]; face = the
//             first f with cdf[f] > t; u1, u2 = (h_1 >> 40) * 2^-24, (h_2 >> 40) * 2^-24; s = sqrt(u1);
//             b = (1 - s, s * (1 - u2), s * u2); point = (b0*A + b1*B) + b2*C per coordinate.
//   grid      R = (rx, ry, rz) cells of side cell_c over the box from lo; idx_c(x) = floorf((x - lo_c) / cell_c) clamped to
//             [0, R_c - 1] (a NaN gives 0); cell = (iz * ry + iy) * rx + ix.  A face is listed in every cell of
//             [idx(min corner), idx(max corner)]: idx is monotone, so every point of the face falls into a listed cell.
//   closest   the point of a triangle closest to p by Voronoi regions (Ericson, Real-Time Collision Detection 5.1.5), in
//             the operation order of hn_md_closest below; a zero denominator gives the parameter 0, a sum of the three
//             interior weights that is not > 0 gives A: never a NaN out of finite input.  d2 = dot(p - q, p - q).
//   query     the lexicographic minimum of (d2, face id) over the faces with d2 < +inf.  The search walks Chebyshev shells
//             r = 0, 1, ... of cells around the query's cell and stops once every cell was visited or best d2 < bound^2
//             (hn_md_bound: the gap to the nearest side of the visited block that is not the grid's edge, shrunk by the
//             roundings of idx and of d2): which faces it skips changes no result.
// Nothing here depends on scheduling: no atomics but the plain store of the same 1 into an error flag.
#include "hn_common.h"

// Limits the host halves mirror (ops/mesh.py; tests/test_mesh_distance_host.py compares the two)
#define HN_MD_MAX_RES 256      // grid cells per axis: a cell index fits 24 bits, a face's cell count an int32
#define HN_MD_TRI_FLOATS 12    // floats per packed triangle (hn_md_pack): A, B, C, three of padding
#define HN_MD_WEIGHT_BITS 24   // the largest face has the integer weight 2^24 (the caller's cdf)

#define HN_MD_U24 5.9604644775390625e-8f      // 2^-24
#define HN_MD_SHRINK 0.99999f                 // the relative margin of the stop rule
#define HN_MD_SLACK 9.5367431640625e-7f       // 16 * 2^-24: its absolute margin, times (|p_c| + |lo_c| + R_c * cell_c)

struct HnMdGrid {
  float lo[3], cell[3];
  int res[3];
};

// host: false unless 1 <= R_c <= HN_MD_MAX_RES, every cell side positive and finite, every lo finite
static bool hn_md_grid(const float* lo_host, const float* cell_host, int rx, int ry, int rz, HnMdGrid* g) {
  if (lo_host == nullptr || cell_host == nullptr) return false;
  const int res[3] = {rx, ry, rz};
  for (int c = 0; c < 3; ++c) {
    const float o = lo_host[c], s = cell_host[c];
    if (res[c] < 1 || res[c] > HN_MD_MAX_RES) return false;
    if (!(s > 0.0f) || !(s <= 3.402823466e38f) || !(o >= -3.402823466e38f && o <= 3.402823466e38f)) return false;
    g->lo[c] = o;
    g->cell[c] = s;
    g->res[c] = res[c];
  }
  return true;
}

HN_DEV float hn_md_dot(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

HN_DEV float hn_md_dop(float a, float b, float c, float d) { return __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, d)); }

// the cell index of coordinate x along axis c; faces and queries share it
HN_DEV int hn_md_idx(const HnMdGrid& g, int c, float x) {
  const float q = floorf(__fdiv_rn(__fsub_rn(x, g.lo[c]), g.cell[c]));
  const int top = g.res[c] - 1;
  if (!(q >= 1.0f)) return 0;
  return q >= (float)top ? top : (int)q;
}

HN_DEV bool hn_md_ids_ok(const int32_t* __restrict__ faces, long long f, long long n_vertices, int32_t* v) {
  v[0] = faces[3 * f];
  v[1] = faces[3 * f + 1];
  v[2] = faces[3 * f + 2];
  return v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] < n_vertices && v[1] < n_vertices && v[2] < n_vertices;
}

// ------------------------------------------------------------------------------------------------
// hn_md_face_weights: twice the area of every face
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_md_face_weights_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                                 const int32_t* __restrict__ faces, long long n_faces,
                                                                 float* __restrict__ a2, int32_t* __restrict__ err) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  int32_t v[3];
  float out = 0.0f;
  if (hn_md_ids_ok(faces, f, n_vertices, v)) {
    float e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = vertices[3 * (size_t)v[0] + c];
      e1[c] = __fsub_rn(vertices[3 * (size_t)v[1] + c], a);
      e2[c] = __fsub_rn(vertices[3 * (size_t)v[2] + c], a);
    }
    const float n[3] = {hn_md_dop(e1[1], e2[2], e1[2], e2[1]), hn_md_dop(e1[2], e2[0], e1[0], e2[2]),
                        hn_md_dop(e1[0], e2[1], e1[1], e2[0])};
    // sqrtf, not __fsqrt_rn: the latter is the hardware's approximate root here, sqrtf the correctly rounded one
    const float len = sqrtf(hn_md_dot(n, n));
    if (len <= 3.402823466e38f) out = len;      // false for NaN and +inf
  } else {
    err[0] = 1;      // whoever gets there stores the same 1
  }
  a2[f] = out;
}

extern "C" int hn_md_face_weights(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                                  float* a2_dev, int32_t* err_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll) return -2;
  if (vertices_dev == nullptr || faces_dev == nullptr || a2_dev == nullptr || err_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_md_face_weights_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, faces_dev, n_faces, a2_dev, err_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_md_sample: sample k of the surface
// ------------------------------------------------------------------------------------------------
HN_DEV uint64_t hn_md_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void hn_md_sample_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                           const int32_t* __restrict__ faces, long long n_faces,
                                                           const int64_t* __restrict__ cdf, long long n, uint64_t key,
                                                           float* __restrict__ points, int32_t* __restrict__ face_out,
                                                           float* __restrict__ bary) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const uint64_t h0 = hn_md_splitmix64(key + 3ull * (uint64_t)k), h1 = hn_md_splitmix64(key + 3ull * (uint64_t)k + 1ull),
                 h2 = hn_md_splitmix64(key + 3ull * (uint64_t)k + 2ull);
  const int64_t total = cdf[n_faces - 1];
  const int64_t t = (int64_t)__umul64hi(h0, total > 0 ? (uint64_t)total : 0ull);
  long long lo = 0, hi = n_faces - 1;      // the first f with cdf[f] > t; t < total, so the last face at the latest
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > t) hi = mid; else lo = mid + 1;
  }
  const float u1 = __fmul_rn((float)(h1 >> 40), HN_MD_U24), u2 = __fmul_rn((float)(h2 >> 40), HN_MD_U24);
  const float s = sqrtf(u1);
  const float b[3] = {__fsub_rn(1.0f, s), __fmul_rn(s, __fsub_rn(1.0f, u2)), __fmul_rn(s, u2)};
  int32_t v[3];
  const bool ok = hn_md_ids_ok(faces, lo, n_vertices, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x = NAN;
    if (ok)
      x = __fadd_rn(__fadd_rn(__fmul_rn(b[0], vertices[3 * (size_t)v[0] + c]), __fmul_rn(b[1], vertices[3 * (size_t)v[1] + c])),
                    __fmul_rn(b[2], vertices[3 * (size_t)v[2] + c]));
    points[3 * (size_t)k + c] = x;
    bary[3 * (size_t)k + c] = b[c];
  }
  face_out[k] = (int32_t)lo;
}

extern "C" int hn_md_sample(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                            const int64_t* cdf_dev, long long n, long long seed, float* points_dev, int32_t* face_dev,
                            float* bary_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll || n <= 0 || n > 2147483647ll)
    return -2;
  if (vertices_dev == nullptr || faces_dev == nullptr || cdf_dev == nullptr || points_dev == nullptr || face_dev == nullptr ||
      bary_dev == nullptr)
    return -3;
  uint64_t key = (uint64_t)seed + 0x9E3779B97F4A7C15ull;      // splitmix64(seed) on the host
  key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
  key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
  key = key ^ (key >> 31);
  hipLaunchKernelGGL(hn_md_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices_dev,
                     n_vertices, faces_dev, n_faces, cdf_dev, n, key, points_dev, face_dev, bary_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_md_pack: tri[f] = A, B, C, 0, 0, 0 (HN_MD_TRI_FLOATS floats, three 16-byte loads); NaN for a face with an id outside
// [0, V), which also stores 1 into err[0]
// ------------------------------------------------------------------------------------------------
static_assert(HN_MD_TRI_FLOATS == 12, "a packed triangle is three float4");

__global__ __launch_bounds__(256) void hn_md_pack_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                         const int32_t* __restrict__ faces, long long n_faces,
                                                         float* __restrict__ tri, int32_t* __restrict__ err) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  int32_t v[3];
  const bool ok = hn_md_ids_ok(faces, f, n_vertices, v);
  if (!ok) err[0] = 1;
  float* out = tri + HN_MD_TRI_FLOATS * (size_t)f;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * j + c] = ok ? vertices[3 * (size_t)v[j] + c] : NAN;
  out[9] = out[10] = out[11] = 0.0f;
}

extern "C" int hn_md_pack(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                          float* tri_dev, int32_t* err_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll) return -2;
  if (vertices_dev == nullptr || faces_dev == nullptr || tri_dev == nullptr || err_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_md_pack_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, faces_dev, n_faces, tri_dev, err_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_md_cell_count / hn_md_cell_fill: the (cell, face) pairs of the grid.  A packed triangle that holds a NaN has none.
// ------------------------------------------------------------------------------------------------
HN_DEV bool hn_md_face_cells(const float* __restrict__ tri, long long f, const HnMdGrid& g, int* first, int* last) {
  const float* t = tri + HN_MD_TRI_FLOATS * (size_t)f;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = t[c], b = t[3 + c], cc = t[6 + c];
    ok = ok && a == a && b == b && cc == cc;
    first[c] = hn_md_idx(g, c, fminf(fminf(a, b), cc));
    last[c] = hn_md_idx(g, c, fmaxf(fmaxf(a, b), cc));
  }
  return ok;
}

__global__ __launch_bounds__(256) void hn_md_cell_count_kernel(const float* __restrict__ tri, long long n_faces, HnMdGrid g,
                                                               int32_t* __restrict__ counts) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  int first[3], last[3];
  int32_t n = 0;
  if (hn_md_face_cells(tri, f, g, first, last))
    n = (last[0] - first[0] + 1) * (last[1] - first[1] + 1) * (last[2] - first[2] + 1);      // <= 256^3
  counts[f] = n;
}

extern "C" int hn_md_cell_count(const float* tri_dev, long long n_faces, const float* lo_host, const float* cell_host, int rx,
                                int ry, int rz, int32_t* counts_dev, hnStream_t stream) {
  HnMdGrid g;
  if (n_faces <= 0 || n_faces > 2147483647ll || !hn_md_grid(lo_host, cell_host, rx, ry, rz, &g)) return -2;
  if (tri_dev == nullptr || counts_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_md_cell_count_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     tri_dev, n_faces, g, counts_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

__global__ __launch_bounds__(256) void hn_md_cell_fill_kernel(const float* __restrict__ tri, long long n_faces, HnMdGrid g,
                                                              const int64_t* __restrict__ ends, long long n_pairs,
                                                              int32_t* __restrict__ pair_cell, int32_t* __restrict__ pair_face) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  int first[3], last[3];
  if (!hn_md_face_cells(tri, f, g, first, last)) return;
  const long long count = (long long)(last[0] - first[0] + 1) * (last[1] - first[1] + 1) * (last[2] - first[2] + 1);
  long long row = ends[f] - count;
  for (int iz = first[2]; iz <= last[2]; ++iz)
    for (int iy = first[1]; iy <= last[1]; ++iy)
      for (int ix = first[0]; ix <= last[0]; ++ix, ++row) {
        if (row < 0 || row >= n_pairs) continue;
        pair_cell[row] = (iz * g.res[1] + iy) * g.res[0] + ix;
        pair_face[row] = (int32_t)f;
      }
}

extern "C" int hn_md_cell_fill(const float* tri_dev, long long n_faces, const float* lo_host, const float* cell_host, int rx,
                               int ry, int rz, const int64_t* ends_dev, long long n_pairs, int32_t* pair_cell_dev,
                               int32_t* pair_face_dev, hnStream_t stream) {
  HnMdGrid g;
  if (n_faces <= 0 || n_faces > 2147483647ll || n_pairs <= 0 || n_pairs > 2147483647ll ||
      !hn_md_grid(lo_host, cell_host, rx, ry, rz, &g))
    return -2;
  if (tri_dev == nullptr || ends_dev == nullptr || pair_cell_dev == nullptr || pair_face_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_md_cell_fill_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     tri_dev, n_faces, g, ends_dev, n_pairs, pair_cell_dev, pair_face_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_md_cell_keys: the (clamped) cell of every query point, the key the caller sorts the queries by
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_md_cell_keys_kernel(const float* __restrict__ points, long long n, HnMdGrid g,
                                                              int32_t* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ix = hn_md_idx(g, 0, points[3 * (size_t)i]), iy = hn_md_idx(g, 1, points[3 * (size_t)i + 1]),
            iz = hn_md_idx(g, 2, points[3 * (size_t)i + 2]);
  keys[i] = (iz * g.res[1] + iy) * g.res[0] + ix;
}

extern "C" int hn_md_cell_keys(const float* points_dev, long long n, const float* lo_host, const float* cell_host, int rx,
                               int ry, int rz, int32_t* keys_dev, hnStream_t stream) {
  HnMdGrid g;
  if (n <= 0 || n > 2147483647ll || !hn_md_grid(lo_host, cell_host, rx, ry, rz, &g)) return -2;
  if (points_dev == nullptr || keys_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_md_cell_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points_dev,
                     n, g, keys_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_md_query
// ------------------------------------------------------------------------------------------------
// q = the point of triangle (a, b, c) closest to p; returns d2 = |p - q|^2
HN_DEV float hn_md_closest(const float* p, const float* a, const float* b, const float* c, float* q) {
  float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = __fsub_rn(b[k], a[k]);
    ac[k] = __fsub_rn(c[k], a[k]);
    ap[k] = __fsub_rn(p[k], a[k]);
    bp[k] = __fsub_rn(p[k], b[k]);
    cp[k] = __fsub_rn(p[k], c[k]);
  }
  const float d1 = hn_md_dot(ab, ap), d2 = hn_md_dot(ac, ap), d3 = hn_md_dot(ab, bp), d4 = hn_md_dot(ac, bp),
              d5 = hn_md_dot(ab, cp), d6 = hn_md_dot(ac, cp);
  const float vc = hn_md_dop(d1, d4, d3, d2), vb = hn_md_dop(d5, d2, d1, d6), va = hn_md_dop(d3, d6, d5, d4);
  const float e43 = __fsub_rn(d4, d3), e56 = __fsub_rn(d5, d6);
  // q = (base + s * u) + t * ac: the region picks base, u and the two parameters (values, not pointers: registers)
  float base[3] = {a[0], a[1], a[2]}, u[3] = {ab[0], ab[1], ab[2]};
  float s = 0.0f, t = 0.0f;
  if (d1 <= 0.0f && d2 <= 0.0f) {                              // vertex A
  } else if (d3 >= 0.0f && d4 <= d3) {                         // vertex B
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = b[k];
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {         // edge AB
    const float den = __fsub_rn(d1, d3);
    s = den != 0.0f ? __fdiv_rn(d1, den) : 0.0f;
  } else if (d6 >= 0.0f && d5 <= d6) {                         // vertex C
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = c[k];
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {         // edge AC
    const float den = __fsub_rn(d2, d6);
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = ac[k];
    s = den != 0.0f ? __fdiv_rn(d2, den) : 0.0f;
  } else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {       // edge BC
    const float den = __fadd_rn(e43, e56);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      base[k] = b[k];
      u[k] = __fsub_rn(c[k], b[k]);
    }
    s = den != 0.0f ? __fdiv_rn(e43, den) : 0.0f;
  } else {                                                     // interior
    const float sum = __fadd_rn(__fadd_rn(va, vb), vc);
    if (sum > 0.0f) {
      s = __fdiv_rn(vb, sum);
      t = __fdiv_rn(vc, sum);
    }
  }
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q[k] = __fadd_rn(__fadd_rn(base[k], __fmul_rn(s, u[k])), __fmul_rn(t, ac[k]));
    d[k] = __fsub_rn(p[k], q[k]);
  }
  return hn_md_dot(d, d);
}

// After shell r around cell pc: a lower bound of the fp32 distance of every face that no visited cell lists, 0 when
// there is none to give (DESIGN.md 3.13 derives the margins), +inf when every cell was visited.
HN_DEV float hn_md_bound(const HnMdGrid& g, const float* p, const int* pc, int r) {
  float bound = INFINITY;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float rel = __fsub_rn(p[c], g.lo[c]);
    const float slack = HN_MD_SLACK * (fabsf(p[c]) + fabsf(g.lo[c]) + (float)g.res[c] * g.cell[c]);
    if (pc[c] - r > 0) {
      const float gap = __fsub_rn(rel, __fmul_rn((float)(pc[c] - r), g.cell[c]));
      bound = fminf(bound, gap * HN_MD_SHRINK - slack);
    }
    if (pc[c] + r < g.res[c] - 1) {
      const float gap = __fsub_rn(__fmul_rn((float)(pc[c] + r + 1), g.cell[c]), rel);
      bound = fminf(bound, gap * HN_MD_SHRINK - slack);
    }
  }
  return bound > 0.0f ? bound : 0.0f;      // NaN -> 0
}

__global__ __launch_bounds__(256) void hn_md_query_kernel(const float* __restrict__ points, long long n,
                                                          const int64_t* __restrict__ perm, const float* __restrict__ tri,
                                                          long long n_faces, const int32_t* __restrict__ cell_begin,
                                                          const int32_t* __restrict__ pair_face, long long n_pairs, HnMdGrid g,
                                                          float max_distance, float* __restrict__ distance,
                                                          int32_t* __restrict__ face_out, float* __restrict__ closest) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
  if (slot >= n) return;
  const long long i = perm != nullptr ? perm[slot] : slot;
  if (i < 0 || i >= n) return;
  const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
  float best = INFINITY, bq[3] = {NAN, NAN, NAN};
  int32_t best_face = -1;
  const bool finite = fabsf(p[0]) <= 3.402823466e38f && fabsf(p[1]) <= 3.402823466e38f && fabsf(p[2]) <= 3.402823466e38f;
  if (finite) {
    const int pc[3] = {hn_md_idx(g, 0, p[0]), hn_md_idx(g, 1, p[1]), hn_md_idx(g, 2, p[2])};
    const int rx = g.res[0], ry = g.res[1], rz = g.res[2];
    const int r_max = max(max(max(pc[0], rx - 1 - pc[0]), max(pc[1], ry - 1 - pc[1])), max(pc[2], rz - 1 - pc[2]));
    for (int r = 0; r <= r_max; ++r) {
      const int x0 = max(pc[0] - r, 0), x1 = min(pc[0] + r, rx - 1);
      const int y0 = max(pc[1] - r, 0), y1 = min(pc[1] + r, ry - 1);
      const int z0 = max(pc[2] - r, 0), z1 = min(pc[2] + r, rz - 1);
      for (int iz = z0; iz <= z1; ++iz) {
        const bool z_face = iz == pc[2] - r || iz == pc[2] + r;
        for (int iy = y0; iy <= y1; ++iy) {
          const int row = (iz * ry + iy) * rx;
          const bool whole = z_face || iy == pc[1] - r || iy == pc[1] + r;
          // a whole row of the shell is one run of the pair list (x is the fastest cell axis); an inner row
          // contributes its two end cells, where they lie inside the grid
          for (int part = 0; part < (whole ? 1 : 2); ++part) {
            int c0, c1;
            if (whole) {
              c0 = row + x0;
              c1 = row + x1;
            } else {
              const int ix = part == 0 ? pc[0] - r : pc[0] + r;
              if (ix < 0 || ix > rx - 1) continue;
              c0 = c1 = row + ix;
            }
            long long j = cell_begin[c0], end = cell_begin[c1 + 1];
            if (j < 0) j = 0;
            if (end > n_pairs) end = n_pairs;
            for (; j < end; ++j) {
              const int32_t f = pair_face[j];
              if (f < 0 || f >= n_faces) continue;
              const f32x4* t4 = reinterpret_cast<const f32x4*>(tri + HN_MD_TRI_FLOATS * (size_t)f);
              const f32x4 t0 = t4[0], t1 = t4[1], t2 = t4[2];
              const float a[3] = {t0[0], t0[1], t0[2]}, b[3] = {t0[3], t1[0], t1[1]}, c[3] = {t1[2], t1[3], t2[0]};
              float q[3];
              const float d2 = hn_md_closest(p, a, b, c, q);
              if (d2 < best || (d2 == best && f < best_face)) {
                best = d2;
                best_face = f;
                bq[0] = q[0];
                bq[1] = q[1];
                bq[2] = q[2];
              }
            }
          }
        }
      }
      if (r == r_max) break;
      const float bound = hn_md_bound(g, p, pc, r);
      if (best < __fmul_rn(bound, bound)) break;
      if (max_distance >= 0.0f && bound > max_distance) break;
    }
  }
  // sqrtf: the correctly rounded root
  float dist = finite ? sqrtf(best) : NAN;
  if (finite && max_distance >= 0.0f && !(dist <= max_distance)) {
    dist = INFINITY;
    best_face = -1;
    bq[0] = bq[1] = bq[2] = NAN;
  }
  distance[i] = dist;
  face_out[i] = best_face;
  closest[3 * (size_t)i] = bq[0];
  closest[3 * (size_t)i + 1] = bq[1];
  closest[3 * (size_t)i + 2] = bq[2];
}

extern "C" int hn_md_query(const float* points_dev, long long n, const int64_t* perm_dev, const float* tri_dev,
                           long long n_faces, const int32_t* cell_begin_dev, const int32_t* pair_face_dev, long long n_pairs,
                           const float* lo_host, const float* cell_host, int rx, int ry, int rz, float max_distance,
                           float* distance_dev, int32_t* face_dev, float* closest_dev, hnStream_t stream) {
  HnMdGrid g;
  if (n <= 0 || n > 2147483647ll || n_faces <= 0 || n_faces > 2147483647ll || n_pairs <= 0 || n_pairs > 2147483647ll ||
      !hn_md_grid(lo_host, cell_host, rx, ry, rz, &g) || max_distance != max_distance)
    return -2;
  if (points_dev == nullptr || tri_dev == nullptr || cell_begin_dev == nullptr || pair_face_dev == nullptr ||
      distance_dev == nullptr || face_dev == nullptr || closest_dev == nullptr)
    return -3;
  hipLaunchKernelGGL(hn_md_query_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points_dev, n,
                     perm_dev, tri_dev, n_faces, cell_begin_dev, pair_face_dev, n_pairs, g, max_distance, distance_dev, face_dev,
                     closest_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
