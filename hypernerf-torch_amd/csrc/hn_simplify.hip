// Mesh simplification by vertex clustering (Rossignac-Borrel cells, Lindstrom-style quadric placement), for gfx950.
//
// Definition (DESIGN.md holds it in full; tests/simplify_restated.py restates it in NumPy float32, bit for bit):
//   cells     idx_c = floorf((v_c - origin_c) / cell_c), key = ix | iy << 21 | iz << 42 (int64).  The clusters are the
//             distinct keys in ascending order, the members of a cluster its vertices in ascending vertex id (the caller's
//             stable sort of the keys).
//   cluster   every sum runs over the members in that order, starts at +0 and is fp32 with every operation rounded on
//             its own (__f*_rn; the library is built with contraction off):
//               mean = sum(p) / k
//               quadric placement: r = p - mean, A = sum(n n^T) + (regularization * k) I, b = sum(n * ((nx*rx + ny*ry) + nz*rz)),
//                 d = adj(A) b / det(A) (d = 0 unless det is finite and positive), x = mean + d clamped into the cell box
//                 [origin + idx * cell, that + cell]
//               normal = sum(n) / |sum(n)| with |u| = sqrt((ux*ux + uy*uy) + uz*uz), the zero vector when |u| is not > 0
//               colours: uint8 (2 * sum + k) / (2 k) in integers, fp32 sum / k
//   faces     every face goes through the cluster ids; one with two equal ids is dropped; the others are rotated so that
//             their smallest id comes first, (a, x, y), and named by the sorted triple (a, b, c) = (a, min(x, y), max(x, y))
//             with the sign +1 when x < y (the face winds as (a, b, c)) and -1 otherwise (it winds as (a, c, b)).  The caller
//             sorts the names; the net of a triple is the sum of its signs, and |net| copies leave, as (a, b, c) when net > 0
//             and (a, c, b) when net < 0, triples ascending.  Opposite pairs, the folded flaps of a collapse, cancel.
// Nothing here depends on scheduling: no float atomics, no atomics at all (the `used` marks are plain stores of the
// same 1 by whoever gets there).  One work-item per cluster walks its members; one per sorted face name that ends a
// group of equal names walks that group backwards (a group holds the fine faces that span the same three cells: a
// handful).
#include "hn_common.h"

#define HN_SIMPLIFY_MASK ((1ll << HN_SIMPLIFY_BITS) - 1ll)
#define HN_SIMPLIFY_DROPPED 0x7fffffffffffffffll

struct HnCells {
  float origin[3], cell[3];
};

// host: false unless every cell side is positive and finite and every origin finite
static bool hn_cells(const float* origin_host, const float* cell_host, HnCells* out) {
  if (origin_host == nullptr || cell_host == nullptr) return false;
  for (int c = 0; c < 3; ++c) {
    const float o = origin_host[c], s = cell_host[c];
    if (!(s > 0.0f) || !(s <= 3.402823466e38f) || !(o >= -3.402823466e38f && o <= 3.402823466e38f)) return false;
    out->origin[c] = o;
    out->cell[c] = s;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// hn_simplify_extent: per workgroup of HN_EXTENT_TILE vertices the per-axis minimum (partial[6 b + 0 .. 2]) and maximum
// (partial[6 b + 3 .. 5]); the caller reduces the partials.  Minimum and maximum do not depend on the order they are
// taken in.  A tile that holds a NaN reports NaN in all six, so that the caller sees it.
// ------------------------------------------------------------------------------------------------
#define HN_EXTENT_PER_THREAD 8
static_assert(HN_EXTENT_TILE == 256 * HN_EXTENT_PER_THREAD, "hn_kernels.h: HN_EXTENT_TILE is one workgroup's vertices");

__global__ __launch_bounds__(256) void hn_simplify_extent_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                                 float* __restrict__ partial) {
  __shared__ float wave_ext[4][6];
  __shared__ int wave_bad[4];
  const long long base = (long long)blockIdx.x * HN_EXTENT_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ext[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (int j = 0; j < HN_EXTENT_PER_THREAD; ++j) {
    const long long i = base + (long long)j * 256 + threadIdx.x;
    if (i < n_vertices) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = vertices[3 * (size_t)i + c];
        bad |= !(x == x);
        ext[c] = fminf(ext[c], x);
        ext[3 + c] = fmaxf(ext[3 + c], x);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ext[c] = fminf(ext[c], __shfl_xor(ext[c], off, 64));
      ext[3 + c] = fmaxf(ext[3 + c], __shfl_xor(ext[3 + c], off, 64));
    }
  }
  const bool wave_has_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) wave_ext[wave][c] = ext[c];
    wave_bad[wave] = wave_has_bad ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    float v = wave_ext[0][c];
    for (int w = 1; w < 4; ++w) v = c < 3 ? fminf(v, wave_ext[w][c]) : fmaxf(v, wave_ext[w][c]);
    if ((wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) != 0) v = NAN;
    partial[6 * (size_t)blockIdx.x + c] = v;
  }
}

extern "C" int hn_simplify_extent(const float* vertices_dev, long long n_vertices, float* partial_dev, long long n_partial,
                                  hnStream_t stream) {
  if (n_vertices <= 0 || n_vertices > 2147483647ll || vertices_dev == nullptr || partial_dev == nullptr) return -2;
  const long long blocks = (n_vertices + HN_EXTENT_TILE - 1) / HN_EXTENT_TILE;
  if (n_partial != blocks) return -2;
  hipLaunchKernelGGL(hn_simplify_extent_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vertices_dev,
                     n_vertices, partial_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_simplify_keys: the cell key of every vertex.  The caller has checked the extent (origin <= min, fewer than 2^21
// cells per axis); an index outside [0, 2^21) all the same (a NaN coordinate) is clamped, so that a key is always one.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_simplify_keys_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                               HnCells g, int64_t* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_vertices) return;
  int64_t key = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float q = floorf(__fdiv_rn(__fsub_rn(vertices[3 * (size_t)i + c], g.origin[c]), g.cell[c]));
    long long idx = 0;
    if (q >= 1.0f) idx = q >= (float)HN_SIMPLIFY_MASK ? HN_SIMPLIFY_MASK : (long long)q;
    key |= (int64_t)idx << (HN_SIMPLIFY_BITS * c);
  }
  keys[i] = key;
}

extern "C" int hn_simplify_keys(const float* vertices_dev, long long n_vertices, const float* origin_host,
                                const float* cell_host, int64_t* keys_dev, hnStream_t stream) {
  HnCells g;
  if (n_vertices <= 0 || n_vertices > 2147483647ll || vertices_dev == nullptr || keys_dev == nullptr ||
      !hn_cells(origin_host, cell_host, &g))
    return -2;
  hipLaunchKernelGGL(hn_simplify_keys_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, vertices_dev, n_vertices, g, keys_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_simplify_reduce: the representative of every cluster.  order (V) = the vertex ids sorted by key (stable), starts
// (C + 1) = where every cluster begins in it.  One work-item per cluster: first walk position, normal and colour sums,
// second walk (quadric placement only) the 3 x 3 system around the mean.  A member id outside [0, V) is skipped.
// ------------------------------------------------------------------------------------------------
HN_DEV float hn_dot3(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

// a*b - c*d, every operation rounded on its own
HN_DEV float hn_diff_of_products(float a, float b, float c, float d) { return __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, d)); }

__global__ __launch_bounds__(256) void hn_simplify_reduce_kernel(
    const float* __restrict__ vertices, const float* __restrict__ normals, const void* __restrict__ colors, int color_kind,
    const int32_t* __restrict__ order, const int32_t* __restrict__ starts, const int64_t* __restrict__ cluster_keys,
    long long n_clusters, long long n_vertices, HnCells g, float regularization, int quadric, float* __restrict__ out_vertices,
    float* __restrict__ out_normals, void* __restrict__ out_colors) {
  const long long cl = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cl >= n_clusters) return;
  long long first = starts[cl], last = starts[cl + 1];
  if (first < 0) first = 0;
  if (last > n_vertices) last = n_vertices;
  float sp[3] = {0.f, 0.f, 0.f}, sn[3] = {0.f, 0.f, 0.f}, scf[3] = {0.f, 0.f, 0.f};
  unsigned long long sci[3] = {0ull, 0ull, 0ull};
  long long k = 0;
  for (long long j = first; j < last; ++j) {
    const int32_t m = order[j];
    if (m < 0 || m >= n_vertices) continue;
    ++k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sp[c] = __fadd_rn(sp[c], vertices[3 * (size_t)m + c]);
      if (normals != nullptr) sn[c] = __fadd_rn(sn[c], normals[3 * (size_t)m + c]);
      if (color_kind == 1) sci[c] += ((const uint8_t*)colors)[3 * (size_t)m + c];
      if (color_kind == 2) scf[c] = __fadd_rn(scf[c], ((const float*)colors)[3 * (size_t)m + c]);
    }
  }
  const float kf = (float)k;
  float mean[3], x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = mean[c] = __fdiv_rn(sp[c], kf);
  if (quadric != 0 && normals != nullptr) {
    float axx = 0.f, axy = 0.f, axz = 0.f, ayy = 0.f, ayz = 0.f, azz = 0.f, b[3] = {0.f, 0.f, 0.f};
    for (long long j = first; j < last; ++j) {
      const int32_t m = order[j];
      if (m < 0 || m >= n_vertices) continue;
      float n[3], r[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        n[c] = normals[3 * (size_t)m + c];
        r[c] = __fsub_rn(vertices[3 * (size_t)m + c], mean[c]);
      }
      axx = __fadd_rn(axx, __fmul_rn(n[0], n[0]));
      axy = __fadd_rn(axy, __fmul_rn(n[0], n[1]));
      axz = __fadd_rn(axz, __fmul_rn(n[0], n[2]));
      ayy = __fadd_rn(ayy, __fmul_rn(n[1], n[1]));
      ayz = __fadd_rn(ayz, __fmul_rn(n[1], n[2]));
      azz = __fadd_rn(azz, __fmul_rn(n[2], n[2]));
      const float along = hn_dot3(n, r);
#pragma unroll
      for (int c = 0; c < 3; ++c) b[c] = __fadd_rn(b[c], __fmul_rn(n[c], along));
    }
    const float lambda = __fmul_rn(regularization, kf);
    axx = __fadd_rn(axx, lambda);
    ayy = __fadd_rn(ayy, lambda);
    azz = __fadd_rn(azz, lambda);
    // adjugate of the symmetric A: rows (c00 c01 c02) (c01 c11 c12) (c02 c12 c22)
    const float c00 = hn_diff_of_products(ayy, azz, ayz, ayz), c01 = hn_diff_of_products(axz, ayz, axy, azz),
                c02 = hn_diff_of_products(axy, ayz, axz, ayy), c11 = hn_diff_of_products(axx, azz, axz, axz),
                c12 = hn_diff_of_products(axy, axz, axx, ayz), c22 = hn_diff_of_products(axx, ayy, axy, axy);
    const float row0[3] = {c00, c01, c02}, row1[3] = {c01, c11, c12}, row2[3] = {c02, c12, c22}, a0[3] = {axx, axy, axz};
    const float det = hn_dot3(a0, row0);
    float d[3] = {0.f, 0.f, 0.f};
    if (det > 0.0f && det <= 3.402823466e38f) {
      d[0] = __fdiv_rn(hn_dot3(row0, b), det);
      d[1] = __fdiv_rn(hn_dot3(row1, b), det);
      d[2] = __fdiv_rn(hn_dot3(row2, b), det);
    }
    const int64_t key = cluster_keys[cl];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float idx = (float)((key >> (HN_SIMPLIFY_BITS * c)) & HN_SIMPLIFY_MASK);
      const float lo = __fadd_rn(g.origin[c], __fmul_rn(idx, g.cell[c])), hi = __fadd_rn(lo, g.cell[c]);
      float v = __fadd_rn(mean[c], d[c]);
      v = v < lo ? lo : v;
      v = v > hi ? hi : v;
      x[c] = v;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out_vertices[3 * (size_t)cl + c] = x[c];
  if (normals != nullptr) {
    // sqrtf, not __fsqrt_rn: the latter is the hardware's approximate root here, sqrtf the correctly rounded one
    const float len = sqrtf(hn_dot3(sn, sn));
    const bool ok = len > 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) out_normals[3 * (size_t)cl + c] = ok ? __fdiv_rn(sn[c], len) : 0.0f;
  }
  if (color_kind == 1) {
    const unsigned long long ku = (unsigned long long)k;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ((uint8_t*)out_colors)[3 * (size_t)cl + c] = ku != 0ull ? (uint8_t)((2ull * sci[c] + ku) / (2ull * ku)) : (uint8_t)0;
  }
  if (color_kind == 2) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ((float*)out_colors)[3 * (size_t)cl + c] = __fdiv_rn(scf[c], kf);
  }
}

extern "C" int hn_simplify_reduce(const float* vertices_dev, const float* normals_dev, const void* colors_dev, int color_kind,
                                  const int32_t* order_dev, const int32_t* starts_dev, const int64_t* cluster_keys_dev,
                                  long long n_clusters, long long n_vertices, const float* origin_host,
                                  const float* cell_host, float regularization, int quadric, float* out_vertices_dev,
                                  float* out_normals_dev, void* out_colors_dev, hnStream_t stream) {
  HnCells g;
  if (n_clusters <= 0 || n_vertices <= 0 || n_clusters > n_vertices || n_vertices > 2147483647ll) return -2;
  if (vertices_dev == nullptr || order_dev == nullptr || starts_dev == nullptr || cluster_keys_dev == nullptr ||
      out_vertices_dev == nullptr || !hn_cells(origin_host, cell_host, &g))
    return -2;
  if (color_kind < 0 || color_kind > 2 || (color_kind != 0 && (colors_dev == nullptr || out_colors_dev == nullptr))) return -2;
  if (normals_dev != nullptr && out_normals_dev == nullptr) return -2;
  if (quadric != 0 && (normals_dev == nullptr || !(regularization >= 0.0f) || !(regularization <= 3.402823466e38f))) return -2;
  hipLaunchKernelGGL(hn_simplify_reduce_kernel, dim3((unsigned)((n_clusters + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, vertices_dev, normals_dev, colors_dev, color_kind, order_dev, starts_dev,
                     cluster_keys_dev, n_clusters, n_vertices, g, regularization, quadric, out_vertices_dev,
                     out_normals_dev, out_colors_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_simplify_face_keys: the name of every face: key_ab = a << 31 | b, key_c = c, sign = +1 / -1; a face that degenerates
// (or holds an id outside [0, V), or a cluster id below 0) gets the largest name and the sign 0, so it sorts last.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_simplify_face_keys_kernel(const int32_t* __restrict__ faces, long long n_faces,
                                                                    const int32_t* __restrict__ vertex_cluster,
                                                                    long long n_vertices, int64_t* __restrict__ key_ab,
                                                                    int32_t* __restrict__ key_c, int32_t* __restrict__ sign) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_faces) return;
  const int32_t v0 = faces[3 * i], v1 = faces[3 * i + 1], v2 = faces[3 * i + 2];
  int64_t ab = HN_SIMPLIFY_DROPPED;
  int32_t cc = 2147483647, s = 0;
  if (v0 >= 0 && v1 >= 0 && v2 >= 0 && v0 < n_vertices && v1 < n_vertices && v2 < n_vertices) {
    int32_t a = vertex_cluster[v0], b = vertex_cluster[v1], c = vertex_cluster[v2];
    if (a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c) {
      if (b < a && b < c) {                       // rotations keep the winding
        const int32_t t = a; a = b; b = c; c = t;
      } else if (c < a && c < b) {
        const int32_t t = a; a = c; c = b; b = t;
      }
      s = 1;
      if (b > c) {
        const int32_t t = b; b = c; c = t;
        s = -1;
      }
      ab = (int64_t)a << 31 | (int64_t)b;
      cc = c;
    }
  }
  key_ab[i] = ab;
  key_c[i] = cc;
  sign[i] = s;
}

extern "C" int hn_simplify_face_keys(const int32_t* faces_dev, long long n_faces, const int32_t* vertex_cluster_dev,
                                     long long n_vertices, int64_t* key_ab_dev, int32_t* key_c_dev, int32_t* sign_dev,
                                     hnStream_t stream) {
  if (n_faces <= 0 || n_vertices <= 0 || n_faces > 2147483647ll || n_vertices > 2147483647ll) return -2;
  if (faces_dev == nullptr || vertex_cluster_dev == nullptr || key_ab_dev == nullptr || key_c_dev == nullptr ||
      sign_dev == nullptr)
    return -2;
  hipLaunchKernelGGL(hn_simplify_face_keys_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, faces_dev, n_faces, vertex_cluster_dev, n_vertices, key_ab_dev, key_c_dev,
                     sign_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The sorted names: position i holds face perm[i]; sorted_ab[i] = key_ab[perm[i]] (the caller's sort delivers it), key_c
// and sign are read through perm.  hn_simplify_face_net: net[i] = the sum of the signs of the group that ENDS at i, zero
// everywhere else and for the dropped faces.  hn_simplify_face_emit: ends = the inclusive scan of |net|; the group that
// ends at i writes its |net[i]| copies to the rows ends[i] - |net[i]| .. ends[i] - 1 and marks its three clusters used.
// A perm entry outside [0, F) ends the walk / drops the group; a row outside [0, n_out) is not written.
// ------------------------------------------------------------------------------------------------
HN_DEV bool hn_simplify_same(const int64_t* __restrict__ sorted_ab, const int32_t* __restrict__ key_c,
                             const int64_t* __restrict__ perm, long long n_faces, long long j, int64_t ab, int32_t c) {
  if (sorted_ab[j] != ab) return false;
  const int64_t f = perm[j];
  return f >= 0 && f < n_faces && key_c[f] == c;
}

__global__ __launch_bounds__(256) void hn_simplify_face_net_kernel(const int64_t* __restrict__ sorted_ab,
                                                                   const int32_t* __restrict__ key_c,
                                                                   const int32_t* __restrict__ sign,
                                                                   const int64_t* __restrict__ perm, long long n_faces,
                                                                   int32_t* __restrict__ net) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_faces) return;
  int32_t sum = 0;
  const int64_t ab = sorted_ab[i], f = perm[i];
  if (ab != HN_SIMPLIFY_DROPPED && f >= 0 && f < n_faces) {
    const int32_t c = key_c[f];
    const bool tail = i == n_faces - 1 || !hn_simplify_same(sorted_ab, key_c, perm, n_faces, i + 1, ab, c);
    if (tail) {
      sum = sign[f];
      for (long long j = i - 1; j >= 0 && hn_simplify_same(sorted_ab, key_c, perm, n_faces, j, ab, c); --j) sum += sign[perm[j]];
    }
  }
  net[i] = sum;
}

extern "C" int hn_simplify_face_net(const int64_t* sorted_ab_dev, const int32_t* key_c_dev, const int32_t* sign_dev,
                                    const int64_t* perm_dev, long long n_faces, int32_t* net_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll) return -2;
  if (sorted_ab_dev == nullptr || key_c_dev == nullptr || sign_dev == nullptr || perm_dev == nullptr || net_dev == nullptr)
    return -2;
  hipLaunchKernelGGL(hn_simplify_face_net_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, sorted_ab_dev, key_c_dev, sign_dev, perm_dev, n_faces, net_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

__global__ __launch_bounds__(256) void hn_simplify_face_emit_kernel(const int64_t* __restrict__ sorted_ab,
                                                                    const int32_t* __restrict__ key_c,
                                                                    const int64_t* __restrict__ perm,
                                                                    const int32_t* __restrict__ net,
                                                                    const int64_t* __restrict__ ends, long long n_faces,
                                                                    long long n_clusters, long long n_out,
                                                                    int32_t* __restrict__ faces_out,
                                                                    int32_t* __restrict__ used) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_faces) return;
  const int32_t s = net[i];
  if (s == 0) return;
  const int64_t ab = sorted_ab[i], f = perm[i];
  if (ab == HN_SIMPLIFY_DROPPED || f < 0 || f >= n_faces) return;
  const long long a = ab >> 31, b = ab & 0x7fffffffll, c = key_c[f];
  if (a >= n_clusters || b >= n_clusters || c < 0 || c >= n_clusters) return;
  const long long count = s > 0 ? s : -(long long)s, row0 = ends[i] - count;
  for (long long r = 0; r < count; ++r) {
    const long long row = row0 + r;
    if (row < 0 || row >= n_out) continue;
    faces_out[3 * (size_t)row] = (int32_t)a;
    faces_out[3 * (size_t)row + 1] = (int32_t)(s > 0 ? b : c);
    faces_out[3 * (size_t)row + 2] = (int32_t)(s > 0 ? c : b);
  }
  used[a] = 1;      // whoever gets there stores the same 1
  used[b] = 1;
  used[c] = 1;
}

extern "C" int hn_simplify_face_emit(const int64_t* sorted_ab_dev, const int32_t* key_c_dev, const int64_t* perm_dev,
                                     const int32_t* net_dev, const int64_t* ends_dev, long long n_faces, long long n_clusters,
                                     long long n_out, int32_t* faces_out_dev, int32_t* used_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_clusters <= 0 || n_clusters > 2147483647ll || n_out <= 0 || n_out > n_faces)
    return -2;
  if (sorted_ab_dev == nullptr || key_c_dev == nullptr || perm_dev == nullptr || net_dev == nullptr || ends_dev == nullptr ||
      faces_out_dev == nullptr || used_dev == nullptr)
    return -2;
  hipLaunchKernelGGL(hn_simplify_face_emit_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, sorted_ab_dev, key_c_dev, perm_dev, net_dev, ends_dev, n_faces, n_clusters, n_out,
                     faces_out_dev, used_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_simplify_relabel: out[v] = the output vertex of input vertex v: scan[cluster] - 1 when its cluster is used (scan =
// the inclusive scan of `used`), -1 when the cluster lost all its faces.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_simplify_relabel_kernel(const int32_t* __restrict__ vertex_cluster,
                                                                  long long n_vertices, const int32_t* __restrict__ used,
                                                                  const int32_t* __restrict__ scan, long long n_clusters,
                                                                  int32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_vertices) return;
  const int32_t cl = vertex_cluster[i];
  out[i] = (cl >= 0 && cl < n_clusters && used[cl] != 0) ? scan[cl] - 1 : -1;
}

extern "C" int hn_simplify_relabel(const int32_t* vertex_cluster_dev, long long n_vertices, const int32_t* used_dev,
                                   const int32_t* scan_dev, long long n_clusters, int32_t* out_dev, hnStream_t stream) {
  if (n_vertices <= 0 || n_vertices > 2147483647ll || n_clusters <= 0 || n_clusters > n_vertices) return -2;
  if (vertex_cluster_dev == nullptr || used_dev == nullptr || scan_dev == nullptr || out_dev == nullptr) return -2;
  hipLaunchKernelGGL(hn_simplify_relabel_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, vertex_cluster_dev, n_vertices, used_dev, scan_dev, n_clusters, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
