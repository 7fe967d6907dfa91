// A texture atlas for a triangle mesh, for gfx950: one chart per face laid out without a host loop, the atlas texels
// rasterised into 3-D, and the sampler that puts the texture back on the rendered mesh.
//
// Definition (DESIGN.md 3.16 holds it in full; tests/texture_restated.py restates it in NumPy float32, face by face).
// Every fp32 operation is rounded on its own (__f*_rn; the library is built with contraction off), in the order written;
// dot(u, v) = (u0*v0 + u1*v1) + u2*v2, cross as in hn_mesh_render.hip.
//   class      of face (ia, ib, ic): m = the largest of the three squared edge lengths dot(e, e), e = V[q] - V[p], folded
//              from 0 by "x > m ? x : m" (a NaN never wins).  side s = the smallest power of two in [min_cell, max_cell]
//              with m <= (L*texel)*(L*texel), L = s - 7; max_cell when there is none.  A face with an id outside [0, V) is
//              given min_cell and stores 1 into err[0].  class = log2(s); key = (10 - class) << 32 | face id.
//   cells      the faces in ascending key order; the faces of one side at ranks r0 .. r1: cell j of that side holds rank
//              r0 + 2j in its lower half and r0 + 2j + 1 (if < r1) in its upper half.  Cells are numbered in that order;
//              cell c of side s has the Morton index M = (sum over the cells before it of (their side / min_cell)^2), its
//              origin is (x, y) * min_cell with x from the even bits of M and y from the odd bits.
//   chart      texel (i, j) has its centre at (i + 0.5, j + 0.5).  Relative to the cell origin the lower half's corners 0, 1, 2
//              sit at (1.5, 1.5), (1.5 + L, 1.5), (1.5, 1.5 + L); the upper half is the point mirror (x, y) -> (s - x, s - y).
//              The lower half owns the texels with i + j <= s - 2, the upper half those with i + j >= s, nobody i + j = s - 1.
//   texel      of face f: (x, y) its centre relative to the origin (mirrored first in the upper half),
//              b1 = (x - 1.5) / L, b2 = (y - 1.5) / L, b0 = (1 - b1) - b2;  position = (b0*v0 + b1*v1) + b2*v2 per coordinate,
//              not clamped: texels outside the triangle extrapolate, so bilinear sampling of an affine function is exact.
//              normal = N / sqrt(dot(N, N)) of N = (b0*n0 + b1*n1) + b2*n2 when there are vertex normals and the length
//              is > 0, else of N = cross(v1 - v0, v2 - v0), else zero.
//   sample     of pixel p with face f and weights w: u = (w0*uv[f][0].x + w1*uv[f][1].x) + w2*uv[f][2].x, clamped into
//              [min, max] of the three (u > lo ? u : lo, then < hi ? : hi; a NaN gives lo), v alike.
//              bilinear: a = u - 0.5, i0 = floor(a), fx = a - i0 (both exact), i1 = i0 + 1, j alike;
//              top = c(i0, j0) + fx*(c(i1, j0) - c(i0, j0)), bot alike on j1, colour = top + fy*(bot - top) —
//              a constant texture comes back unchanged.  nearest: c(floor(u), floor(v)).  c = texel / 255 (uint8) or as it
//              is (fp32); indices are clamped into the texture.  Normal, headlight factor, clamp, rgb8 and background are
//              hn_mesh_shade's, operation for operation.
// Nothing depends on scheduling: no atomics, no reductions.
#include "hn_common.h"

#define HN_TEX_MIN_SIDE 16          // the smallest cell: L = 9 texels
#define HN_TEX_MAX_SIDE 1024        // the largest cell
#define HN_TEX_MAX_ATLAS 16384      // atlas sides: texel coordinates + 0.5 stay exact in fp32
#define HN_TEX_CLASSES 7            // sides 1024 >> q, q = 0 .. 6
#define HN_TEX_GUTTER 7             // s - L

HN_DEV float hn_tx_dot(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

HN_DEV void hn_tx_cross(const float* p, const float* q, float* out) {
  out[0] = __fsub_rn(__fmul_rn(p[1], q[2]), __fmul_rn(p[2], q[1]));
  out[1] = __fsub_rn(__fmul_rn(p[2], q[0]), __fmul_rn(p[0], q[2]));
  out[2] = __fsub_rn(__fmul_rn(p[0], q[1]), __fmul_rn(p[1], q[0]));
}

HN_DEV float hn_tx_mix(const float* w, float a, float b, float c) {
  return __fadd_rn(__fadd_rn(__fmul_rn(w[0], a), __fmul_rn(w[1], b)), __fmul_rn(w[2], c));
}

// N / |N|, or false (N untouched) when the length is not > 0
HN_DEV bool hn_tx_normalize(float* N) {
  // sqrtf, not __fsqrt_rn: the correctly rounded root (see hn_simplify.hip)
  const float len = sqrtf(hn_tx_dot(N, N));
  if (!(len > 0.0f)) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c) N[c] = __fdiv_rn(N[c], len);
  return true;
}

static bool hn_tex_pow2(int s) { return s >= HN_TEX_MIN_SIDE && s <= HN_TEX_MAX_SIDE && (s & (s - 1)) == 0; }

static int hn_tex_log2(int s) {
  int k = 0;
  while ((1 << k) < s) ++k;
  return k;
}

// ------------------------------------------------------------------------------------------------
// hn_tex_classify: one thread per face
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_tex_classify_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                              const int32_t* __restrict__ faces, long long n_faces,
                                                              float texel, int log_min, int log_max,
                                                              int32_t* __restrict__ cls_out, int64_t* __restrict__ keys,
                                                              int32_t* __restrict__ err) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  const int32_t id[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
  int cls = log_min;
  if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] >= n_vertices || id[1] >= n_vertices || id[2] >= n_vertices) {
    err[0] = 1;      // whoever gets there stores the same 1
  } else {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int32_t p = id[c], q = id[(c + 1) % 3];
      float e[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) e[a] = __fsub_rn(vertices[3 * (size_t)q + a], vertices[3 * (size_t)p + a]);
      const float x = hn_tx_dot(e, e);
      m = x > m ? x : m;
    }
    cls = log_max;
    for (int k = log_min; k < log_max; ++k) {
      const float reach = __fmul_rn((float)((1 << k) - HN_TEX_GUTTER), texel);
      if (m <= __fmul_rn(reach, reach)) {
        cls = k;
        break;
      }
    }
  }
  cls_out[f] = cls;
  keys[f] = ((int64_t)(10 - cls) << 32) | (int64_t)f;
}

extern "C" int hn_tex_classify(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                               float texel, int min_cell, int max_cell, int32_t* class_dev, int64_t* keys_dev,
                               int32_t* err_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll || !hn_tex_pow2(min_cell) ||
      !hn_tex_pow2(max_cell) || min_cell > max_cell || !(texel > 0.0f) || !(texel <= 3.0e38f))
    return -2;
  if (vertices_dev == nullptr || faces_dev == nullptr || class_dev == nullptr || keys_dev == nullptr || err_dev == nullptr)
    return -3;
  hipLaunchKernelGGL(hn_tex_classify_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, faces_dev, n_faces, texel, hn_tex_log2(min_cell), hn_tex_log2(max_cell),
                     class_dev, keys_dev, err_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The cells of an atlas by side: sides 1024 >> q, q = 0 .. 6.  Cells cell0[q] .. cell0[q + 1] have that side, the first of
// them the Morton index morton0[q] (in units of min_cell x min_cell), each (side / min_cell)^2 further; their faces are the
// sorted ranks rank0[q] .. rank0[q + 1], two per cell.
// ------------------------------------------------------------------------------------------------
struct HnTexClasses {
  long long rank0[HN_TEX_CLASSES + 1], cell0[HN_TEX_CLASSES + 1], morton0[HN_TEX_CLASSES + 1];
  int log_unit;      // log2(min_cell)
};

// from the 8 ascending first ranks (faces; by_cells = false) or first cells (by_cells = true) of the sides; false when
// they are not ascending from 0, a side below min_cell is used, or the atlas would exceed 16384 x 16384
static bool hn_tex_classes(const int64_t* first_host, bool by_cells, int min_cell, HnTexClasses* t) {
  t->log_unit = hn_tex_log2(min_cell);
  if (first_host[0] != 0) return false;
  long long cells = 0, morton = 0;
  for (int q = 0; q <= HN_TEX_CLASSES; ++q) {
    t->cell0[q] = cells;
    t->morton0[q] = morton;
    t->rank0[q] = by_cells ? 0 : first_host[q];
    if (q == HN_TEX_CLASSES) break;
    const long long n = first_host[q + 1] - first_host[q];
    if (n < 0 || n > 2147483647ll) return false;
    const long long n_cells = by_cells ? n : (n + 1) / 2;
    const int side = HN_TEX_MAX_SIDE >> q;
    if (n_cells > 0 && side < min_cell) return false;
    const long long per_side = side >= min_cell ? side / min_cell : 1;
    cells += n_cells;
    morton += n_cells * per_side * per_side;
    if (morton > (long long)(HN_TEX_MAX_ATLAS / min_cell) * (HN_TEX_MAX_ATLAS / min_cell)) return false;
  }
  return true;
}

HN_DEV int hn_tx_class_of_cell(const HnTexClasses& t, long long c) {
  int q = 0;
#pragma unroll
  for (int k = 1; k < HN_TEX_CLASSES; ++k) q += c >= t.cell0[k] ? 1 : 0;
  return q;
}

// the even bits of m, packed
HN_DEV uint32_t hn_tx_even_bits(uint32_t m) {
  m &= 0x55555555u;
  m = (m | (m >> 1)) & 0x33333333u;
  m = (m | (m >> 2)) & 0x0f0f0f0fu;
  m = (m | (m >> 4)) & 0x00ff00ffu;
  m = (m | (m >> 8)) & 0x0000ffffu;
  return m;
}

// x on the even bits
HN_DEV uint32_t hn_tx_spread_bits(uint32_t x) {
  x &= 0x0000ffffu;
  x = (x | (x << 8)) & 0x00ff00ffu;
  x = (x | (x << 4)) & 0x0f0f0f0fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

// ------------------------------------------------------------------------------------------------
// hn_tex_layout: one thread per cell
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_tex_layout_kernel(const int64_t* __restrict__ keys, long long n_faces, HnTexClasses t,
                                                            long long n_cells, int32_t* __restrict__ cell_start,
                                                            int32_t* __restrict__ cell_side, int32_t* __restrict__ cell_face,
                                                            float* __restrict__ uv) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cells) return;
  const int q = hn_tx_class_of_cell(t, c);
  const int s = HN_TEX_MAX_SIDE >> q, per_side = s >> t.log_unit;
  const long long j = c - t.cell0[q];
  const uint32_t m = (uint32_t)(t.morton0[q] + j * per_side * per_side);
  const int ox = (int)(hn_tx_even_bits(m) << t.log_unit), oy = (int)(hn_tx_even_bits(m >> 1) << t.log_unit);
  cell_start[2 * (size_t)c] = ox;
  cell_start[2 * (size_t)c + 1] = oy;
  cell_side[c] = s;
  const float L = (float)(s - HN_TEX_GUTTER);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const long long r = t.rank0[q] + 2 * j + half;
    int32_t f = -1;
    if (r < t.rank0[q + 1] && r < n_faces) {
      const int64_t key = keys[r];
      f = (int32_t)(key & 0xffffffffll);
      if (f < 0 || f >= n_faces) f = -1;
    }
    cell_face[2 * (size_t)c + half] = f;
    if (f < 0) continue;
    // corner 0, then along x, then along y; the upper half mirrored through the cell's centre
    const float x0 = half == 0 ? (float)ox + 1.5f : (float)(ox + s) - 1.5f, y0 = half == 0 ? (float)oy + 1.5f : (float)(oy + s) - 1.5f;
    const float d = half == 0 ? L : -L;
    float* o = uv + 6 * (size_t)f;
    o[0] = x0;     o[1] = y0;
    o[2] = x0 + d; o[3] = y0;
    o[4] = x0;     o[5] = y0 + d;
  }
}

extern "C" int hn_tex_layout(const int64_t* sorted_keys_dev, long long n_faces, const int64_t* class_rank_host, int min_cell,
                             long long n_cells, int32_t* cell_start_dev, int32_t* cell_side_dev, int32_t* cell_face_dev,
                             float* uv_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || !hn_tex_pow2(min_cell) || class_rank_host == nullptr) return -2;
  HnTexClasses t;
  if (!hn_tex_classes(class_rank_host, false, min_cell, &t) || class_rank_host[HN_TEX_CLASSES] != n_faces ||
      t.cell0[HN_TEX_CLASSES] != n_cells)
    return -2;
  if (sorted_keys_dev == nullptr || cell_start_dev == nullptr || cell_side_dev == nullptr || cell_face_dev == nullptr ||
      uv_dev == nullptr)
    return -3;
  hipLaunchKernelGGL(hn_tex_layout_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     sorted_keys_dev, n_faces, t, n_cells, cell_start_dev, cell_side_dev, cell_face_dev, uv_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_tex_rasterize: one thread per atlas texel, consecutive threads along a row.  The texel's Morton index names its
// cell: the side whose index range holds it, then a division.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_tex_rasterize_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                               const int32_t* __restrict__ faces, long long n_faces,
                                                               const float* __restrict__ normals,
                                                               const int32_t* __restrict__ cell_face, HnTexClasses t, int H,
                                                               int W, int32_t* __restrict__ owner,
                                                               float* __restrict__ position, float* __restrict__ normal) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)H * W) return;
  const int j = (int)(p / W), i = (int)(p - (long long)j * W);
  const long long m = (long long)(hn_tx_spread_bits((uint32_t)(i >> t.log_unit)) | (hn_tx_spread_bits((uint32_t)(j >> t.log_unit)) << 1));
  int32_t f = -1;
  int half = 0, s = 0;
  if (m < t.morton0[HN_TEX_CLASSES]) {
    int q = 0;
#pragma unroll
    for (int k = 1; k < HN_TEX_CLASSES; ++k) q += m >= t.morton0[k] ? 1 : 0;
    s = HN_TEX_MAX_SIDE >> q;
    const int per_side = s >> t.log_unit;
    const long long c = t.cell0[q] + (m - t.morton0[q]) / ((long long)per_side * per_side);
    const int sum = (i & (s - 1)) + (j & (s - 1));      // cells are aligned to their side
    half = sum >= s ? 1 : 0;
    if (sum != s - 1 && c < t.cell0[HN_TEX_CLASSES]) f = cell_face[2 * (size_t)c + half];
  }
  int32_t id[3] = {0, 0, 0};
  if (f >= n_faces) f = -1;
  if (f >= 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) id[c] = faces[3 * (size_t)f + c];
    if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] >= n_vertices || id[1] >= n_vertices || id[2] >= n_vertices) f = -1;
  }
  float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f};
  if (f >= 0) {
    float x = (float)(i & (s - 1)) + 0.5f, y = (float)(j & (s - 1)) + 0.5f;
    if (half) {
      x = (float)s - x;
      y = (float)s - y;
    }
    const float L = (float)(s - HN_TEX_GUTTER);
    float b[3];
    b[1] = __fdiv_rn(__fsub_rn(x, 1.5f), L);
    b[2] = __fdiv_rn(__fsub_rn(y, 1.5f), L);
    b[0] = __fsub_rn(__fsub_rn(1.0f, b[1]), b[2]);
    float v[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = vertices[3 * (size_t)id[k] + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) P[c] = hn_tx_mix(b, v[0][c], v[1][c], v[2][c]);
    bool ok = false;
    if (normals != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        N[c] = hn_tx_mix(b, normals[3 * (size_t)id[0] + c], normals[3 * (size_t)id[1] + c], normals[3 * (size_t)id[2] + c]);
      ok = hn_tx_normalize(N);
    }
    if (!ok) {
      float e1[3], e2[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        e1[c] = __fsub_rn(v[1][c], v[0][c]);
        e2[c] = __fsub_rn(v[2][c], v[0][c]);
      }
      hn_tx_cross(e1, e2, N);
      if (!hn_tx_normalize(N)) N[0] = N[1] = N[2] = 0.0f;
    }
  }
  owner[p] = f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    position[3 * (size_t)p + c] = P[c];
    normal[3 * (size_t)p + c] = N[c];
  }
}

static bool hn_tex_atlas_ok(int H, int W, int unit) {
  return H > 0 && W > 0 && H <= HN_TEX_MAX_ATLAS && W <= HN_TEX_MAX_ATLAS && H % unit == 0 && W % unit == 0;
}

extern "C" int hn_tex_rasterize(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                                const float* normals_dev, const int32_t* cell_face_dev, long long n_cells,
                                const int64_t* class_cells_host, int min_cell, int H, int W, int32_t* owner_dev,
                                float* position_dev, float* normal_dev, hnStream_t stream) {
  if (n_vertices < 0 || n_vertices > 2147483647ll || n_faces < 0 || n_faces > 2147483647ll || n_cells < 0 ||
      n_cells > 2147483647ll || !hn_tex_pow2(min_cell) || !hn_tex_atlas_ok(H, W, min_cell) || class_cells_host == nullptr)
    return -2;
  HnTexClasses t;
  if (!hn_tex_classes(class_cells_host, true, min_cell, &t) || t.cell0[HN_TEX_CLASSES] != n_cells) return -2;
  if (owner_dev == nullptr || position_dev == nullptr || normal_dev == nullptr) return -3;
  if (n_cells > 0 && (cell_face_dev == nullptr || faces_dev == nullptr || vertices_dev == nullptr || n_faces == 0 ||
                      n_vertices == 0))
    return -3;
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(hn_tex_rasterize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, faces_dev, n_faces, normals_dev, cell_face_dev, t, H, W, owner_dev,
                     position_dev, normal_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_tex_shade: one thread per pixel, hn_mesh_shade with the colour fetched from the atlas
// ------------------------------------------------------------------------------------------------
struct HnTexShade {
  float ambient, background[3];
  int headlight, kind, bilinear, H, W;
};

HN_DEV float hn_tx_texel(const void* __restrict__ tex, int kind, int W, int i, int j, int c) {
  const size_t at = 3 * ((size_t)j * W + i) + c;
  return kind == 1 ? __fdiv_rn((float)((const uint8_t*)tex)[at], 255.0f) : ((const float*)tex)[at];
}

HN_DEV int hn_tx_clampi(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

__global__ __launch_bounds__(256) void hn_tex_shade_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                           const int32_t* __restrict__ faces, long long n_faces,
                                                           const float* __restrict__ normals, const float* __restrict__ uv,
                                                           const void* __restrict__ tex, const float* __restrict__ rays,
                                                           int ray_ld, long long n_pixels, const int32_t* __restrict__ face,
                                                           const float* __restrict__ bary, HnTexShade s,
                                                           float* __restrict__ normal_out, float* __restrict__ rgb_out,
                                                           uint8_t* __restrict__ rgb8_out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  const int32_t f = face[p];
  float N[3] = {0.f, 0.f, 0.f}, rgb[3] = {s.background[0], s.background[1], s.background[2]};
  int32_t id[3] = {-1, -1, -1};
  bool hit = f >= 0 && f < n_faces;
  if (hit) {
    for (int c = 0; c < 3; ++c) id[c] = faces[3 * (size_t)f + c];
    hit = id[0] >= 0 && id[1] >= 0 && id[2] >= 0 && id[0] < n_vertices && id[1] < n_vertices && id[2] < n_vertices;
  }
  if (hit) {
    const float w[3] = {bary[3 * (size_t)p], bary[3 * (size_t)p + 1], bary[3 * (size_t)p + 2]};
    if (normals != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        N[c] = hn_tx_mix(w, normals[3 * (size_t)id[0] + c], normals[3 * (size_t)id[1] + c], normals[3 * (size_t)id[2] + c]);
    } else {
      float e1[3], e2[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        e1[c] = __fsub_rn(vertices[3 * (size_t)id[1] + c], vertices[3 * (size_t)id[0] + c]);
        e2[c] = __fsub_rn(vertices[3 * (size_t)id[2] + c], vertices[3 * (size_t)id[0] + c]);
      }
      hn_tx_cross(e1, e2, N);
    }
    if (!hn_tx_normalize(N)) N[0] = N[1] = N[2] = 0.0f;
    float k = 1.0f;
    if (s.headlight != 0) {
      const float* r = rays + (size_t)p * ray_ld;
      const float d[3] = {r[3], r[4], r[5]};
      k = __fadd_rn(s.ambient, __fmul_rn(__fsub_rn(1.0f, s.ambient), fabsf(hn_tx_dot(N, d))));
    }
    // (u, v), clamped into the chart's bounding box
    const float* q = uv + 6 * (size_t)f;
    float t[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float lo = fminf(fminf(q[a], q[2 + a]), q[4 + a]), hi = fmaxf(fmaxf(q[a], q[2 + a]), q[4 + a]);
      const float x = hn_tx_mix(w, q[a], q[2 + a], q[4 + a]);
      const float above = x > lo ? x : lo;
      t[a] = above < hi ? above : hi;
    }
    if (s.bilinear) {
      const float ax = __fsub_rn(t[0], 0.5f), ay = __fsub_rn(t[1], 0.5f);
      const float fi = floorf(ax), fj = floorf(ay);
      const float fx = __fsub_rn(ax, fi), fy = __fsub_rn(ay, fj);
      // a uv that is not finite (a foreign uv tensor) must not index outside: clamp in fp32 first
      const int i0r = (int)fminf(fmaxf(fi, -1.0f), (float)s.W), j0r = (int)fminf(fmaxf(fj, -1.0f), (float)s.H);
      const int i0 = hn_tx_clampi(i0r, s.W - 1), i1 = hn_tx_clampi(i0r + 1, s.W - 1);
      const int j0 = hn_tx_clampi(j0r, s.H - 1), j1 = hn_tx_clampi(j0r + 1, s.H - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float c00 = hn_tx_texel(tex, s.kind, s.W, i0, j0, c), c10 = hn_tx_texel(tex, s.kind, s.W, i1, j0, c);
        const float c01 = hn_tx_texel(tex, s.kind, s.W, i0, j1, c), c11 = hn_tx_texel(tex, s.kind, s.W, i1, j1, c);
        const float top = __fadd_rn(c00, __fmul_rn(fx, __fsub_rn(c10, c00)));
        const float bot = __fadd_rn(c01, __fmul_rn(fx, __fsub_rn(c11, c01)));
        rgb[c] = __fadd_rn(top, __fmul_rn(fy, __fsub_rn(bot, top)));
      }
    } else {
      const int i = hn_tx_clampi((int)fminf(fmaxf(floorf(t[0]), -1.0f), (float)s.W), s.W - 1);
      const int j = hn_tx_clampi((int)fminf(fmaxf(floorf(t[1]), -1.0f), (float)s.H), s.H - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = hn_tx_texel(tex, s.kind, s.W, i, j, c);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = __fmul_rn(rgb[c], k);
      const float lo = x > 0.0f ? x : 0.0f;
      rgb[c] = lo < 1.0f ? lo : 1.0f;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    normal_out[3 * (size_t)p + c] = N[c];
    rgb_out[3 * (size_t)p + c] = rgb[c];
    rgb8_out[3 * (size_t)p + c] = (uint8_t)floorf(__fadd_rn(__fmul_rn(255.0f, rgb[c]), 0.5f));
  }
}

extern "C" int hn_tex_shade(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                            const float* normals_dev, const float* uv_dev, const void* texture_dev, int texture_kind,
                            int tex_h, int tex_w, int filter, const float* rays_dev, int ray_ld, long long n_pixels,
                            const int32_t* face_dev, const float* bary_dev, int headlight, float ambient,
                            const float* background_host, float* normal_out_dev, float* rgb_out_dev, uint8_t* rgb8_out_dev,
                            hnStream_t stream) {
  if (n_vertices < 0 || n_vertices > 2147483647ll || n_faces < 0 || n_faces > 2147483647ll || n_pixels <= 0 ||
      n_pixels > 2147483647ll || ray_ld < 6 || (texture_kind != 1 && texture_kind != 2) || (filter != 0 && filter != 1) ||
      tex_h <= 0 || tex_w <= 0 || tex_h > HN_TEX_MAX_ATLAS || tex_w > HN_TEX_MAX_ATLAS || !(ambient >= 0.0f && ambient <= 1.0f))
    return -2;
  if (rays_dev == nullptr || face_dev == nullptr || bary_dev == nullptr || background_host == nullptr ||
      normal_out_dev == nullptr || rgb_out_dev == nullptr || rgb8_out_dev == nullptr)
    return -3;
  if (n_faces > 0 && (faces_dev == nullptr || vertices_dev == nullptr || n_vertices == 0 || uv_dev == nullptr ||
                      texture_dev == nullptr))
    return -3;
  HnTexShade s;
  s.ambient = ambient;
  s.headlight = headlight;
  s.kind = texture_kind;
  s.bilinear = filter;
  s.H = tex_h;
  s.W = tex_w;
  for (int c = 0; c < 3; ++c) {
    const float g = background_host[c];
    if (!(g >= 0.0f && g <= 1.0f)) return -2;
    s.background[c] = g;
  }
  hipLaunchKernelGGL(hn_tex_shade_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, faces_dev, n_faces, normals_dev, uv_dev, texture_dev, rays_dev, ray_ld,
                     n_pixels, face_dev, bary_dev, s, normal_out_dev, rgb_out_dev, rgb8_out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
