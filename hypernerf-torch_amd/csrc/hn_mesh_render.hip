// Rendering a triangle mesh to depth, face-id and shaded colour images through the cameras the field is rendered with,
// for gfx950.
//
// Definition (DESIGN.md 3.11 holds it in full; tests/mesh_render_restated.py restates it in NumPy float32, bit for bit):
// the image is defined by RAY CASTING.  Pixel p has the ray (o, d) = row p of the caller's ray tensor; projection only
// bounds which faces a pixel must look at.  Every operation is one fp32 operation rounded on its own (__f*_rn; the library
// is built with contraction off), in the order written:
//   cross(p, q) = (p1*q2 - p2*q1, p2*q0 - p0*q2, p0*q1 - p1*q0),   dot(u, v) = (u0*v0 + u1*v1) + u2*v2
//   face (ia, ib, ic):  A = V[ia] - o, B = V[ib] - o, C = V[ic] - o
//   edge value of P -> Q with ids ip, iq:  dot(d, cross(P, Q)) when ip < iq,  -dot(d, cross(Q, P)) when ip > iq — both
//     faces on an edge evaluate the same expression on the same operands and get exactly opposite values: no pinholes
//   ea, eb, ec = the values of B -> C, C -> A, A -> B;  a face with two equal ids is never hit
//   inside = (all three >= 0 or all three <= 0) and not all three == 0      (two-sided; NaN compares false)
//   n = cross(V[ib] - V[ia], V[ic] - V[ia]),  den = dot(d, n),  num = dot(A, n),  t = num / den
//   hit = inside and den != 0 and 0 < t < +inf;  the smallest t wins, equal t goes to the smaller face id
//   face = the winner or -1,  depth = t or 0,  bary = (ea / s, eb / s, ec / s) with s = (ea + eb) + ec, or zeros
// Nothing depends on scheduling: no atomics, no floating-point reduction; a pixel's thread walks the faces of its tile
// and keeps (t, face) in registers.  The binning (hn_mesh_project, hn_mesh_bin_count, hn_mesh_bin_fill) must only be
// conservative: the picture does not depend on it — but for a near-degenerate sliver face, whose edge values are rounding
// noise for every ray on the extension of its line: the definition can report a hit there, which binning confines to the
// face's own tiles (limits).
#include "hn_camera.h"

#define HN_MESH_BATCH 64           // faces staged through LDS at a time

HN_DEV float hn_mr_dot(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}

HN_DEV void hn_mr_cross(const float* p, const float* q, float* out) {
  out[0] = __fsub_rn(__fmul_rn(p[1], q[2]), __fmul_rn(p[2], q[1]));
  out[1] = __fsub_rn(__fmul_rn(p[2], q[0]), __fmul_rn(p[0], q[2]));
  out[2] = __fsub_rn(__fmul_rn(p[0], q[1]), __fmul_rn(p[1], q[0]));
}

// the value of the directed edge P -> Q in canonical order; ip != iq
HN_DEV float hn_mr_edge(const float* d, const float* P, const float* Q, int32_t ip, int32_t iq) {
  float c[3];
  if (ip < iq) {
    hn_mr_cross(P, Q, c);
    return hn_mr_dot(d, c);
  }
  hn_mr_cross(Q, P, c);
  return -hn_mr_dot(d, c);
}

// hn_mesh_project: the forward camera model (hn_mr_project, hn_camera.h) per vertex.  It feeds the bins only, so its
// rounding is of no consequence to the picture.
__global__ __launch_bounds__(256) void hn_mesh_project_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                              const float* __restrict__ cam, float* __restrict__ pix,
                                                              int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_vertices) return;
  float u, v;
  flags[i] = hn_mr_project(cam, vertices[3 * (size_t)i], vertices[3 * (size_t)i + 1], vertices[3 * (size_t)i + 2], &u, &v);
  pix[2 * (size_t)i] = u;
  pix[2 * (size_t)i + 1] = v;
}

extern "C" int hn_mesh_project(const float* vertices_dev, long long n_vertices, const float* cam_dev, float* pix_dev,
                               int32_t* flags_dev, hnStream_t stream) {
  if (n_vertices <= 0 || n_vertices > 2147483647ll) return -2;
  if (vertices_dev == nullptr || cam_dev == nullptr || pix_dev == nullptr || flags_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_mesh_project_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, cam_dev, pix_dev, flags_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The tile box of a face, shared by hn_mesh_bin_count and hn_mesh_bin_fill: the pixel box of its three projected
// vertices and three projected edge midpoints, padded by 1 pixel (and by 1/8 of its larger side under a camera with
// distortion, whose image of a straight edge bends), clipped to the image.  Any unprojectable point gives the whole
// image, where the ray rejects what is behind; all three vertices behind the camera give nothing.
// Returns false when the face holds an id outside [0, V) (box left empty); an empty box has tx1 < tx0.
// ------------------------------------------------------------------------------------------------
struct HnTileBox {
  int tx0, tx1, ty0, ty1;
};

HN_DEV bool hn_mr_face_box(const int32_t* __restrict__ faces, long long f, const float* __restrict__ vertices,
                           const float* __restrict__ pix, const int32_t* __restrict__ vflags, long long n_vertices,
                           const float* __restrict__ cam, int H, int W, HnTileBox* box) {
  box->tx0 = box->ty0 = 0;
  box->tx1 = box->ty1 = -1;
  const int32_t id[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
  for (int c = 0; c < 3; ++c)
    if (id[c] < 0 || id[c] >= n_vertices) return false;
  const int fl[3] = {vflags[id[0]], vflags[id[1]], vflags[id[2]]};
  if ((fl[0] & fl[1] & fl[2] & HN_MESH_BEHIND) != 0) return true;
  int any = fl[0] | fl[1] | fl[2];
  float ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
  if (any == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int a = id[c], b = id[(c + 1) % 3];
      float u = pix[2 * (size_t)a], v = pix[2 * (size_t)a + 1];
      ulo = fminf(ulo, u); uhi = fmaxf(uhi, u); vlo = fminf(vlo, v); vhi = fmaxf(vhi, v);
      any |= hn_mr_project(cam, 0.5f * (vertices[3 * (size_t)a] + vertices[3 * (size_t)b]),
                           0.5f * (vertices[3 * (size_t)a + 1] + vertices[3 * (size_t)b + 1]),
                           0.5f * (vertices[3 * (size_t)a + 2] + vertices[3 * (size_t)b + 2]), &u, &v);
      ulo = fminf(ulo, u); uhi = fmaxf(uhi, u); vlo = fminf(vlo, v); vhi = fmaxf(vhi, v);
    }
  }
  if (any != 0) {
    box->tx1 = (W - 1) / HN_MESH_TILE;
    box->ty1 = (H - 1) / HN_MESH_TILE;
    return true;
  }
  const bool distorted = cam[17] != 0.0f || cam[18] != 0.0f || cam[19] != 0.0f || cam[20] != 0.0f || cam[21] != 0.0f;
  const float pad = 1.0f + (distorted ? 0.125f * fmaxf(uhi - ulo, vhi - vlo) : 0.0f);
  // clamped in fp32 first (the sides are at most 65535, exact), so that the conversions to int cannot overflow
  const float u0 = fmaxf(ulo - pad, 0.0f), u1 = fminf(uhi + pad, (float)(W - 1));
  const float v0 = fmaxf(vlo - pad, 0.0f), v1 = fminf(vhi + pad, (float)(H - 1));
  if (!(u0 <= u1) || !(v0 <= v1)) return true;      // beside the image (or a NaN pad: inf - inf cannot occur, finite box)
  box->tx0 = (int)floorf(u0) / HN_MESH_TILE;
  box->tx1 = (int)floorf(u1) / HN_MESH_TILE;
  box->ty0 = (int)floorf(v0) / HN_MESH_TILE;
  box->ty1 = (int)floorf(v1) / HN_MESH_TILE;
  return true;
}

__global__ __launch_bounds__(256) void hn_mesh_bin_count_kernel(const int32_t* __restrict__ faces, long long n_faces,
                                                                const float* __restrict__ vertices,
                                                                const float* __restrict__ pix,
                                                                const int32_t* __restrict__ vflags, long long n_vertices,
                                                                const float* __restrict__ cam, int H, int W,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ err) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  HnTileBox b;
  if (!hn_mr_face_box(faces, f, vertices, pix, vflags, n_vertices, cam, H, W, &b)) {
    err[0] = 1;      // whoever gets there stores the same 1
    counts[f] = 0;
    return;
  }
  counts[f] = b.tx1 < b.tx0 || b.ty1 < b.ty0 ? 0 : (b.tx1 - b.tx0 + 1) * (b.ty1 - b.ty0 + 1);
}

__global__ __launch_bounds__(256) void hn_mesh_bin_fill_kernel(const int32_t* __restrict__ faces, long long n_faces,
                                                               const float* __restrict__ vertices,
                                                               const float* __restrict__ pix,
                                                               const int32_t* __restrict__ vflags, long long n_vertices,
                                                               const float* __restrict__ cam, int H, int W,
                                                               const int64_t* __restrict__ ends, long long n_pairs,
                                                               int32_t* __restrict__ pair_tile,
                                                               int32_t* __restrict__ pair_face) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  HnTileBox b;
  if (!hn_mr_face_box(faces, f, vertices, pix, vflags, n_vertices, cam, H, W, &b)) return;
  if (b.tx1 < b.tx0 || b.ty1 < b.ty0) return;
  const int tiles_x = (W + HN_MESH_TILE - 1) / HN_MESH_TILE;
  // the rows of this face end at ends[f] (the inclusive scan of the counts): a row outside [0, n_pairs) is not written
  long long row = ends[f] - (long long)(b.tx1 - b.tx0 + 1) * (b.ty1 - b.ty0 + 1);
  for (int ty = b.ty0; ty <= b.ty1; ++ty)
    for (int tx = b.tx0; tx <= b.tx1; ++tx, ++row) {
      if (row < 0 || row >= n_pairs) continue;
      pair_tile[row] = ty * tiles_x + tx;
      pair_face[row] = (int32_t)f;
    }
}

static bool hn_mesh_image_ok(int H, int W) { return H > 0 && W > 0 && H <= HN_MESH_MAX_SIDE && W <= HN_MESH_MAX_SIDE; }

extern "C" int hn_mesh_bin_count(const int32_t* faces_dev, long long n_faces, const float* vertices_dev, const float* pix_dev,
                                 const int32_t* vflags_dev, long long n_vertices, const float* cam_dev, int H, int W,
                                 int32_t* counts_dev, int32_t* err_dev, hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll || !hn_mesh_image_ok(H, W))
    return -2;
  if (faces_dev == nullptr || vertices_dev == nullptr || pix_dev == nullptr || vflags_dev == nullptr || cam_dev == nullptr ||
      counts_dev == nullptr || err_dev == nullptr)
    return -3;
  hipLaunchKernelGGL(hn_mesh_bin_count_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     faces_dev, n_faces, vertices_dev, pix_dev, vflags_dev, n_vertices, cam_dev, H, W, counts_dev, err_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_mesh_bin_fill(const int32_t* faces_dev, long long n_faces, const float* vertices_dev, const float* pix_dev,
                                const int32_t* vflags_dev, long long n_vertices, const float* cam_dev, int H, int W,
                                const int64_t* ends_dev, long long n_pairs, int32_t* pair_tile_dev, int32_t* pair_face_dev,
                                hnStream_t stream) {
  if (n_faces <= 0 || n_faces > 2147483647ll || n_vertices <= 0 || n_vertices > 2147483647ll || !hn_mesh_image_ok(H, W) ||
      n_pairs <= 0 || n_pairs > 2147483647ll)
    return -2;
  if (faces_dev == nullptr || vertices_dev == nullptr || pix_dev == nullptr || vflags_dev == nullptr || cam_dev == nullptr ||
      ends_dev == nullptr || pair_tile_dev == nullptr || pair_face_dev == nullptr)
    return -3;
  hipLaunchKernelGGL(hn_mesh_bin_fill_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     faces_dev, n_faces, vertices_dev, pix_dev, vflags_dev, n_vertices, cam_dev, H, W, ends_dev, n_pairs,
                     pair_tile_dev, pair_face_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_mesh_trace: one workgroup per tile, one thread per pixel.  The faces of tile T are pair_face[tile_begin[T] ..
// tile_end[T]) (the pairs grouped by tile; with every tile given [0, F) and pair_face = 0 .. F - 1 it is the brute-force
// caster).  64 faces at a time go through LDS — nine floats and three ids each, read by every thread at the same address
// (a broadcast) — and every thread tests each of them by the definition at the top of this file.  A pair entry or a
// vertex id out of range stages a face that is never hit.  Threads of an edge tile outside the image only keep the
// barriers.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_mesh_trace_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                            const int32_t* __restrict__ faces, long long n_faces,
                                                            const float* __restrict__ rays, int ray_ld, int H, int W,
                                                            const int64_t* __restrict__ tile_begin,
                                                            const int64_t* __restrict__ tile_end,
                                                            const int32_t* __restrict__ pair_face, long long n_pairs,
                                                            int32_t* __restrict__ face_out, float* __restrict__ depth_out,
                                                            float* __restrict__ bary_out) {
  __shared__ float s_v[HN_MESH_BATCH][9];
  __shared__ int32_t s_id[HN_MESH_BATCH][3];
  __shared__ int32_t s_face[HN_MESH_BATCH];
  const int tiles_x = (W + HN_MESH_TILE - 1) / HN_MESH_TILE;
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int i = tx * HN_MESH_TILE + (threadIdx.x & (HN_MESH_TILE - 1)), j = ty * HN_MESH_TILE + (threadIdx.x / HN_MESH_TILE);
  const bool live = i < W && j < H;
  const size_t p = live ? (size_t)j * W + i : 0;
  float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
  if (live) {
    const float* r = rays + p * (size_t)ray_ld;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; d[0] = r[3]; d[1] = r[4]; d[2] = r[5];
  }
  long long first = tile_begin[tile], last = tile_end[tile];      // uniform over the workgroup
  if (first < 0) first = 0;
  if (last > n_pairs) last = n_pairs;
  float best_t = INFINITY, best_e[3] = {0.f, 0.f, 0.f};
  int32_t best_f = -1;
  for (long long base = first; base < last; base += HN_MESH_BATCH) {
    const int n = (int)(last - base < HN_MESH_BATCH ? last - base : HN_MESH_BATCH);
    __syncthreads();      // the previous batch has been read by everyone
    if ((int)threadIdx.x < n) {
      const int k = threadIdx.x;
      const int32_t f = pair_face[base + k];
      int32_t id[3] = {0, 0, 0};      // equal ids: never hit
      bool ok = f >= 0 && f < n_faces;
      if (ok) {
        for (int c = 0; c < 3; ++c) id[c] = faces[3 * (size_t)f + c];
        ok = id[0] >= 0 && id[1] >= 0 && id[2] >= 0 && id[0] < n_vertices && id[1] < n_vertices && id[2] < n_vertices;
      }
      for (int c = 0; c < 3; ++c) {
        s_id[k][c] = ok ? id[c] : 0;
        for (int a = 0; a < 3; ++a) s_v[k][3 * c + a] = ok ? vertices[3 * (size_t)id[c] + a] : 0.0f;
      }
      s_face[k] = ok ? f : -1;
    }
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < n; ++k) {
      const int32_t ia = s_id[k][0], ib = s_id[k][1], ic = s_id[k][2];
      if (ia == ib || ib == ic || ia == ic) continue;
      const float* va = s_v[k];
      const float* vb = s_v[k] + 3;
      const float* vc = s_v[k] + 6;
      float A[3], B[3], Cc[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        A[c] = __fsub_rn(va[c], o[c]);
        B[c] = __fsub_rn(vb[c], o[c]);
        Cc[c] = __fsub_rn(vc[c], o[c]);
      }
      const float ea = hn_mr_edge(d, B, Cc, ib, ic), eb = hn_mr_edge(d, Cc, A, ic, ia), ec = hn_mr_edge(d, A, B, ia, ib);
      const bool inside = ((ea >= 0.0f && eb >= 0.0f && ec >= 0.0f) || (ea <= 0.0f && eb <= 0.0f && ec <= 0.0f)) &&
                          !(ea == 0.0f && eb == 0.0f && ec == 0.0f);
      if (!inside) continue;
      float e1[3], e2[3], nrm[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        e1[c] = __fsub_rn(vb[c], va[c]);
        e2[c] = __fsub_rn(vc[c], va[c]);
      }
      hn_mr_cross(e1, e2, nrm);
      const float den = hn_mr_dot(d, nrm), num = hn_mr_dot(A, nrm);
      const float t = __fdiv_rn(num, den);
      if (!(den != 0.0f) || !(t > 0.0f) || !(t < INFINITY)) continue;
      const int32_t f = s_face[k];
      if (t < best_t || (t == best_t && f < best_f)) {
        best_t = t;
        best_f = f;
        best_e[0] = ea; best_e[1] = eb; best_e[2] = ec;
      }
    }
  }
  if (!live) return;
  face_out[p] = best_f;
  if (best_f >= 0) {
    const float s = __fadd_rn(__fadd_rn(best_e[0], best_e[1]), best_e[2]);
    depth_out[p] = best_t;
#pragma unroll
    for (int c = 0; c < 3; ++c) bary_out[3 * p + c] = __fdiv_rn(best_e[c], s);
  } else {
    depth_out[p] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) bary_out[3 * p + c] = 0.0f;
  }
}

extern "C" int hn_mesh_trace(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                             const float* rays_dev, int ray_ld, int H, int W, const int64_t* tile_begin_dev,
                             const int64_t* tile_end_dev, const int32_t* pair_face_dev, long long n_pairs,
                             int32_t* face_out_dev, float* depth_out_dev, float* bary_out_dev, hnStream_t stream) {
  if (n_vertices < 0 || n_vertices > 2147483647ll || n_faces < 0 || n_faces > 2147483647ll || n_pairs < 0 ||
      n_pairs > 2147483647ll || ray_ld < 6 || !hn_mesh_image_ok(H, W) || (long long)H * W > 2147483647ll)
    return -2;
  if (rays_dev == nullptr || tile_begin_dev == nullptr || tile_end_dev == nullptr || face_out_dev == nullptr ||
      depth_out_dev == nullptr || bary_out_dev == nullptr)
    return -3;
  if (n_pairs > 0 && (pair_face_dev == nullptr || faces_dev == nullptr || vertices_dev == nullptr || n_faces == 0 ||
                      n_vertices == 0))
    return -3;
  const int tiles = ((W + HN_MESH_TILE - 1) / HN_MESH_TILE) * ((H + HN_MESH_TILE - 1) / HN_MESH_TILE);
  hipLaunchKernelGGL(hn_mesh_trace_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, vertices_dev, n_vertices,
                     faces_dev, n_faces, rays_dev, ray_ld, H, W, tile_begin_dev, tile_end_dev, pair_face_dev, n_pairs,
                     face_out_dev, depth_out_dev, bary_out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_mesh_shade: one thread per pixel, from `face` and `bary` (w) to normal, rgb (fp32) and rgb8:
//   N = (wa*Na + wb*Nb) + wc*Nc from the vertex normals, or the face's n without them, divided by its length
//       sqrt(dot(N, N)) — the zero vector when the length is not > 0
//   c = (wa*ca + wb*cb) + wc*cc from the vertex colours (uint8 / 255, or fp32 as they are), or base_color without them
//   k = ambient + (1 - ambient) * |dot(N, d)| (headlight != 0), or 1
//   rgb = min(max(c * k, 0), 1) with max(x, 0) = x > 0 ? x : 0 (a NaN gives 0),  rgb8 = floor(255 * rgb + 0.5)
// A pixel whose face lies outside [0, F) — none — gets normal 0 and the background.
// ------------------------------------------------------------------------------------------------
struct HnShade {
  float ambient, base[3], background[3];
  int headlight, color_kind;
};

__global__ __launch_bounds__(256) void hn_mesh_shade_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                            const int32_t* __restrict__ faces, long long n_faces,
                                                            const float* __restrict__ normals,
                                                            const void* __restrict__ colors, const float* __restrict__ rays,
                                                            int ray_ld, long long n_pixels,
                                                            const int32_t* __restrict__ face, const float* __restrict__ bary,
                                                            HnShade s, float* __restrict__ normal_out,
                                                            float* __restrict__ rgb_out, uint8_t* __restrict__ rgb8_out) {
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
        N[c] = __fadd_rn(__fadd_rn(__fmul_rn(w[0], normals[3 * (size_t)id[0] + c]), __fmul_rn(w[1], normals[3 * (size_t)id[1] + c])),
                         __fmul_rn(w[2], normals[3 * (size_t)id[2] + c]));
    } else {
      float e1[3], e2[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        e1[c] = __fsub_rn(vertices[3 * (size_t)id[1] + c], vertices[3 * (size_t)id[0] + c]);
        e2[c] = __fsub_rn(vertices[3 * (size_t)id[2] + c], vertices[3 * (size_t)id[0] + c]);
      }
      hn_mr_cross(e1, e2, N);
    }
    // sqrtf, not __fsqrt_rn: the correctly rounded root (see hn_simplify.hip)
    const float len = sqrtf(hn_mr_dot(N, N));
    const bool ok = len > 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) N[c] = ok ? __fdiv_rn(N[c], len) : 0.0f;
    float k = 1.0f;
    if (s.headlight != 0) {
      const float* r = rays + (size_t)p * ray_ld;
      const float d[3] = {r[3], r[4], r[5]};
      k = __fadd_rn(s.ambient, __fmul_rn(__fsub_rn(1.0f, s.ambient), fabsf(hn_mr_dot(N, d))));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float col = s.base[c];
      if (s.color_kind == 1) {
        const uint8_t* u = (const uint8_t*)colors;
        col = __fadd_rn(__fadd_rn(__fmul_rn(w[0], __fdiv_rn((float)u[3 * (size_t)id[0] + c], 255.0f)),
                                  __fmul_rn(w[1], __fdiv_rn((float)u[3 * (size_t)id[1] + c], 255.0f))),
                        __fmul_rn(w[2], __fdiv_rn((float)u[3 * (size_t)id[2] + c], 255.0f)));
      } else if (s.color_kind == 2) {
        const float* u = (const float*)colors;
        col = __fadd_rn(__fadd_rn(__fmul_rn(w[0], u[3 * (size_t)id[0] + c]), __fmul_rn(w[1], u[3 * (size_t)id[1] + c])),
                        __fmul_rn(w[2], u[3 * (size_t)id[2] + c]));
      }
      const float x = __fmul_rn(col, k);
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

extern "C" int hn_mesh_shade(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                             const float* normals_dev, const void* colors_dev, int color_kind, const float* rays_dev,
                             int ray_ld, long long n_pixels, const int32_t* face_dev, const float* bary_dev, int headlight,
                             float ambient, const float* base_color_host, const float* background_host,
                             float* normal_out_dev, float* rgb_out_dev, uint8_t* rgb8_out_dev, hnStream_t stream) {
  if (n_vertices < 0 || n_vertices > 2147483647ll || n_faces < 0 || n_faces > 2147483647ll || n_pixels <= 0 ||
      n_pixels > 2147483647ll || ray_ld < 6 || color_kind < 0 || color_kind > 2 || !(ambient >= 0.0f && ambient <= 1.0f))
    return -2;
  if (rays_dev == nullptr || face_dev == nullptr || bary_dev == nullptr || base_color_host == nullptr ||
      background_host == nullptr || normal_out_dev == nullptr || rgb_out_dev == nullptr || rgb8_out_dev == nullptr)
    return -3;
  if (n_faces > 0 && (faces_dev == nullptr || vertices_dev == nullptr || n_vertices == 0)) return -3;
  if (color_kind != 0 && colors_dev == nullptr && n_faces > 0) return -3;
  HnShade s;
  s.ambient = ambient;
  s.headlight = headlight;
  s.color_kind = color_kind;
  for (int c = 0; c < 3; ++c) {
    const float b = base_color_host[c], g = background_host[c];
    if (!(b >= 0.0f && b <= 1.0f) || !(g >= 0.0f && g <= 1.0f)) return -2;
    s.base[c] = b;
    s.background[c] = g;
  }
  hipLaunchKernelGGL(hn_mesh_shade_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices_dev, n_vertices, faces_dev, n_faces, normals_dev, colors_dev, rays_dev, ray_ld, n_pixels,
                     face_dev, bary_dev, s, normal_out_dev, rgb_out_dev, rgb8_out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
