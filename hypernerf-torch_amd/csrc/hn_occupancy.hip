// Empty-space skipping for the render path on gfx950: a density lattice becomes one bit per lattice CELL, the bits are
// dilated, and every ray of an image is clipped to the part of [near, far] between the first and the last occupied cell
// it crosses (DESIGN.md 3.18 holds the definition; tests/occupancy_restated.py restates all four kernels in NumPy).
//
// Layout.  The lattice is hn_grid_points' (nx, ny, nz) fp32, z fastest; it has (cx, cy, cz) = (nx-1, ny-1, nz-1) cells,
// cell (i, j, k) between lattice points (i, j, k) and (i+1, j+1, k+1).  Bits are (cx, cy, words) uint64 with
// words = ceil(cz / 64): bit b of word w of row (i, j) is cell (i, j, 64 w + b); the bits past cz are zero.
//
//   hn_occ_mark       a cell is occupied iff one of its 8 corners is >= sigma_min or NaN.  One wave = one word: lane b
//                     decides cell 64 w + b, a 64-bit __ballot is the word.  No atomics.
//   hn_occ_dilate     out = in dilated by the 3 x 3 x 3 cube: one work-item per word ORs the (up to) nine words of the
//                     neighbouring rows, each with its two shifts and the carry bits of the words before and behind it.
//                     Nothing wraps at the faces of the grid and the padding bits stay zero.
//   hn_occ_count      the number of set bits (integer atomics: the sum does not depend on their order).
//   hn_occ_clip_rays  one ray per lane, a 3-D DDA through the cells (below).
//   hn_occ_clip_batch the same DDA for a training batch: each ray against the grid of its own frame, graph-capturable
//                     (tests/occupancy_train_restated.py).
#include "hn_camera.h"

#define HN_OCC_MAX_CELLS 2048      // cells per axis: every (float)index is exact and the walk's bound stays small

struct HnOccGrid {
  int c[3], words;
  float lo[3], cell[3];
};

// host: false when a side has no cell or too many, the bits would not fit the int32 indices of the lattice, hi <= lo or a
// bound is not finite
static inline bool hn_occ_grid(int cx, int cy, int cz, const float* bounds, HnOccGrid* g) {
  if (cx < 1 || cy < 1 || cz < 1 || cx > HN_OCC_MAX_CELLS || cy > HN_OCC_MAX_CELLS || cz > HN_OCC_MAX_CELLS) return false;
  HnLattice lattice;
  if (!hn_lattice(cx + 1, cy + 1, cz + 1, bounds, &lattice)) return false;
  g->c[0] = cx; g->c[1] = cy; g->c[2] = cz;
  g->words = (cz + 63) / 64;
  for (int a = 0; a < 3; ++a) {
    const float lo = bounds != nullptr ? bounds[2 * a] : 0.0f, hi = bounds != nullptr ? bounds[2 * a + 1] : 1.0f;
    if (!(fabsf(lo) <= 3.402823466e38f) || !(fabsf(hi) <= 3.402823466e38f)) return false;
    g->lo[a] = lo;
    g->cell[a] = lattice.step[a];      // (hi - lo) / cells, in fp32
    if (!(g->cell[a] > 0.0f) || !(g->cell[a] <= 3.402823466e38f)) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// hn_occ_mark
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_occ_mark_kernel(const float* __restrict__ f, int ny, int nz, int cx, int cy,
                                                          int cz, int words, float sigma_min,
                                                          unsigned long long* __restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // uniform over the wave
  if (word >= (long long)cx * cy * words) return;
  const int lane = threadIdx.x & 63;
  const int w = (int)(word % words), j = (int)((word / words) % cy), i = (int)(word / ((long long)words * cy));
  const int k = 64 * w + lane;
  bool occupied = false;
  if (k < cz) {
    const size_t p = ((size_t)i * ny + j) * nz + k;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const float v = f[p + ((size_t)(corner >> 2) * ny + ((corner >> 1) & 1)) * nz + (corner & 1)];
      occupied = occupied || !(v < sigma_min);      // >= sigma_min, or NaN
    }
  }
  const unsigned long long m = __ballot(occupied);
  if (lane == 0) bits[word] = m;
}

extern "C" int hn_occ_mark(const float* grid_dev, int nx, int ny, int nz, float sigma_min, uint64_t* bits_dev,
                           hnStream_t stream) {
  HnOccGrid g;
  if (!hn_occ_grid(nx - 1, ny - 1, nz - 1, nullptr, &g)) return -2;
  if (sigma_min != sigma_min) return -2;
  if (grid_dev == nullptr || bits_dev == nullptr) return -3;
  const long long n_words = (long long)g.c[0] * g.c[1] * g.words;
  hipLaunchKernelGGL(hn_occ_mark_kernel, dim3((unsigned)((n_words + 3) / 4)), dim3(256), 0, (hipStream_t)stream, grid_dev,
                     ny, nz, g.c[0], g.c[1], g.c[2], g.words, sigma_min,
                     reinterpret_cast<unsigned long long*>(bits_dev));
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_occ_dilate
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_occ_dilate_kernel(const unsigned long long* __restrict__ in, int cx, int cy,
                                                            int cz, int words, unsigned long long* __restrict__ out) {
  const long long word = (long long)blockIdx.x * 256 + threadIdx.x;
  if (word >= (long long)cx * cy * words) return;
  const int w = (int)(word % words), j = (int)((word / words) % cy), i = (int)(word / ((long long)words * cy));
  unsigned long long m = 0ull;
  for (int di = -1; di <= 1; ++di) {
    if (i + di < 0 || i + di >= cx) continue;
    for (int dj = -1; dj <= 1; ++dj) {
      if (j + dj < 0 || j + dj >= cy) continue;
      const unsigned long long* row = in + ((size_t)(i + di) * cy + (j + dj)) * words;
      const unsigned long long here = row[w];
      m |= here | (here << 1) | (here >> 1);
      if (w > 0) m |= row[w - 1] >> 63;
      if (w + 1 < words) m |= row[w + 1] << 63;
    }
  }
  const int tail = cz - 64 * w;      // cells of this word: the bits past them are padding
  if (tail < 64) m &= (1ull << tail) - 1ull;
  out[word] = m;
}

extern "C" int hn_occ_dilate(const uint64_t* in_dev, uint64_t* out_dev, int cx, int cy, int cz, hnStream_t stream) {
  HnOccGrid g;
  if (!hn_occ_grid(cx, cy, cz, nullptr, &g)) return -2;
  if (in_dev == nullptr || out_dev == nullptr) return -3;
  if (in_dev == out_dev) return -2;      // a word reads its neighbours: not in place
  const long long n_words = (long long)cx * cy * g.words;
  hipLaunchKernelGGL(hn_occ_dilate_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(in_dev), cx, cy, cz, g.words,
                     reinterpret_cast<unsigned long long*>(out_dev));
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_occ_count
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_occ_count_kernel(const unsigned long long* __restrict__ bits, long long n_words,
                                                           unsigned long long* __restrict__ count) {
  const long long word = (long long)blockIdx.x * 256 + threadIdx.x;
  int c = word < n_words ? __popcll(bits[word]) : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(count, (unsigned long long)c);
}

extern "C" int hn_occ_count(const uint64_t* bits_dev, long long n_words, int64_t* count_dev, hnStream_t stream) {
  if (n_words < 1 || n_words > 2147483647ll) return -2;
  if (bits_dev == nullptr || count_dev == nullptr) return -3;
  hipError_t e = hipMemsetAsync(count_dev, 0, sizeof(int64_t), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(hn_occ_count_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(bits_dev), n_words,
                     reinterpret_cast<unsigned long long*>(count_dev));
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_occ_clip_rays.  Every operation is one fp32 operation rounded on its own, in the order written.  Plane i of axis a
// lies at x(a, i) = lo[a] + (float)i * cell[a]; a ray (o, d) meets it at T(a, i) = (x(a, i) - o[a]) / d[a] — always from the
// index, never by accumulating a step, so every T carries the error of one subtraction and one division whatever the
// size of the grid.
//   1. A ray with a component of o or d that is not finite is a miss.
//   2. Box: te = near, tx = far; per axis with d[a] != 0: (ta, tb) = (T(a, 0), T(a, c[a])), swapped when d[a] < 0,
//      te = max(te, ta), tx = min(tx, tb); an axis with d[a] == +-0 makes the ray a miss unless x(a, 0) <= o[a] <= x(a, c[a]),
//      and constrains nothing otherwise.  A miss unless te < tx.
//   3. First cell, per axis: the estimate floor((p - lo[a]) / cell[a]) with p = o[a] + d[a] * te (p = o[a] for d[a] == 0),
//      clamped to [0, c[a] - 1], then corrected by at most one cell with the planes' own T (positions for d[a] == 0):
//      d > 0: T(i) > te -> i - 1, else T(i + 1) <= te -> i + 1;  d < 0: T(i + 1) > te -> i + 1, else T(i) <= te -> i - 1.
//      The cell therefore comes from comparisons of accurate T, not from a rounded position.
//   4. Walk, at most c[0] + c[1] + c[2] + 3 steps, tc = te: tn[a] = T of the plane the ray leaves the cell through on
//      axis a (+inf for d[a] == 0), tout = min(tn[0], tn[1], tn[2], tx).  An occupied cell with tout > tc counts: the
//      first one sets t0 = tc, every one sets t1 = tout.  Stop unless tout < tx; otherwise step along the axis of the
//      smallest tn (ties: x before y before z), stop when that leaves the grid, tc = max(tc, tout).
//   5. Without a counted cell the ray is a miss: t = (near, far), hit = 0, affine = (0, 1), the row is copied.  Otherwise
//      t1 = far when clip_far == 0; if t1 - t0 < min_span both ends move out by half the difference and are clamped to
//      [near, far]; b = (t1 - t0) / (far - near), a = t0 - b * near ((0, 1) and a copied row when t0 == near and
//      t1 == far); o' = o + d * a, d' = b * d, columns 6 .. ray_ld - 1 are copied.
// ------------------------------------------------------------------------------------------------
HN_DEV float hn_occ_plane(const HnOccGrid& g, int a, int i) { return __fadd_rn(g.lo[a], __fmul_rn((float)i, g.cell[a])); }
HN_DEV float hn_occ_t(const HnOccGrid& g, int a, int i, float o, float d) {
  return __fdiv_rn(__fsub_rn(hn_occ_plane(g, a, i), o), d);
}

// Steps 1-4 for one ray against the grid whose words start at `bits`: true when a cell counted, with t0 the entry of the
// first and t1 the exit of the last counted cell (both untouched otherwise).  first_only ends the walk at the first
// counted cell: t0 is final there, and t1 is only that cell's exit — for a caller that replaces it (clip_far == 0).
HN_DEV bool hn_occ_walk(const HnOccGrid& g, const unsigned long long* __restrict__ bits, float o0, float o1, float o2,
                        float d0, float d1, float d2, float near, float far, bool first_only, float& t0, float& t1) {
  const float inf = __builtin_huge_valf(), fmax_ = 3.402823466e38f;
  const float o[3] = {o0, o1, o2}, d[3] = {d0, d1, d2};
  bool hit = false;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && fabsf(o[a]) <= fmax_ && fabsf(d[a]) <= fmax_;
  float te = near, tx = far;
  if (ok) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (d[a] == 0.0f) {
        ok = ok && o[a] >= hn_occ_plane(g, a, 0) && o[a] <= hn_occ_plane(g, a, g.c[a]);
      } else {
        const float tlo = hn_occ_t(g, a, 0, o[a], d[a]), thi = hn_occ_t(g, a, g.c[a], o[a], d[a]);
        te = fmaxf(te, d[a] > 0.0f ? tlo : thi);
        tx = fminf(tx, d[a] > 0.0f ? thi : tlo);
      }
    }
    ok = ok && te < tx;
  }
  if (ok) {
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int last = g.c[a] - 1;
      const float p = d[a] == 0.0f ? o[a] : __fadd_rn(o[a], __fmul_rn(d[a], te));
      const float fl = floorf(__fdiv_rn(__fsub_rn(p, g.lo[a]), g.cell[a]));
      int i = !(fl > 0.0f) ? 0 : (fl > (float)last ? last : (int)fl);
      if (d[a] > 0.0f) {
        if (i > 0 && hn_occ_t(g, a, i, o[a], d[a]) > te) --i;
        else if (i < last && hn_occ_t(g, a, i + 1, o[a], d[a]) <= te) ++i;
      } else if (d[a] < 0.0f) {
        if (i < last && hn_occ_t(g, a, i + 1, o[a], d[a]) > te) ++i;
        else if (i > 0 && hn_occ_t(g, a, i, o[a], d[a]) <= te) --i;
      } else {
        if (i > 0 && hn_occ_plane(g, a, i) > o[a]) --i;
        else if (i < last && hn_occ_plane(g, a, i + 1) <= o[a]) ++i;
      }
      idx[a] = i;
    }
    int i0 = idx[0], i1 = idx[1], i2 = idx[2];
    float tc = te;
    const int max_steps = g.c[0] + g.c[1] + g.c[2] + 3;
    for (int step = 0; step < max_steps; ++step) {
      const float tn0 = d0 > 0.0f ? hn_occ_t(g, 0, i0 + 1, o0, d0) : (d0 < 0.0f ? hn_occ_t(g, 0, i0, o0, d0) : inf);
      const float tn1 = d1 > 0.0f ? hn_occ_t(g, 1, i1 + 1, o1, d1) : (d1 < 0.0f ? hn_occ_t(g, 1, i1, o1, d1) : inf);
      const float tn2 = d2 > 0.0f ? hn_occ_t(g, 2, i2 + 1, o2, d2) : (d2 < 0.0f ? hn_occ_t(g, 2, i2, o2, d2) : inf);
      const float tout = fminf(fminf(tn0, tn1), fminf(tn2, tx));
      const unsigned long long word = bits[((size_t)i0 * g.c[1] + i1) * g.words + (i2 >> 6)];
      if (((word >> (i2 & 63)) & 1ull) != 0ull && tout > tc) {
        if (!hit) t0 = tc;
        t1 = tout;
        hit = true;
        if (first_only) break;
      }
      if (!(tout < tx)) break;
      if (tn0 <= tn1 && tn0 <= tn2) {
        i0 += d0 > 0.0f ? 1 : -1;
        if (i0 < 0 || i0 >= g.c[0]) break;
      } else if (tn1 <= tn2) {
        i1 += d1 > 0.0f ? 1 : -1;
        if (i1 < 0 || i1 >= g.c[1]) break;
      } else {
        i2 += d2 > 0.0f ? 1 : -1;
        if (i2 < 0 || i2 >= g.c[2]) break;
      }
      tc = fmaxf(tc, tout);
    }
  }
  return hit;
}

// Step 5 up to the affine map: (t0, t1) of a hit become final (clip_far, min_span), those of a miss (near, far); true
// when the row is to be copied ((t0, t1) == (near, far): a = 0, b = 1).
HN_DEV bool hn_occ_span(bool hit, float near, float far, int clip_far, float min_span, float& t0, float& t1, float& a,
                        float& b) {
  if (hit) {
    if (clip_far == 0) t1 = far;
    const float span = __fsub_rn(t1, t0);
    if (span < min_span) {
      const float grow = __fmul_rn(0.5f, __fsub_rn(min_span, span));
      t0 = fmaxf(near, __fsub_rn(t0, grow));
      t1 = fminf(far, __fadd_rn(t1, grow));
    }
  } else {
    t0 = near;
    t1 = far;
  }
  const bool identity = t0 == near && t1 == far;
  b = identity ? 1.0f : __fdiv_rn(__fsub_rn(t1, t0), __fsub_rn(far, near));
  a = identity ? 0.0f : __fsub_rn(t0, __fmul_rn(b, near));
  return identity;
}

// The output row: o + d * a, b * d (the input's bits when `identity`), columns 6 .. ray_ld - 1 copied.
HN_DEV void hn_occ_store_row(const float* __restrict__ row, int ray_ld, bool identity, float a, float b,
                             float* __restrict__ dst) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float oc = row[c], dc = row[3 + c];
    dst[c] = identity ? oc : __fadd_rn(oc, __fmul_rn(dc, a));
    dst[3 + c] = identity ? dc : __fmul_rn(b, dc);
  }
  for (int c = 6; c < ray_ld; ++c) dst[c] = row[c];
}

__global__ __launch_bounds__(256) void hn_occ_clip_rays_kernel(const float* __restrict__ rays, long long n, int ray_ld,
                                                               const unsigned long long* __restrict__ bits, HnOccGrid g,
                                                               float near, float far, int clip_far, float min_span,
                                                               float* __restrict__ t_out, uint8_t* __restrict__ hit_out,
                                                               float* __restrict__ rays_out,
                                                               float* __restrict__ affine_out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float* __restrict__ row = rays + (size_t)r * ray_ld;
  float t0 = near, t1 = far, a, b;
  const bool hit = hn_occ_walk(g, bits, row[0], row[1], row[2], row[3], row[4], row[5], near, far, false, t0, t1);
  const bool identity = hn_occ_span(hit, near, far, clip_far, min_span, t0, t1, a, b);
  if (t_out != nullptr) {
    t_out[2 * (size_t)r] = t0;
    t_out[2 * (size_t)r + 1] = t1;
  }
  if (hit_out != nullptr) hit_out[r] = (uint8_t)hit;
  if (affine_out != nullptr) {
    affine_out[2 * (size_t)r] = a;
    affine_out[2 * (size_t)r + 1] = b;
  }
  if (rays_out != nullptr) hn_occ_store_row(row, ray_ld, identity, a, b, rays_out + (size_t)r * ray_ld);
}

extern "C" int hn_occ_clip_rays(const float* rays_dev, long long n, int ray_ld, const uint64_t* bits_dev, int cx, int cy,
                                int cz, const float* bounds_host, float t_near, float t_far, int clip_far, float min_span,
                                float* t_dev, uint8_t* hit_dev, float* rays_out_dev, float* affine_dev, hnStream_t stream) {
  HnOccGrid g;
  if (bounds_host == nullptr || !hn_occ_grid(cx, cy, cz, bounds_host, &g)) return -2;
  if (n < 1 || n > 2147483647ll || ray_ld < 6 || ray_ld > 64) return -2;
  if (!(fabsf(t_near) <= 3.402823466e38f) || !(fabsf(t_far) <= 3.402823466e38f) || !(t_far > t_near)) return -2;
  if (!(min_span >= 0.0f && min_span <= 3.402823466e38f)) return -2;
  if (rays_dev == nullptr || bits_dev == nullptr) return -3;
  if (rays_out_dev == rays_dev) return -2;
  hipLaunchKernelGGL(hn_occ_clip_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rays_dev, n, ray_ld, reinterpret_cast<const unsigned long long*>(bits_dev), g, t_near, t_far,
                     clip_far, min_span, t_dev, hit_dev, rays_out_dev, affine_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_occ_clip_batch: the same clip for a batch that mixes frames, one ray per lane, each against the grid of its own
// frame.  bits holds n_slots grids of one geometry back to back; the ray's id v (column id_col of its row, 0 when
// id_col < 0) picks slot_of_id[(int)v] when v is finite and 0 <= (int)v < n_ids.  Any other v, and a slot outside
// [0, n_slots), means "no grid": the row is copied, hit = 0, affine = (0, 1).  With a slot, steps 1-5 above on that grid;
// clip_far == 0 ends the walk at the first counted cell (t1 becomes far whatever the rest of the walk would find).
// Every pointer the launch reads is fixed: a replayed graph sees what the host wrote into bits and slot_of_id since.
// hit_count: zeroed on the stream ahead of the launch, then one integer atomic per wave after a wave reduction (the count
// does not depend on their order).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_occ_clip_batch_kernel(const float* __restrict__ rays, long long n, int ray_ld,
                                                                int id_col, const unsigned long long* __restrict__ bits,
                                                                int n_slots, const int32_t* __restrict__ slot_of_id,
                                                                int n_ids, HnOccGrid g, float near, float far, int clip_far,
                                                                float min_span, float* __restrict__ rays_out,
                                                                float* __restrict__ viewdirs_out,
                                                                float* __restrict__ affine_out,
                                                                uint8_t* __restrict__ hit_out,
                                                                unsigned long long* __restrict__ hit_count) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (r < n) {      // no early return: every lane of the wave takes part in the reduction below
    const float* __restrict__ row = rays + (size_t)r * ray_ld;
    const float v = id_col < 0 ? 0.0f : row[id_col];
    int slot = -1;
    if (v > -1.0f && v < 2147483648.0f) {      // false for NaN and +-inf; (int)v is then defined, and >= 0
      const int id = (int)v;
      if (id < n_ids) slot = slot_of_id[id];
    }
    float t0 = near, t1 = far, a, b;
    if (slot >= 0 && slot < n_slots) {
      const unsigned long long* __restrict__ grid = bits + (size_t)slot * g.c[0] * g.c[1] * g.words;
      hit = hn_occ_walk(g, grid, row[0], row[1], row[2], row[3], row[4], row[5], near, far, clip_far == 0, t0, t1);
    }
    const bool identity = hn_occ_span(hit, near, far, clip_far, min_span, t0, t1, a, b);
    if (hit_out != nullptr) hit_out[r] = (uint8_t)hit;
    if (affine_out != nullptr) {
      affine_out[2 * (size_t)r] = a;
      affine_out[2 * (size_t)r + 1] = b;
    }
    if (viewdirs_out != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) viewdirs_out[3 * (size_t)r + c] = row[3 + c];
    }
    if (rays_out != nullptr) hn_occ_store_row(row, ray_ld, identity, a, b, rays_out + (size_t)r * ray_ld);
  }
  if (hit_count != nullptr) {
    int c = hit ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(hit_count, (unsigned long long)c);
  }
}

__global__ void hn_occ_zero_kernel(unsigned long long* __restrict__ count) {
  if (threadIdx.x == 0) *count = 0ull;
}

extern "C" int hn_occ_clip_batch(const float* rays_dev, long long n, int ray_ld, int id_col, const uint64_t* bits_dev,
                                 int n_slots, int cx, int cy, int cz, const int32_t* slot_of_id_dev, int n_ids,
                                 const float* bounds_host, float t_near, float t_far, int clip_far, float min_span,
                                 float* rays_out_dev, float* viewdirs_out_dev, float* affine_dev, uint8_t* hit_dev,
                                 int64_t* hit_count_dev, hnStream_t stream) {
  HnOccGrid g;
  if (bounds_host == nullptr || !hn_occ_grid(cx, cy, cz, bounds_host, &g)) return -2;
  if (n < 1 || n > 2147483647ll || ray_ld < 6 || ray_ld > 64) return -2;
  if (id_col >= ray_ld || (id_col >= 0 && id_col < 6)) return -2;
  if (n_slots < 1 || n_ids < 1) return -2;
  if (!(fabsf(t_near) <= 3.402823466e38f) || !(fabsf(t_far) <= 3.402823466e38f) || !(t_far > t_near)) return -2;
  if (!(min_span >= 0.0f && min_span <= 3.402823466e38f)) return -2;
  if (rays_dev == nullptr || bits_dev == nullptr || slot_of_id_dev == nullptr) return -3;
  if (rays_out_dev == rays_dev) return -2;
  if (hit_count_dev != nullptr) {
    // a one-lane kernel node, not a memset node: under replays that alternate with eager work the memset node of this
    // counter was seen to leave 0x01 bytes behind once in a dozen replays on the MI355X
    hipLaunchKernelGGL(hn_occ_zero_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long*>(hit_count_dev));
    HN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(hn_occ_clip_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rays_dev, n, ray_ld, id_col, reinterpret_cast<const unsigned long long*>(bits_dev), n_slots,
                     slot_of_id_dev, n_ids, g, t_near, t_far, clip_far, min_span, rays_out_dev, viewdirs_out_dev, affine_dev,
                     hit_dev, reinterpret_cast<unsigned long long*>(hit_count_dev));
  HN_CHECK_LAUNCH();
  return 0;
}
