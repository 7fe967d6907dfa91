// Mesh registration for gfx950: the similarity transform of a point set and the sums an ICP iteration solves from.
//
// Definition (DESIGN.md 3.15 holds it in full; tests/registration_restated.py restates it in NumPy, bit for bit).
//   transform  out = s * (R p) + t in fp32, every operation rounded on its own (__f*_rn; the library is built with
//              contraction off): row_i = (R_i0*x + R_i1*y) + R_i2*z, out_i = row_i * s + t_i.  The direction form has no
//              s and no t: out = row / len, len = sqrtf((row_0^2 + row_1^2) + row_2^2), row itself unless len > 0 (a zero
//              vector stays zero).  A point with a coordinate that is not finite gives NaN, NaN, NaN.
//   inlier     point k counts when distance[k] <= tau (false for NaN; +inf only fails the finite test), distance[k] is
//              finite, 0 <= face[k] < F and, in plane mode, its face has a normal of positive finite length.  Everything
//              else is skipped: its rows are never read into a sum, not even multiplied by zero.
//   terms      every input is converted to double first, every double operation is rounded on its own;
//              dot(u, v) = (ux*vx + uy*vy) + uz*vz, cross(u, v)_x = uy*vz - uz*vy (and cyclic).
//              point mode, HN_REG_POINT_SUMS values: 1 | d*d | p (3) | q (3) | q_i*p_j (9, index 3 i + j) | dot(p, p) |
//              dot(q, q), d the fp32 distance, p the point, q its closest point.
//              plane mode, HN_REG_SUMS values: 1 | d*d | r*r | J_a*J_b for a <= b (28, rows of the upper triangle) |
//              J_a*r (7), with m = cross(B - A, C - A) of the packed triangle, len = sqrt(dot(m, m)), n = m / len,
//              r = dot(p - q, n), J = [cross(p, n), n, dot(p, n)].
//   order      thread g = block * 256 + lane-in-block starts from +0 and adds the terms of the inliers among points g,
//              g + T, g + 2 T, ... (T = 256 n_blocks) in that order; a wave folds its 64 lanes by x[l] += x[l + w] for
//              w = 32, 16, 8, 4, 2, 1; the block adds its four waves as (w0 + w1) + (w2 + w3); the finishing launch
//              adds the n_blocks partials of a value one after the other from +0 in block order.  A function of N
//              and n_blocks only: no atomics, the same bits on every run.
#include <float.h>

#include "hn_common.h"

// Limits the host half mirrors (ops/registration; tests/test_registration_host.py compares the two)
#define HN_REG_THREADS 256        // threads per workgroup of the moments launch
#define HN_REG_MAX_BLOCKS 1024    // the most workgroups (partials) a moments launch takes
#define HN_REG_POINT_SUMS 19      // values of a point-mode result
#define HN_REG_SUMS 38            // values of a plane-mode result, and the doubles per partial and per result
#define HN_REG_PARAMS 13          // host floats of a transform: R row-major (9), s, t (3)

#define HN_REG_STAGE_BLOCKS 128   // partials the finishing pass holds in LDS at a time (38 KiB)

// ------------------------------------------------------------------------------------------------
// hn_reg_transform
// ------------------------------------------------------------------------------------------------
struct HnRegParams {
  float r[9], s, t[3];
};

__global__ __launch_bounds__(256) void hn_reg_transform_kernel(const float* __restrict__ points, long long n, HnRegParams m,
                                                               int direction, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  float o[3] = {NAN, NAN, NAN};
  if (fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX) {
    float row[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      row[c] = __fadd_rn(__fadd_rn(__fmul_rn(m.r[3 * c], x), __fmul_rn(m.r[3 * c + 1], y)), __fmul_rn(m.r[3 * c + 2], z));
    if (direction) {
      // sqrtf, not __fsqrt_rn: the correctly rounded root (csrc/hn_mesh_distance.hip has the reason)
      const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(row[0], row[0]), __fmul_rn(row[1], row[1])), __fmul_rn(row[2], row[2])));
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = len > 0.0f ? __fdiv_rn(row[c], len) : row[c];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = __fadd_rn(__fmul_rn(row[c], m.s), m.t[c]);
    }
  }
  out[3 * (size_t)i] = o[0];
  out[3 * (size_t)i + 1] = o[1];
  out[3 * (size_t)i + 2] = o[2];
}

extern "C" int hn_reg_transform(const float* points_dev, long long n, const float* params_host, int direction, float* out_dev,
                                hnStream_t stream) {
  if (n <= 0 || n > 2147483647ll || params_host == nullptr || (direction != 0 && direction != 1)) return -2;
  HnRegParams m;
  for (int k = 0; k < HN_REG_PARAMS; ++k) {
    const float v = params_host[k];
    if (!(v >= -FLT_MAX && v <= FLT_MAX)) return -2;
    (k < 9 ? m.r[k] : k == 9 ? m.s : m.t[k - 10]) = v;
  }
  if (points_dev == nullptr || out_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_reg_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points_dev,
                     n, m, direction, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_reg_moments
// ------------------------------------------------------------------------------------------------
HN_DEV double hn_reg_dot(const double* a, const double* b) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
}

HN_DEV void hn_reg_cross(const double* a, const double* b, double* out) {
  out[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
  out[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
  out[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
}

// PLANE = false: HN_REG_POINT_SUMS values per thread; true: HN_REG_SUMS.  Every accumulator index is a constant after
// unrolling: registers, no scratch.
template <bool PLANE>
__global__ __launch_bounds__(HN_REG_THREADS) void hn_reg_moments_kernel(const float* __restrict__ points,
                                                                        const float* __restrict__ closest,
                                                                        const float* __restrict__ distance,
                                                                        const int32_t* __restrict__ face, long long n,
                                                                        const float* __restrict__ tri, long long n_faces,
                                                                        const float* __restrict__ tau_dev,
                                                                        double* __restrict__ partials) {
  constexpr int NS = PLANE ? HN_REG_SUMS : HN_REG_POINT_SUMS;
  __shared__ double wave_sums[HN_REG_THREADS / 64][HN_REG_SUMS];
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  const float tau = tau_dev[0];
  const long long stride = (long long)gridDim.x * HN_REG_THREADS;
  for (long long i = (long long)blockIdx.x * HN_REG_THREADS + threadIdx.x; i < n; i += stride) {
    const float d32 = distance[i];
    const int32_t f = face[i];
    if (!(d32 <= tau) || !(fabsf(d32) <= FLT_MAX) || f < 0 || f >= n_faces) continue;
    const double d = (double)d32;
    const double p[3] = {(double)points[3 * (size_t)i], (double)points[3 * (size_t)i + 1], (double)points[3 * (size_t)i + 2]};
    const double q[3] = {(double)closest[3 * (size_t)i], (double)closest[3 * (size_t)i + 1], (double)closest[3 * (size_t)i + 2]};
    if (!PLANE) {
      acc[0] = __dadd_rn(acc[0], 1.0);
      acc[1] = __dadd_rn(acc[1], __dmul_rn(d, d));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        acc[2 + c] = __dadd_rn(acc[2 + c], p[c]);
        acc[5 + c] = __dadd_rn(acc[5 + c], q[c]);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[8 + 3 * c + j] = __dadd_rn(acc[8 + 3 * c + j], __dmul_rn(q[c], p[j]));
      }
      acc[17] = __dadd_rn(acc[17], hn_reg_dot(p, p));
      acc[18] = __dadd_rn(acc[18], hn_reg_dot(q, q));
    } else {
      const f32x4* t4 = reinterpret_cast<const f32x4*>(tri + 12 * (size_t)f);      // a packed triangle of hn_md_pack
      const f32x4 t0 = t4[0], t1 = t4[1], t2 = t4[2];
      const double a[3] = {(double)t0[0], (double)t0[1], (double)t0[2]};
      const double e1[3] = {__dsub_rn((double)t0[3], a[0]), __dsub_rn((double)t1[0], a[1]), __dsub_rn((double)t1[1], a[2])};
      const double e2[3] = {__dsub_rn((double)t1[2], a[0]), __dsub_rn((double)t1[3], a[1]), __dsub_rn((double)t2[0], a[2])};
      double m[3];
      hn_reg_cross(e1, e2, m);
      const double len = sqrt(hn_reg_dot(m, m));      // sqrt and / of doubles are the correctly rounded ones
      if (!(len > 0.0) || !(len <= DBL_MAX)) continue;      // no area, an overflow, a NaN corner
      const double nrm[3] = {m[0] / len, m[1] / len, m[2] / len};
      const double pq[3] = {__dsub_rn(p[0], q[0]), __dsub_rn(p[1], q[1]), __dsub_rn(p[2], q[2])};
      const double r = hn_reg_dot(pq, nrm);
      double J[7];
      hn_reg_cross(p, nrm, J);
      J[3] = nrm[0];
      J[4] = nrm[1];
      J[5] = nrm[2];
      J[6] = hn_reg_dot(p, nrm);
      acc[0] = __dadd_rn(acc[0], 1.0);
      acc[1] = __dadd_rn(acc[1], __dmul_rn(d, d));
      acc[2] = __dadd_rn(acc[2], __dmul_rn(r, r));
#pragma unroll
      for (int ja = 0; ja < 7; ++ja)
#pragma unroll
        for (int jb = ja; jb < 7; ++jb) {
          const int k = 3 + 7 * ja - ja * (ja - 1) / 2 + (jb - ja);      // row ja of the upper triangle starts here
          acc[k] = __dadd_rn(acc[k], __dmul_rn(J[ja], J[jb]));
        }
#pragma unroll
      for (int ja = 0; ja < 7; ++ja) acc[31 + ja] = __dadd_rn(acc[31 + ja], __dmul_rn(J[ja], r));
    }
  }
  // the wave's tree: x[l] += x[l + w]; lane 0 ends with the wave's sum (what the other lanes hold is not used)
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1)
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = __dadd_rn(acc[k], __shfl_down(acc[k], w, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NS; ++k) wave_sums[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < HN_REG_SUMS) {
    const int k = threadIdx.x;
    double v = 0.0;
    if (k < NS) v = __dadd_rn(__dadd_rn(wave_sums[0][k], wave_sums[1][k]), __dadd_rn(wave_sums[2][k], wave_sums[3][k]));
    partials[(size_t)blockIdx.x * HN_REG_SUMS + k] = v;
  }
}

static_assert(HN_REG_THREADS == 256, "four waves per workgroup: the block's tree is (w0 + w1) + (w2 + w3)");

__global__ __launch_bounds__(256) void hn_reg_finish_kernel(const double* __restrict__ partials, int n_blocks,
                                                            double* __restrict__ sums) {
  __shared__ double stage[HN_REG_STAGE_BLOCKS * HN_REG_SUMS];
  double s = 0.0;
  for (int base = 0; base < n_blocks; base += HN_REG_STAGE_BLOCKS) {
    const int blocks = min(HN_REG_STAGE_BLOCKS, n_blocks - base);
    for (int j = threadIdx.x; j < blocks * HN_REG_SUMS; j += 256) stage[j] = partials[(size_t)base * HN_REG_SUMS + j];
    __syncthreads();
    if (threadIdx.x < HN_REG_SUMS) {
      // eight LDS reads in flight, then their additions one after the other: the order is that of the plain loop
      int b = 0;
      for (; b + 8 <= blocks; b += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = stage[(b + j) * HN_REG_SUMS + threadIdx.x];
#pragma unroll
        for (int j = 0; j < 8; ++j) s = __dadd_rn(s, v[j]);
      }
      for (; b < blocks; ++b) s = __dadd_rn(s, stage[b * HN_REG_SUMS + threadIdx.x]);
    }
    __syncthreads();
  }
  if (threadIdx.x < HN_REG_SUMS) sums[threadIdx.x] = s;
}

extern "C" int hn_reg_moments(const float* points_dev, const float* closest_dev, const float* distance_dev,
                              const int32_t* face_dev, long long n, const float* tri_dev, long long n_faces,
                              const float* tau_dev, int mode, int n_blocks, double* partials_dev, double* sums_dev,
                              hnStream_t stream) {
  if (n <= 0 || n > 2147483647ll || n_faces <= 0 || n_faces > 2147483647ll || (mode != 0 && mode != 1) || n_blocks < 1 ||
      n_blocks > HN_REG_MAX_BLOCKS)
    return -2;
  if (points_dev == nullptr || closest_dev == nullptr || distance_dev == nullptr || face_dev == nullptr || tau_dev == nullptr ||
      partials_dev == nullptr || sums_dev == nullptr || (mode == 1 && tri_dev == nullptr))
    return -3;
  if (mode == 1)
    hipLaunchKernelGGL(hn_reg_moments_kernel<true>, dim3((unsigned)n_blocks), dim3(HN_REG_THREADS), 0, (hipStream_t)stream,
                       points_dev, closest_dev, distance_dev, face_dev, n, tri_dev, n_faces, tau_dev, partials_dev);
  else
    hipLaunchKernelGGL(hn_reg_moments_kernel<false>, dim3((unsigned)n_blocks), dim3(HN_REG_THREADS), 0, (hipStream_t)stream,
                       points_dev, closest_dev, distance_dev, face_dev, n, tri_dev, n_faces, tau_dev, partials_dev);
  HN_CHECK_LAUNCH();
  hipLaunchKernelGGL(hn_reg_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials_dev, n_blocks, sums_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
