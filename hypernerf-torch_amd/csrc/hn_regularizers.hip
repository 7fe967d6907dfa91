// Regularization terms of a training step for gfx950 that do not come from rendered rays.
//
// Background regularization (HyperNeRF's training loop, on by default in its configs): a batch of the capture's static
// structure-from-motion points goes through the warp field under randomly chosen warp embeddings and a robust loss pulls
// warp(p) back to p.  Two kernels: the sampler that draws the batch from the point table (hn_bg_sample) and the loss
// head (hn_bg_loss_*), Barron's general loss at alpha = -2 (Geman-McClure) on the squared residual.  Both are a few
// bytes per point and HBM / latency bound; the warp field between them is the MLP machine's business.
#include "hn_common.h"
#include "hn_window.h"      // hn_wave_sum

// ------------------------------------------------------------------------------------------------
// sampler: out_ids[n] = ids[min(int(u[n,1] * K), K-1)], out_points[n] = points[min(int(u[n,0] * M), M-1)] + std * nrm[n]
// u = 24-bit uniforms in [0, 1) and nrm = normals of hn_random_fill (no second generator here).  The products u * M
// and std * nrm and the sum are rounded one by one (no contraction), so a float32 NumPy restatement is bit-exact.
// One thread per drawn point.  The indices are clamped on both sides: whatever `u` holds (an injected buffer may hold
// anything), nothing outside the two tables is read.
// ------------------------------------------------------------------------------------------------
HN_DEV int hn_bg_index(float u, int rows) {
  const float f = __fmul_rn(u, (float)rows);      // rows <= 2^24: (float)rows is exact
  if (!(f > 0.0f)) return 0;                      // NaN and negatives as well
  if (f >= (float)rows) return rows - 1;
  return (int)f;                                  // truncation, as numpy's astype(int64) of a non-negative float
}

__global__ __launch_bounds__(256) void hn_bg_sample_kernel(const float* __restrict__ points, int m,
                                                           const int64_t* __restrict__ ids, int k,
                                                           const float* __restrict__ u, const float* __restrict__ nrm,
                                                           int n, float noise_std, float* __restrict__ out_points,
                                                           int64_t* __restrict__ out_ids) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int i = hn_bg_index(u[2 * (size_t)row], m);
  const int j = hn_bg_index(u[2 * (size_t)row + 1], k);
  out_ids[row] = ids[j];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out_points[3 * (size_t)row + c] = __fadd_rn(points[3 * (size_t)i + c], __fmul_rn(noise_std, nrm[3 * (size_t)row + c]));
}

extern "C" int hn_bg_sample(const float* points, int m, const int64_t* ids, int k, const float* u, const float* nrm, int n,
                            float noise_std, float* out_points, int64_t* out_ids, hnStream_t stream) {
  if (n <= 0 || m <= 0 || k <= 0 || m > (1 << 24) || k > (1 << 24)) return -2;
  if (points == nullptr || ids == nullptr || u == nullptr || nrm == nullptr || out_points == nullptr || out_ids == nullptr)
    return -2;
  hipLaunchKernelGGL(hn_bg_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, m,
                     ids, k, u, nrm, n, noise_std, out_points, out_ids);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// loss head: x_n = |w_n - p_n|^2 / scale^2, loss = mean_n 2 x_n / (x_n + 4),
// d loss / d w_n = 16 (w_n - p_n) / (scale^2 (x_n + 4)^2 N); p carries no gradient.  x = 0 gives 0 and 0 (no division
// by the residual anywhere).  One row's arithmetic is ONE device function for the forward, the forward that also writes
// the gradient, and the backward: the gradients of the last two agree bit for bit for a root gradient of 1.
// The mean as hn_mse_fwd_kernel takes it: one workgroup, per-thread sums in row order, a wave64 butterfly, sixteen wave
// sums added in order by one thread — no float atomics, the same bits every run.
// ------------------------------------------------------------------------------------------------
struct HnBgRow { float loss; float d[3]; };

// gs = g * 16 / (scale^2 N) (hn_bg_gscale); inv_s2 = 1 / scale^2
HN_DEV HnBgRow hn_bg_row(const float* __restrict__ w, const float* __restrict__ p, float inv_s2, float gs) {
  const float d0 = w[0] - p[0], d1 = w[1] - p[1], d2 = w[2] - p[2];
  const float x = (d0 * d0 + d1 * d1 + d2 * d2) * inv_s2;
  const float t = x + 4.0f;
  const float coef = gs / (t * t);
  HnBgRow r;
  r.loss = 2.0f * x / t;
  r.d[0] = d0 * coef; r.d[1] = d1 * coef; r.d[2] = d2 * coef;
  return r;
}
HN_DEV float hn_bg_gscale(float g, float inv_s2, int n) { return g * 16.0f * inv_s2 / (float)n; }

__global__ __launch_bounds__(1024) void hn_bg_loss_fwd_kernel(const float* __restrict__ warped,
                                                              const float* __restrict__ points, int n, float inv_s2,
                                                              float* __restrict__ loss, float* __restrict__ d_warped) {
  __shared__ float part[16];
  const float gs = hn_bg_gscale(1.0f, inv_s2, n);      // hn_bg_loss_bwd_kernel's factor for a root gradient of exactly 1
  float s = 0.0f;
  for (int row = threadIdx.x; row < n; row += 1024) {
    const HnBgRow r = hn_bg_row(warped + 3 * (size_t)row, points + 3 * (size_t)row, inv_s2, gs);
    s += r.loss;
    if (d_warped != nullptr) {
      float* o = d_warped + 3 * (size_t)row;
      o[0] = r.d[0]; o[1] = r.d[1]; o[2] = r.d[2];
    }
  }
  s = hn_wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.0f;
    for (int k = 0; k < 16; ++k) a += part[k];
    loss[0] = a / (float)n;
  }
}

__global__ __launch_bounds__(256) void hn_bg_loss_bwd_kernel(const float* __restrict__ warped,
                                                             const float* __restrict__ points, int n, float inv_s2,
                                                             const float* __restrict__ g_loss,
                                                             float* __restrict__ d_warped) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const float gs = hn_bg_gscale(g_loss[0], inv_s2, n);
  const HnBgRow r = hn_bg_row(warped + 3 * (size_t)row, points + 3 * (size_t)row, inv_s2, gs);
  float* o = d_warped + 3 * (size_t)row;
  o[0] = r.d[0]; o[1] = r.d[1]; o[2] = r.d[2];
}

// 1 / scale^2, rounded once (the product and the quotient in double)
static float hn_bg_inv_s2(float scale) { return (float)(1.0 / ((double)scale * (double)scale)); }

extern "C" int hn_bg_loss_forward(const float* warped, const float* points, int n, float scale, float* loss_out,
                                  hnStream_t stream) {
  if (n <= 0 || !(scale > 0.0f)) return -2;
  if (warped == nullptr || points == nullptr || loss_out == nullptr) return -2;
  hipLaunchKernelGGL(hn_bg_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, warped, points, n,
                     hn_bg_inv_s2(scale), loss_out, (float*)nullptr);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_bg_loss_forward_grad(const float* warped, const float* points, int n, float scale, float* loss_out,
                                       float* d_warped, hnStream_t stream) {
  if (n <= 0 || !(scale > 0.0f)) return -2;
  if (warped == nullptr || points == nullptr || loss_out == nullptr || d_warped == nullptr) return -2;
  hipLaunchKernelGGL(hn_bg_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, warped, points, n,
                     hn_bg_inv_s2(scale), loss_out, d_warped);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_bg_loss_backward(const float* warped, const float* points, int n, float scale, const float* g_loss,
                                   float* d_warped, hnStream_t stream) {
  if (n <= 0 || !(scale > 0.0f)) return -2;
  if (warped == nullptr || points == nullptr || g_loss == nullptr || d_warped == nullptr) return -2;
  hipLaunchKernelGGL(hn_bg_loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, warped,
                     points, n, hn_bg_inv_s2(scale), g_loss, d_warped);
  HN_CHECK_LAUNCH();
  return 0;
}
