// Regularization terms of a training step for gfx950 beside the photometric loss.
//
// Background regularization (HyperNeRF's training loop, on by default in its configs): a batch of the capture's static
// structure-from-motion points goes through the warp field under randomly chosen warp embeddings and a robust loss pulls
// warp(p) back to p.  Two kernels: the sampler that draws the batch from the point table (hn_bg_sample) and the loss
// head (hn_bg_loss_*), Barron's general loss at alpha = -2 (Geman-McClure) on the squared residual.  Both are a few
// bytes per point and HBM / latency bound; the warp field between them is the MLP machine's business.
//
// Distortion loss (Mip-NeRF 360): a per-ray penalty on compositing weights that are spread out or split along the ray,
// behind the compositing launch (hn_distortion_*, at the end of this file).
#include "hn_common.h"
#include "hn_wave.h"        // the wave64 scans
#include "hn_window.h"      // hn_wave_sum, hn_block_sum

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

// ------------------------------------------------------------------------------------------------
// distortion loss (Mip-NeRF 360, eq. 15) on one level's compositing weights, in the weights' sorted order:
//   s_i = (z_i - near) / (far - near)  [linear]  or  (1/z_i - 1/near) / (1/far - 1/near)  [disparity],
//   sample i < S-1 owns [s_i, s_{i+1}]: d_i = s_{i+1} - s_i, m_i = (s_i + s_{i+1}) / 2; the last one d = 0, m = s_{S-1},
//   L_ray = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i,   dL_ray/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i.
// The midpoints ascend with i, so sum_j w_j |m_i - m_j| = m_i (A_i - B_i) + (Bm_i - Am_i) with the exclusive prefixes
// A, Am and the exclusive suffixes B, Bm of sum w and sum w m: O(S) per ray.  One wave per ray, four rays per block,
// sample s = k * 64 + lane (hn_composite_ray's layout: the same coalesced rows); a forward sweep over the segments takes
// the prefixes (wave scan + carry), a backward sweep the suffixes (segment total - inclusive scan + carry).
// One ray's arithmetic is ONE device function for the forward, the forward that also writes the gradient, and the
// backward: the gradients of the last two agree bit for bit for equal root gradients.
// The mean: per-ray values go to `per_ray`; the block that arrives LAST (an integer ticket, as in hn_grad_norm_kernel)
// adds them in a fixed order — no float atomics, the same bits every run.
// ------------------------------------------------------------------------------------------------
constexpr int HN_DIST_SEG = 8;      // 512 samples per ray, as the compositing kernel
constexpr int HN_SPACING_LINEAR = 0, HN_SPACING_DISPARITY = 1;      // `spacing` of the entry points

struct HnDistRange { float near, inv_range, far; int disparity; };

// the disparity form is the linear one times far / z: (1/z - 1/near) / (1/far - 1/near) = (z - near) far / ((far - near) z),
// no difference of reciprocals
HN_DEV float hn_dist_s(const HnDistRange& r, float z) {
  const float t = (z - r.near) * r.inv_range;
  return r.disparity ? t * r.far / z : t;
}

// returns the ray's loss in lane 0; GRAD: d_w[s] = gs * dL_ray/dw_s
template <bool GRAD>
HN_DEV float hn_distortion_ray(const float* __restrict__ w, const float* __restrict__ z, int S, const HnDistRange& r,
                               float gs, float* __restrict__ d_w, int lane) {
  const int nseg = (S + 63) / 64;
  float wv[HN_DIST_SEG], mv[HN_DIST_SEG], dv[HN_DIST_SEG];      // weight, midpoint, width
  float pw[HN_DIST_SEG], pm[HN_DIST_SEG];                       // exclusive prefixes A, Am
  float iw[HN_DIST_SEG], im[HN_DIST_SEG];                       // inclusive scans inside the segment
  float tw[HN_DIST_SEG], tm[HN_DIST_SEG];                       // segment totals (wave-uniform)
  // every load of the ray first, at clamped indices (no branch around a load: they are all in flight together, one
  // memory latency for the ray instead of two per segment); mv / dv hold z_s / z_{s+1} until the sweep below
#pragma unroll
  for (int k = 0; k < HN_DIST_SEG; ++k) {
    if (k < nseg) {
      const int s = k * 64 + lane;
      wv[k] = w[min(s, S - 1)];
      mv[k] = z[min(s, S - 1)];
      dv[k] = z[min(s + 1, S - 1)];      // the last sample: its own depth, a point mass (d = 0, m = s_{S-1})
    }
  }
  float cw = 0.0f, cm = 0.0f;                                   // sums over all earlier segments
#pragma unroll
  for (int k = 0; k < HN_DIST_SEG; ++k) {
    if (k < nseg) {
      const int s = k * 64 + lane;
      const float wi = s < S ? wv[k] : 0.0f;
      const float s0 = hn_dist_s(r, mv[k]), s1 = hn_dist_s(r, dv[k]);
      const float d = s1 - s0, m = 0.5f * (s0 + s1);
      const float incw = hn_wave_incl_scan_add(wi, lane), incm = hn_wave_incl_scan_add(wi * m, lane);
      wv[k] = wi; mv[k] = m; dv[k] = d;
      pw[k] = cw + hn_wave_shr1(incw, 0.0f);
      pm[k] = cm + hn_wave_shr1(incm, 0.0f);
      iw[k] = incw; im[k] = incm;
      tw[k] = hn_wave_bcast(incw, 63);
      tm[k] = hn_wave_bcast(incm, 63);
      cw += tw[k];
      cm += tm[k];
    }
  }
  float sw = 0.0f, sm = 0.0f;      // sums over all later segments
  float acc = 0.0f;
#pragma unroll
  for (int k = HN_DIST_SEG - 1; k >= 0; --k) {
    if (k < nseg) {
      const int s = k * 64 + lane;
      const float bw = sw + (tw[k] - iw[k]), bm = sm + (tm[k] - im[k]);      // exclusive suffixes B, Bm
      const float inner = mv[k] * (pw[k] - bw) + (bm - pm[k]);               // sum_j w_j |m_i - m_j|
      const float self = wv[k] * dv[k];
      acc += wv[k] * (inner + (1.0f / 3.0f) * self);
      if (GRAD && s < S) d_w[s] = gs * (2.0f * inner + (2.0f / 3.0f) * self);
      sw += tw[k];
      sm += tm[k];
    }
  }
  return hn_wave_sum(acc);
}

template <bool GRAD>
__global__ __launch_bounds__(256) void hn_distortion_fwd_kernel(const float* __restrict__ w, const float* __restrict__ z,
                                                                int n_rays, int S, HnDistRange r, float grad_scale,
                                                                float* per_ray, float* __restrict__ loss_out,
                                                                unsigned* ticket, float* __restrict__ d_w) {
  __shared__ float sh[8];      // [0, 4) hn_block_sum's wave sums, [4] "this block arrived last"
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray < n_rays) {
    const size_t row = (size_t)ray * S;
    const float l = hn_distortion_ray<GRAD>(w + row, z + row, S, r, grad_scale / (float)n_rays,
                                            GRAD ? d_w + row : nullptr, lane);
    // published to whichever block arrives last, on any XCD: a write-through store, drained by the storing wave
    if (lane == 0) __hip_atomic_store(per_ray + ray, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  if (loss_out == nullptr) return;      // reduction 'none' (uniform over the grid)
  __syncthreads();
  if (threadIdx.x == 0) {
    // no release fence: the payload is write-through and drained by every storing wave ahead of the barrier, the ticket
    // an agent-scope atomic (a fence here writes back the XCD's whole L2, the gradient rows included: 1.8 us of the
    // launch's 9.7 at 1024 rays); the last arriver acquires before any wave of it reads a per-ray value
    const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh[4] = last ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (sh[4] == 0.0f) return;      // uniform over the block
  float s = 0.0f;
  for (int i = threadIdx.x; i < n_rays; i += 256)
    s += __hip_atomic_load(per_ray + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s = hn_block_sum<256>(s, sh);
  if (threadIdx.x == 0) {
    loss_out[0] = s / (float)n_rays;
    // every block has drawn its ticket: re-arm it for the next launch or replay
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// g_loss: ONE float (the mean's root gradient; the 1 / n_rays is applied here) or, per_ray_g, one per ray (no 1 / n_rays)
__global__ __launch_bounds__(256) void hn_distortion_bwd_kernel(const float* __restrict__ w, const float* __restrict__ z,
                                                                int n_rays, int S, HnDistRange r,
                                                                const float* __restrict__ g_loss, int per_ray_g,
                                                                float* __restrict__ d_w) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;
  const size_t row = (size_t)ray * S;
  const float gs = per_ray_g ? g_loss[ray] : g_loss[0] / (float)n_rays;
  hn_distortion_ray<true>(w + row, z + row, S, r, gs, d_w + row, lane);
}

// refused before any launch; fills the range
static int hn_dist_check(const float* w, const float* z, int n_rays, int n_samples, float near, float far, int spacing,
                         HnDistRange* r) {
  if (w == nullptr || z == nullptr) return -2;
  if (n_rays <= 0 || n_samples <= 0 || n_samples > 64 * HN_DIST_SEG) return -2;
  if (spacing != HN_SPACING_LINEAR && spacing != HN_SPACING_DISPARITY) return -2;
  if (!(far != near) || !(far - near == far - near)) return -2;      // equal, NaN or both infinite
  if (spacing == HN_SPACING_DISPARITY && !(near > 0.0f)) return -2;
  r->near = near;
  r->inv_range = (float)(1.0 / ((double)far - (double)near));      // rounded once
  r->far = far;
  r->disparity = spacing == HN_SPACING_DISPARITY;
  return 0;
}

extern "C" int hn_distortion_forward(const float* weights, const float* z, int n_rays, int n_samples, float near, float far,
                                     int spacing, float* per_ray, float* loss_out, uint32_t* ticket, hnStream_t stream) {
  HnDistRange r;
  if (hn_dist_check(weights, z, n_rays, n_samples, near, far, spacing, &r) != 0) return -2;
  if (per_ray == nullptr || (loss_out != nullptr && ticket == nullptr)) return -2;
  hipLaunchKernelGGL(hn_distortion_fwd_kernel<false>, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     weights, z, n_rays, n_samples, r, 1.0f, per_ray, loss_out, ticket, (float*)nullptr);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_distortion_forward_grad(const float* weights, const float* z, int n_rays, int n_samples, float near,
                                          float far, int spacing, float grad_scale, float* per_ray, float* loss_out,
                                          uint32_t* ticket, float* d_weights, hnStream_t stream) {
  HnDistRange r;
  if (hn_dist_check(weights, z, n_rays, n_samples, near, far, spacing, &r) != 0) return -2;
  if (per_ray == nullptr || loss_out == nullptr || ticket == nullptr || d_weights == nullptr) return -2;
  if (!(grad_scale == grad_scale)) return -2;
  hipLaunchKernelGGL(hn_distortion_fwd_kernel<true>, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     weights, z, n_rays, n_samples, r, grad_scale, per_ray, loss_out, ticket, d_weights);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_distortion_backward(const float* weights, const float* z, int n_rays, int n_samples, float near, float far,
                                      int spacing, const float* g_loss, int per_ray_g, float* d_weights,
                                      hnStream_t stream) {
  HnDistRange r;
  if (hn_dist_check(weights, z, n_rays, n_samples, near, far, spacing, &r) != 0) return -2;
  if (g_loss == nullptr || d_weights == nullptr) return -2;
  hipLaunchKernelGGL(hn_distortion_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     weights, z, n_rays, n_samples, r, g_loss, per_ray_g, d_weights);
  HN_CHECK_LAUNCH();
  return 0;
}
