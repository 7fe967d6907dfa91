// Fused optimizer steps over a flat parameter arena: Adam (torch.optim.Adam, utils.get_optimizer's default) and the other
// three optimizers of the reference's get_optimizer — SGD, RAdam and Ranger (utils/__init__.py:23-41; RAdam and Ranger
// from utils/optimizers.py:6-95 and :266-405).  All are built alike: a grid-stride pass of at most 256 blocks x 256
// threads over f32x4 vectors (scalar tail), the step counter on the device and advanced by the last block
// (hn_adam_ticket), the gradient cleared on the way out.
//
// For SGD, RAdam and Ranger the reference computes its schedule scalars (beta^t, N_sma, the step size and the products
// with lr) as Python doubles and hands them to fp32 tensor ops, which round them once.  Here thread 0 of every block does
// the same in fp64 from the device step counter and the fp64 hyper-parameter array, rounds each coefficient to fp32 once
// and passes them and the branch flags to the block through LDS.  (fp32 is not enough: for beta2 = 0.999 it puts N_sma at
// t = 6 at 6.0005 instead of 5.9942, and the first rectified step size 0.3 % off.)  The per-element arithmetic is the
// reference's fp32 tensor arithmetic, operation for operation.
#include "hn_common.h"
#include "hn_window.h"      // hn_wave_sum

// The launch grid of every *_step entry point: one block per CU, grid-stride: every thread pays the schedule arithmetic
// (Adam: two powf, an rsqrtf) once for ~6 vectors instead of once per vector (Adam, 2048 blocks: 26.3 us per launch at
// config 2, 512: 16.5, 256: 15.2)
static unsigned hn_step_blocks(long long n) {
  const long long blocks = (n / 4 + 255) / 256;
  return (unsigned)(blocks > 256 ? 256 : blocks < 1 ? 1 : blocks);
}

// ------------------------------------------------------------------------------------------------
// Fused Adam over a flat parameter arena (torch.optim.Adam semantics, utils.get_optimizer's default):
// one pass over p, g, m, v (28 B/parameter, HBM bound), the step counter lives on the device so the launch can be
// captured in a HIP graph, and the gradient is zeroed on the way out (saves the separate fill of the next step).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_adam_kernel(float* p, float* g, float* m, float* v, long long n,
                                                       const float* __restrict__ hyper, float* step,
                                                       int zero_grad) {
  // every block reads step[0] (hn_adam_consts) before it does anything else; the block that finishes LAST advances it
  const HnAdamConsts k = hn_adam_consts(hyper, step);
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<f32x4*>(g + i);
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        hn_adam_update(k, pe, gg[e], me, ve);
        pp[e] = pe; mm[e] = me; vv[e] = ve;
      }
      *reinterpret_cast<f32x4*>(p + i) = pp;
      *reinterpret_cast<f32x4*>(m + i) = mm;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      if (zero_grad) *reinterpret_cast<f32x4*>(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (long long j = i; j < n; ++j) {
        hn_adam_update(k, p[j], g[j], m[j], v[j]);
        if (zero_grad) g[j] = 0.f;
      }
    }
  }
  hn_adam_ticket(step, k.t);
}

extern "C" int hn_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                            const float* hyper_dev, float* step_dev, int zero_grad, hnStream_t stream) {
  if (n <= 0) return -2;
  if (params == nullptr || grads == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || step_dev == nullptr ||
      hyper_dev == nullptr)
    return -3;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return -4;
  hipLaunchKernelGGL(hn_adam_kernel, dim3(hn_step_blocks(n)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                     exp_avg_sq, n, hyper_dev, step_dev, zero_grad);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// SGD (torch.optim.SGD, which get_optimizer builds directly): d = g*gscale + wd*p; with momentum buf = d on update 1,
// buf = momentum*buf + (1-dampening)*d after that; d = d + momentum*buf (Nesterov) or buf; p += (-lr)*d.
// ------------------------------------------------------------------------------------------------
struct HnSgdCoef {
  float gscale, wd, momentum, one_m_damp, neg_lr, t;
  int use_buf, first, nesterov;
};

HN_DEV void hn_sgd_update(const HnSgdCoef& c, float& p, float g, float* buf) {
  float d = g * c.gscale;
  d = d + c.wd * p;
  if (c.use_buf) {
    float b = c.first ? d : *buf * c.momentum + c.one_m_damp * d;
    *buf = b;
    d = c.nesterov ? d + c.momentum * b : b;
  }
  p = p + c.neg_lr * d;
}

__global__ __launch_bounds__(256) void hn_sgd_kernel(float* p, float* g, float* buf, long long n,
                                                      const double* __restrict__ hyper, float* step, int zero_grad) {
  __shared__ HnSgdCoef sc;
  if (threadIdx.x == 0) {
    // every block reads step[0] here, before its ticket; the block that finishes LAST advances it
    const double lr = hyper[0], momentum = hyper[1], dampening = hyper[2], wd = hyper[3];
    HnSgdCoef c;
    c.t = step[0] + 1.0f;
    c.gscale = (float)hyper[5];
    c.wd = (float)wd;
    c.momentum = (float)momentum;
    c.one_m_damp = (float)(1.0 - dampening);
    c.neg_lr = (float)(-lr);
    c.use_buf = (momentum != 0.0 && buf != nullptr) ? 1 : 0;
    c.first = c.t == 1.0f;
    c.nesterov = hyper[4] != 0.0;
    sc = c;
  }
  __syncthreads();
  const HnSgdCoef k = sc;
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<f32x4*>(g + i);
      if (k.use_buf) {
        f32x4 bb = k.first ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<f32x4*>(buf + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], be = bb[e];
          hn_sgd_update(k, pe, gg[e], &be);
          pp[e] = pe; bb[e] = be;
        }
        *reinterpret_cast<f32x4*>(buf + i) = bb;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e];
          hn_sgd_update(k, pe, gg[e], nullptr);
          pp[e] = pe;
        }
      }
      *reinterpret_cast<f32x4*>(p + i) = pp;
      if (zero_grad) *reinterpret_cast<f32x4*>(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (long long j = i; j < n; ++j) {
        hn_sgd_update(k, p[j], g[j], k.use_buf ? buf + j : nullptr);
        if (zero_grad) g[j] = 0.f;
      }
    }
  }
  hn_adam_ticket(step, k.t);
}

extern "C" int hn_sgd_step(float* params, float* grads, float* momentum_buf, long long n, const double* hyper_dev,
                           float* step_dev, int zero_grad, hnStream_t stream) {
  if (n <= 0) return -2;
  if (params == nullptr || grads == nullptr || hyper_dev == nullptr || step_dev == nullptr) return -3;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) != 0 || ((uintptr_t)hyper_dev & 7) != 0 ||
      ((uintptr_t)step_dev & 3) != 0)
    return -4;
  hipLaunchKernelGGL(hn_sgd_kernel, dim3(hn_step_blocks(n)), dim3(256), 0, (hipStream_t)stream, params, grads,
                     momentum_buf, n, hyper_dev, step_dev, zero_grad);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// RAdam (utils/optimizers.py:29-95) and Ranger = RAdam + lookahead (:322-405).  Per element, in the reference's order:
//   v = v*b2 + ((1-b2)*g)*g;  m = m*b1 + (1-b1)*g
//   weight decay (RAdam: only when an update happens; Ranger: always):  p = p + (-wd*lr)*p
//   rectified (RAdam N_sma >= 5, Ranger N_sma > threshold):  p = p + ((-step_size*lr)*m) / (sqrt(v) + eps)
//   otherwise (degenerated to SGD):                          p = p + (-step_size*lr)*m
//   RAdam with degenerated_to_sgd = False below the threshold: no update at all.
//   Ranger: slow = p before update 1; after every update t with t % k == 0: slow = slow + alpha*(p - slow), p = slow.
// ------------------------------------------------------------------------------------------------
struct HnRadamCoef {
  float gscale, b1, b2, one_m_b1, one_m_b2, eps, neg_step_lr, neg_wd_lr, alpha, t;
  int rect, update, decay, first, sync;
};

HN_DEV void hn_radam_update(const HnRadamCoef& c, float& p, float g, float& m, float& v) {
  g = g * c.gscale;
  v = v * c.b2 + c.one_m_b2 * g * g;
  m = m * c.b1 + c.one_m_b1 * g;
  if (c.decay) p = p + c.neg_wd_lr * p;
  if (c.rect) {
    const float denom = sqrtf(v) + c.eps;
    p = p + c.neg_step_lr * m / denom;
  } else if (c.update) {
    p = p + c.neg_step_lr * m;
  }
}

template <bool RANGER>
__global__ __launch_bounds__(256) void hn_radam_kernel(float* p, float* g, float* m, float* v, float* slow, long long n,
                                                        int k_la, const double* __restrict__ hyper, float* step,
                                                        int zero_grad) {
  __shared__ HnRadamCoef sc;
  if (threadIdx.x == 0) {
    const double lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], wd = hyper[4];
    HnRadamCoef c;
    c.t = step[0] + 1.0f;
    const double t = (double)c.t;
    const double beta2_t = pow(beta2, t);
    const double n_sma_max = 2.0 / (1.0 - beta2) - 1.0;
    const double n_sma = n_sma_max - 2.0 * t * beta2_t / (1.0 - beta2_t);
    const bool rect = RANGER ? n_sma > hyper[6] : n_sma >= 5.0;
    double step_size;
    if (rect)
      step_size = sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_sma_max - 4.0) * (n_sma - 2.0) / n_sma * n_sma_max /
                       (n_sma_max - 2.0)) /
                  (1.0 - pow(beta1, t));
    else if (RANGER || hyper[7] != 0.0)
      step_size = 1.0 / (1.0 - pow(beta1, t));
    else
      step_size = -1.0;
    c.rect = rect;
    c.update = rect || step_size > 0.0;
    c.decay = wd != 0.0 && (RANGER || c.update);
    c.gscale = (float)hyper[5];
    c.b1 = (float)beta1;
    c.b2 = (float)beta2;
    c.one_m_b1 = (float)(1.0 - beta1);
    c.one_m_b2 = (float)(1.0 - beta2);
    c.eps = (float)hyper[3];
    c.neg_step_lr = (float)(-step_size * lr);
    c.neg_wd_lr = (float)(-wd * lr);
    c.alpha = (float)hyper[8];
    c.first = RANGER && c.t == 1.0f;
    c.sync = RANGER && ((long long)c.t % (long long)k_la) == 0;
    sc = c;
  }
  __syncthreads();
  const HnRadamCoef k = sc;
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<f32x4*>(g + i);
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
      // update 1 and lookahead updates only (uniform across the grid): the slow buffer
      f32x4 ss = f32x4{0.f, 0.f, 0.f, 0.f};
      if (RANGER && (k.first || k.sync)) ss = k.first ? pp : *reinterpret_cast<f32x4*>(slow + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        hn_radam_update(k, pe, gg[e], me, ve);
        if (RANGER && k.sync) {
          ss[e] = ss[e] + k.alpha * (pe - ss[e]);
          pe = ss[e];
        }
        pp[e] = pe; mm[e] = me; vv[e] = ve;
      }
      *reinterpret_cast<f32x4*>(p + i) = pp;
      *reinterpret_cast<f32x4*>(m + i) = mm;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      if (RANGER && (k.first || k.sync)) *reinterpret_cast<f32x4*>(slow + i) = ss;
      if (zero_grad) *reinterpret_cast<f32x4*>(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (long long j = i; j < n; ++j) {
        float s = 0.f;
        if (RANGER && (k.first || k.sync)) s = k.first ? p[j] : slow[j];
        float pj = p[j];
        hn_radam_update(k, pj, g[j], m[j], v[j]);
        if (RANGER && k.sync) {
          s = s + k.alpha * (pj - s);
          pj = s;
        }
        p[j] = pj;
        if (RANGER && (k.first || k.sync)) slow[j] = s;
        if (zero_grad) g[j] = 0.f;
      }
    }
  }
  hn_adam_ticket(step, k.t);
}

extern "C" int hn_radam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* slow, long long n,
                             int k, const double* hyper_dev, float* step_dev, int zero_grad, hnStream_t stream) {
  if (n <= 0 || k < 1) return -2;
  if (params == nullptr || grads == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || hyper_dev == nullptr ||
      step_dev == nullptr)
    return -3;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)slow) & 15) != 0 ||
      ((uintptr_t)hyper_dev & 7) != 0 || ((uintptr_t)step_dev & 3) != 0)
    return -4;
  if (slow != nullptr)
    hipLaunchKernelGGL(hn_radam_kernel<true>, dim3(hn_step_blocks(n)), dim3(256), 0, (hipStream_t)stream, params, grads,
                       exp_avg, exp_avg_sq, slow, n, k, hyper_dev, step_dev, zero_grad);
  else
    hipLaunchKernelGGL(hn_radam_kernel<false>, dim3(hn_step_blocks(n)), dim3(256), 0, (hipStream_t)stream, params, grads,
                       exp_avg, exp_avg_sq, slow, n, k, hyper_dev, step_dev, zero_grad);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Gradient clipping over the flat gradient buffer, ahead of any *_step launch: torch.nn.utils.clip_grad_value_ and then
// clip_grad_norm_ (norm_type 2, error_if_nonfinite False) of the gradient that counts, s*g (s = grad_scale, which the
// step kernels apply themselves later).  clamp(s*g, +-v) = s*clamp(g, +-v/s), so both kernels work on the raw buffer with
// the threshold v' = fp32(v/s):  total_norm = s*sqrt(sum clamp(g, +-v')^2),  coef = min(max_norm / (total_norm + 1e-6), 1)
// (a NaN stays NaN, as torch.clamp(max=1.0) leaves it),  g <- clamp(g, +-v') * coef.
// Two launches on the step kernels' grid.  hn_grad_norm: per-thread fp32 sums of squares, a wave64 butterfly, the four
// wave sums added in order, ONE partial per block; the block that arrives LAST adds the partials in index order in fp64
// and publishes [total_norm, coef].  No float atomics: the same input gives the same bits on every run and replay.
// hn_grad_scale: every block reads coef and returns at once when nothing can change (coef == 1, no value clip).
// ------------------------------------------------------------------------------------------------
// written with comparisons: a NaN gradient stays NaN as in torch (fminf / fmaxf would drop it); v = +inf changes nothing
HN_DEV float hn_clip_value(float g, float v) { return g > v ? v : (g < -v ? -v : g); }

#define HN_CLIP_PARTIALS 256      // floats of `work` ahead of the ticket word: the largest grid of hn_step_blocks

__global__ __launch_bounds__(256) void hn_grad_norm_kernel(const float* g, long long n, float vp, float gscale,
                                                            float max_norm, float* work, float* out) {
  // ONE LDS array: [0, 256) the partials for the last block, [256, 260) the wave sums, [260] "this block arrived last"
  __shared__ float sh[HN_CLIP_PARTIALS + 8];
  float s = 0.0f;
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  // four grid strides per trip, their loads issued together (one load per trip leaves the pass latency bound); the terms
  // are still added in the order of a one-stride loop
  for (long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i0 < n; i0 += 4 * stride) {
    f32x4 gg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * stride;
      gg[u] = i + 4 <= n ? *reinterpret_cast<const f32x4*>(g + i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * stride;
      if (i + 4 <= n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float c = hn_clip_value(gg[u][e], vp);
          s += c * c;
        }
      } else {
        for (long long j = i; j < n; ++j) {      // the scalar tail: at most three elements, one thread of the grid
          const float c = hn_clip_value(g[j], vp);
          s += c * c;
        }
      }
    }
  }
  s = hn_wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[HN_CLIP_PARTIALS + (threadIdx.x >> 6)] = s;
  __syncthreads();
  unsigned* ticket = reinterpret_cast<unsigned*>(work + HN_CLIP_PARTIALS);
  if (threadIdx.x == 0) {
    const float part = ((sh[HN_CLIP_PARTIALS] + sh[HN_CLIP_PARTIALS + 1]) + sh[HN_CLIP_PARTIALS + 2]) +
                       sh[HN_CLIP_PARTIALS + 3];
    // publish the partial to whichever block arrives last, on any XCD: the store (write-through), drained, an
    // agent-scope release, drained again, THEN the ticket; the last arriver acquires at agent scope before any block of
    // it reads a partial
    __hip_atomic_store(work + blockIdx.x, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh[HN_CLIP_PARTIALS + 4] = last ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (sh[HN_CLIP_PARTIALS + 4] == 0.0f) return;      // uniform over the block
  sh[threadIdx.x] = threadIdx.x < gridDim.x
                        ? __hip_atomic_load(work + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                        : 0.0f;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) acc += (double)sh[b];
    const float total = (float)((double)gscale * sqrt(acc));
    const float coef = (float)((double)max_norm / ((double)total + 1e-6));
    out[0] = total;
    out[1] = coef > 1.0f ? 1.0f : coef;      // NaN > 1 is false: a NaN stays NaN
    // every block has drawn its ticket: re-arm it for the next launch or replay
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void hn_grad_scale_kernel(float* g, long long n, float vp, int value_clip,
                                                             const float* out) {
  const float coef = out != nullptr ? out[1] : 1.0f;
  if (coef == 1.0f && !value_clip) return;      // the common case; bit-identical to multiplying by 1
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i0 < n; i0 += 4 * stride) {
    f32x4 gg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {      // as hn_grad_norm_kernel: the loads of four grid strides in flight together
      const long long i = i0 + u * stride;
      if (i + 4 <= n) gg[u] = *reinterpret_cast<f32x4*>(g + i);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * stride;
      if (i + 4 <= n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) gg[u][e] = hn_clip_value(gg[u][e], vp) * coef;
        *reinterpret_cast<f32x4*>(g + i) = gg[u];
      } else {
        for (long long j = i; j < n; ++j) g[j] = hn_clip_value(g[j], vp) * coef;
      }
    }
  }
}

// refused before any launch: -2 n <= 0, or a grad_scale / clip_value / max_norm that is not positive (NaN included)
static int hn_clip_check(long long n, float grad_scale, float clip_value, float max_norm) {
  return (n <= 0 || !(grad_scale > 0.0f) || !(clip_value > 0.0f) || !(max_norm > 0.0f)) ? -2 : 0;
}
// v' = fp32(v / s), the division in double (+inf stays +inf: no value clip)
static float hn_clip_threshold(float clip_value, float grad_scale) {
  return (float)((double)clip_value / (double)grad_scale);
}

extern "C" int hn_grad_norm(const float* grad, long long n, float grad_scale, float clip_value, float max_norm,
                            float* work, float* out, hnStream_t stream) {
  if (hn_clip_check(n, grad_scale, clip_value, max_norm) != 0) return -2;
  if (grad == nullptr || work == nullptr || out == nullptr) return -3;
  if ((((uintptr_t)grad | (uintptr_t)work) & 15) != 0 || ((uintptr_t)out & 3) != 0) return -4;
  hipLaunchKernelGGL(hn_grad_norm_kernel, dim3(hn_step_blocks(n)), dim3(256), 0, (hipStream_t)stream, grad, n,
                     hn_clip_threshold(clip_value, grad_scale), grad_scale, max_norm, work, out);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_grad_scale(float* grad, long long n, float grad_scale, float clip_value, const float* out,
                             hnStream_t stream) {
  if (hn_clip_check(n, grad_scale, clip_value, 1.0f) != 0) return -2;
  if (grad == nullptr) return -3;
  if (((uintptr_t)grad & 15) != 0 || ((uintptr_t)out & 3) != 0) return -4;
  hipLaunchKernelGGL(hn_grad_scale_kernel, dim3(hn_step_blocks(n)), dim3(256), 0, (hipStream_t)stream, grad, n,
                     hn_clip_threshold(clip_value, grad_scale), (int)!(clip_value == INFINITY), out);
  HN_CHECK_LAUNCH();
  return 0;
}
