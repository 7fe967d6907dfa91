// SSIM of the reference's metrics.py:15-20 (kornia's ssim loss, its `dssim`): forward, deterministic sum, backward.
//
// One workgroup of 256 threads per 32 x 16 output tile of one (n, c) plane.  The inputs are staged with their halo in
// LDS, reflect indexing resolved at load time (kornia's filter2d pads with F.pad(mode='reflect')), so every later read
// is an LDS read without a branch on the border.  The 2-D Gaussian window is the outer product of the 1-D weights the
// host passes by value (kornia's get_gaussian_kernel1d, computed by torch), applied as a horizontal pass over LDS and a
// vertical pass into registers; the five moments (x, y, x^2, y^2, xy) share both passes.  The SSIM arithmetic is
// kornia's tensor arithmetic, operation for operation (the library builds with -ffp-contract=off).
//
// The sum over all elements takes no float atomics: every workgroup writes its partial (summed in a fixed order) to
// the workspace and a second launch of one workgroup sums the partials in a fixed order, so the result is the same
// bits run to run.
//
// The backward is the adjoint of the forward, reflect padding included.  Per output pixel q of the map the upstream
// gradient times d dssim/dS gives four maps, A = g dS/dmux - 2 mux g dS/dsxx - muy g dS/dsxy (A' with x and y
// swapped), B = g dS/dsxx (= g dS/dsyy) and C = g dS/dsxy; the gradient at pixel p is the correlation of these with
// the transposed window, where a tap that the forward read from a mirrored coordinate t (refl(t) = p) adds its share
// to p: d/dx = A^ + 2 x B^ + y C^, d/dy = A'^ + 2 y B^ + x C^.  Every tap that reaches p comes from a map pixel within
// the window radius of p (reflection only brings coordinates closer), so a tile needs the maps on its tile + R halo
// and the inputs on tile + 2R.
//
// The tile, the image pair, the two passes and the sums are hn_window.h's, shared with hn_msssim.hip.
#include "hn_window.h"

struct HnSsimWin {
  float w[2 * HN_SSIM_MAX_R + 1];
};

struct HnSsimShape : HnWinPair {
  float eps;
};

// reflect padding's source coordinate for t in [-(n-1), 2(n-1)] (F.pad mode='reflect': the edge is not repeated),
// clamped into the image so that tiles reaching past the bottom / right edge stay in bounds (those lanes feed no output)
HN_DEV int hn_reflect(int t, int n) {
  t = t < 0 ? -t : t;
  t = t >= n ? 2 * (n - 1) - t : t;
  return t < 0 ? 0 : (t >= n ? n - 1 : t);
}

HN_DEV float hn_ld(const float* p, const long long* s, int n, int c, int yy, int xx) {
  return p[n * s[0] + c * s[1] + yy * s[2] + xx * s[3]];
}

// kornia 0.6.1 metrics.ssim for one pixel from its five filtered moments
struct HnSsimPix {
  float mu1, mu2, mu1_sq, mu2_sq, mu1_mu2, s1, s2, s12, n1, n2, d1, d2, den, s;
};

HN_DEV HnSsimPix hn_ssim_pix(const float m[5], float c1, float c2, float eps) {
  HnSsimPix p;
  p.mu1 = m[0];
  p.mu2 = m[1];
  p.mu1_sq = p.mu1 * p.mu1;
  p.mu2_sq = p.mu2 * p.mu2;
  p.mu1_mu2 = p.mu1 * p.mu2;
  p.s1 = m[2] - p.mu1_sq;
  p.s2 = m[3] - p.mu2_sq;
  p.s12 = m[4] - p.mu1_mu2;
  p.n1 = 2.0f * p.mu1_mu2 + c1;
  p.n2 = 2.0f * p.s12 + c2;
  p.d1 = p.mu1_sq + p.mu2_sq + c1;
  p.d2 = p.s1 + p.s2 + c2;
  p.den = p.d1 * p.d2 + eps;
  p.s = (p.n1 * p.n2) / p.den;
  return p;
}

// (1 - S) / 2 clamped to [0, 1]
HN_DEV float hn_dssim(float s) { return fminf(fmaxf((1.0f - s) / 2.0f, 0.0f), 1.0f); }

// Stage x and y of rows [y0 - HALO, y0 + TH + HALO) x cols [x0 - HALO, x0 + TW + HALO) with reflect indexing.  With
// `zero_far`, coordinates beyond the reflect range [-R, n-1+R] load 0 (they only feed map pixels outside the image).
template <int R, int HALO>
HN_DEV void hn_ssim_stage(const HnSsimShape& a, const HnWinTile& t, float* sx, float* sy, bool zero_far) {
  constexpr int SW = HN_WIN_TW + 2 * HALO, SH = HN_WIN_TH + 2 * HALO;
  for (int i = threadIdx.x; i < SH * SW; i += HN_WIN_THREADS) {
    const int gy = t.y0 - HALO + i / SW, gx = t.x0 - HALO + i % SW;
    float vx = 0.0f, vy = 0.0f;
    if (!zero_far || (gy >= -R && gy <= a.h - 1 + R && gx >= -R && gx <= a.w - 1 + R)) {
      const int ry = hn_reflect(gy, a.h), rx = hn_reflect(gx, a.w);
      vx = hn_ld(a.x, a.xs, t.n, t.c, ry, rx);
      vy = hn_ld(a.y, a.ys, t.n, t.c, ry, rx);
    }
    sx[i] = vx;
    sy[i] = vy;
  }
}

template <int R>
__global__ __launch_bounds__(HN_WIN_THREADS) void hn_ssim_forward_kernel(HnSsimShape a, HnSsimWin win, float* map,
                                                                           float* partials) {
  constexpr int SW = HN_WIN_TW + 2 * R, SH = HN_WIN_TH + 2 * R;
  __shared__ float sx[SH * SW], sy[SH * SW];
  __shared__ float hm[5 * SH * HN_WIN_TW];
  __shared__ float red[HN_WIN_THREADS / 64];
  const HnWinTile t = hn_win_tile(a);
  hn_ssim_stage<R, R>(a, t, sx, sy, false);
  __syncthreads();
  hn_win_row_pass<2 * R + 1>(win.w, 0, sx, sy, SW, hm, SH, HN_WIN_TW, SH * HN_WIN_TW);
  __syncthreads();
  const int col = threadIdx.x % HN_WIN_TW, gx = t.x0 + col;
  float acc = 0.0f;
  for (int row = threadIdx.x / HN_WIN_TW; row < HN_WIN_TH; row += HN_WIN_THREADS / HN_WIN_TW) {
    const int gy = t.y0 + row;
    if (gy >= a.h || gx >= a.w) continue;
    float m[5];
    hn_win_col_pass<2 * R + 1>(win.w, 0, hm, HN_WIN_TW, SH * HN_WIN_TW, row, col, m);
    const float l = hn_dssim(hn_ssim_pix(m, a.c1, a.c2, a.eps).s);
    if (map != nullptr) map[((long long)t.plane * a.h + gy) * a.w + gx] = l;
    acc += l;
  }
  if (partials != nullptr) {
    const float s = hn_block_sum<HN_WIN_THREADS>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(HN_WIN_THREADS) void hn_ssim_sum_kernel(const float* partials, int n, float* out) {
  __shared__ float red[HN_WIN_THREADS / 64];
  float v = 0.0f;
  for (int i = threadIdx.x; i < n; i += HN_WIN_THREADS) v += partials[i];
  const float s = hn_block_sum<HN_WIN_THREADS>(v, red);
  if (threadIdx.x == 0) out[0] = s;
}

// sum over the source coordinates t with refl(t) = p, of sum_{j=-R..R} w[R+j] * g(t - j) (g = 0 outside [0, n)):
// `at(q)` reads the map at image coordinate q
template <int R, typename F>
HN_DEV float hn_ssim_adjoint(const HnSsimWin& win, int p, int n, F at) {
  float acc = 0.0f;
  int ts[3];
  int nt = 0;
  ts[nt++] = p;
  if (p >= 1 && p <= R) ts[nt++] = -p;                            // left / top mirror
  if (p <= n - 2 && p >= n - 1 - R) ts[nt++] = 2 * (n - 1) - p;    // right / bottom mirror
  for (int i = 0; i < nt; ++i) {
    const int tt = ts[i];
    float s = 0.0f;
#pragma unroll
    for (int j = -R; j <= R; ++j) {
      const int q = tt - j;
      if (q >= 0 && q < n) s += win.w[R + j] * at(q);
    }
    acc += s;
  }
  return acc;
}

template <int R>
__global__ __launch_bounds__(HN_WIN_THREADS) void hn_ssim_backward_kernel(HnSsimShape a, HnSsimWin win,
                                                                            const float* g_scalar, const float* g_map,
                                                                            float* d_x, float* d_y) {
  constexpr int SW = HN_WIN_TW + 4 * R, SH = HN_WIN_TH + 4 * R;    // inputs: tile + 2R
  constexpr int GW = HN_WIN_TW + 2 * R, GH = HN_WIN_TH + 2 * R;    // maps: tile + R
  constexpr int HM = 5 * SH * GW, HA = 4 * GH * HN_WIN_TW;
  __shared__ float sx[SH * SW], sy[SH * SW];
  __shared__ float hm[HM > HA ? HM : HA];    // horizontal moments, then the horizontal adjoint of the four maps
  __shared__ float gm[4 * GH * GW];          // A, A', B, C
  const HnWinTile t = hn_win_tile(a);
  hn_ssim_stage<R, 2 * R>(a, t, sx, sy, true);
  __syncthreads();
  hn_win_row_pass<2 * R + 1>(win.w, 0, sx, sy, SW, hm, SH, GW, SH * GW);
  __syncthreads();
  const float gs = g_scalar != nullptr ? g_scalar[0] : 0.0f;
  for (int i = threadIdx.x; i < GH * GW; i += HN_WIN_THREADS) {
    const int row = i / GW, col = i % GW;
    const int qy = t.y0 - R + row, qx = t.x0 - R + col;
    float ga = 0.0f, gb = 0.0f, gbb = 0.0f, gc = 0.0f;
    if (qy >= 0 && qy < a.h && qx >= 0 && qx < a.w) {
      float m[5];
      hn_win_col_pass<2 * R + 1>(win.w, 0, hm, GW, SH * GW, row, col, m);
      const HnSsimPix p = hn_ssim_pix(m, a.c1, a.c2, a.eps);
      const float l = (1.0f - p.s) / 2.0f;
      const float up = g_map != nullptr ? g_map[((long long)t.plane * a.h + qy) * a.w + qx] : gs;
      const float g = (l >= 0.0f && l <= 1.0f) ? up * -0.5f : 0.0f;          // torch.clamp passes its bounds
      // S = n1 n2 / (d1 d2 + eps)
      const float inv = 1.0f / p.den;
      const float dmu1 = (2.0f * p.mu2 * p.n2 - p.s * 2.0f * p.mu1 * p.d2) * inv;
      const float dmu2 = (2.0f * p.mu1 * p.n2 - p.s * 2.0f * p.mu2 * p.d2) * inv;
      const float dsig = -p.s * p.d1 * inv;             // dS/dsxx = dS/dsyy
      const float dcov = 2.0f * p.n1 * inv;             // dS/dsxy
      gb = g * dsig;
      gc = g * dcov;
      ga = g * dmu1 - 2.0f * p.mu1 * gb - p.mu2 * gc;
      gbb = g * dmu2 - 2.0f * p.mu2 * gb - p.mu1 * gc;
    }
    gm[i] = ga;
    gm[GH * GW + i] = gbb;
    gm[2 * GH * GW + i] = gb;
    gm[3 * GH * GW + i] = gc;
  }
  __syncthreads();
  // horizontal adjoint: rows of the map region, the tile's columns
  for (int i = threadIdx.x; i < GH * HN_WIN_TW; i += HN_WIN_THREADS) {
    const int row = i / HN_WIN_TW, col = i % HN_WIN_TW, gx = t.x0 + col;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (gx < a.w) {
      const int base = t.x0 - R;      // image column of map col 0; |q - gx| <= R for every tap that is read
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* g = gm + k * GH * GW + row * GW;
        v[k] = hn_ssim_adjoint<R>(win, gx, a.w, [&](int q) { return g[q - base]; });
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) hm[k * GH * HN_WIN_TW + i] = v[k];
  }
  __syncthreads();
  // vertical adjoint and the products with the inputs
  const int col = threadIdx.x % HN_WIN_TW, gx = t.x0 + col;
  for (int row = threadIdx.x / HN_WIN_TW; row < HN_WIN_TH; row += HN_WIN_THREADS / HN_WIN_TW) {
    const int gy = t.y0 + row;
    if (gy >= a.h || gx >= a.w) continue;
    const int base = t.y0 - R;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* h = hm + k * GH * HN_WIN_TW + col;
      v[k] = hn_ssim_adjoint<R>(win, gy, a.h, [&](int q) { return h[(q - base) * HN_WIN_TW]; });
    }
    const int s = (row + 2 * R) * SW + col + 2 * R;
    const float xv = sx[s], yv = sy[s];
    const long long o = ((long long)t.plane * a.h + gy) * a.w + gx;
    d_x[o] = v[0] + 2.0f * xv * v[2] + yv * v[3];
    if (d_y != nullptr) d_y[o] = v[1] + 2.0f * yv * v[2] + xv * v[3];
  }
}

// the window and shape checks of every entry point: the launch's workgroups, or 0 for arguments that are refused
static long long hn_ssim_blocks(int n, int c, int h, int w, int window) {
  if (window < 3 || window > 2 * HN_SSIM_MAX_R + 1 || (window & 1) == 0) return 0;
  if (h <= window / 2 || w <= window / 2) return 0;      // reflect padding needs more than the radius
  return hn_win_blocks(n, c, h, w);
}

static int hn_ssim_setup(const float* x, const int64_t* xs, const float* y, const int64_t* ys, int n, int c, int h, int w,
                         const float* window_host, int window, float c1, float c2, float eps, HnSsimShape* a,
                         HnSsimWin* win, long long* blocks) {
  *blocks = hn_ssim_blocks(n, c, h, w, window);
  if (*blocks == 0) return -2;
  if (x == nullptr || y == nullptr || xs == nullptr || ys == nullptr || window_host == nullptr) return -3;
  hn_win_pair(a, x, xs, y, ys, c, h, w);
  a->c1 = c1;
  a->c2 = c2;
  a->eps = eps;
  for (int i = 0; i < 2 * HN_SSIM_MAX_R + 1; ++i) win->w[i] = i < window ? window_host[i] : 0.0f;
  return 0;
}

extern "C" int hn_ssim_workspace_bytes(int n, int c, int h, int w, int window, int64_t* bytes) {
  if (bytes == nullptr) return -3;
  const long long blocks = hn_ssim_blocks(n, c, h, w, window);
  if (blocks == 0) return -2;
  *bytes = (blocks * 4 + 15) / 16 * 16;
  return 0;
}

#define HN_SSIM_DISPATCH(KERNEL, ...)                                                                                \
  switch (window / 2) {                                                                                              \
    case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                                                       \
    case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                                                       \
    case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                                                       \
    case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                                                       \
    case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                                                       \
    case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                                                       \
    default: hipLaunchKernelGGL(KERNEL<7>, __VA_ARGS__); break;                                                      \
  }

extern "C" int hn_ssim_forward(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides,
                               int n, int c, int h, int w, const float* window_host, int window, float c1, float c2,
                               float eps, float* dssim_map, float* sum_out, void* workspace, hnStream_t stream) {
  HnSsimShape a;
  HnSsimWin win;
  long long blocks = 0;
  const int rc = hn_ssim_setup(pred, pred_strides, gt, gt_strides, n, c, h, w, window_host, window, c1, c2, eps, &a,
                               &win, &blocks);
  if (rc != 0) return rc;
  if (dssim_map == nullptr && sum_out == nullptr) return -3;
  if (sum_out != nullptr && workspace == nullptr) return -3;
  float* partials = sum_out != nullptr ? static_cast<float*>(workspace) : nullptr;
  HN_SSIM_DISPATCH(hn_ssim_forward_kernel, dim3((unsigned)blocks), dim3(HN_WIN_THREADS), 0, (hipStream_t)stream, a, win,
                   dssim_map, partials)
  HN_CHECK_LAUNCH();
  if (sum_out != nullptr) {
    hipLaunchKernelGGL(hn_ssim_sum_kernel, dim3(1), dim3(HN_WIN_THREADS), 0, (hipStream_t)stream, partials, (int)blocks,
                       sum_out);
    HN_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int hn_ssim_backward(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides,
                                int n, int c, int h, int w, const float* window_host, int window, float c1, float c2,
                                float eps, const float* g_scalar, const float* g_map, float* d_pred, float* d_gt,
                                hnStream_t stream) {
  HnSsimShape a;
  HnSsimWin win;
  long long blocks = 0;
  const int rc = hn_ssim_setup(pred, pred_strides, gt, gt_strides, n, c, h, w, window_host, window, c1, c2, eps, &a,
                               &win, &blocks);
  if (rc != 0) return rc;
  if (d_pred == nullptr || (g_scalar == nullptr) == (g_map == nullptr)) return -3;
  HN_SSIM_DISPATCH(hn_ssim_backward_kernel, dim3((unsigned)blocks), dim3(HN_WIN_THREADS), 0, (hipStream_t)stream, a,
                   win, g_scalar, g_map, d_pred, d_gt)
  HN_CHECK_LAUNCH();
  return 0;
}
