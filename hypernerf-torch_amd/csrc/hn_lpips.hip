// LPIPS v0.1 (Zhang et al. 2018; the `lpips` package with normalize=True, spatial=False, eval mode): the pieces of the
// frozen AlexNet / VGG16 backbones and of the distance head, in exact fp32.  The layer tables live on the host
// (ops/lpips/, lpips_net), which calls one entry point per layer; DESIGN.md 3.14 holds the definition.
//
//   hn_lpips_prepare    both images of every pair into one (2n, 3, h, w) batch, scaled: images [0, n) are pred, [n, 2n) gt
//   hn_lpips_conv       convolution + bias (+ ReLU) as an implicit GEMM on v_mfma_f32_32x32x2_f32
//   hn_lpips_maxpool    floor-mode max pool without padding
//   hn_lpips_distance   one tap's term of the metric: unit-normalise over channels, weighted squared difference, pixel mean
//
// The convolution: M = output channels, N = output pixels of the whole batch, K = cin * kh * kw in torch's weight order
// (ci, ky, kx).  A workgroup owns a BM x BN output tile and walks K in steps of BK: the weight tile comes from the
// packed, transposed, zero-padded weights wt[Kpad][Mpad] (coalesced along M), the activation tile is gathered (im2col
// on the fly: the k-th row's (ci, ky, kx) comes from a table the host built with the weights, a tap outside the image
// contributes 0); both go through registers into LDS while the matrix core works on the previous step, and the table
// rows of a step are turned into element offsets once per workgroup, a step ahead of their use.  Every
// wave owns TM x TN accumulator tiles of 32 x 32.  An output element is ONE accumulator that takes its K products in
// ascending k, two per instruction: a k-ordered fmaf chain from 0, then + bias, then max(., 0).  The chain does not
// depend on the tile shape, on the position in the batch or on the other image (padded k rows have zero weights AND
// zero activations: fma(0, 0, acc) = acc), so the results are the same bits run to run, for any batch split and any of
// the three tile shapes.  There is no split-K and no atomic.
//
// Tile shapes:  128 x 128 by 4 waves (2 x 2 waves of 2 x 2 tiles) with BK = 16,  64 x 64 by 4 waves and 32 x 64 by 2 waves
// with BK = 64.  The host picks the largest whose grid fills the 256 CUs (and no 128-row tile for 64 output channels,
// which would multiply zeros in half of its rows): alex conv3-5 at 378 x 504 have only 1320 pixels and run the smallest.
// A small layer has too few workgroups to hide anything behind one another: its time is one workgroup's walk over K,
// hence the long steps of the small tiles (DESIGN.md 3.14 has the measured times and what is not explained in them).
#include "hn_common.h"

#define HN_LPIPS_BK 64            /* Kpad is a multiple of it: the longest K step of the convolution's tile shapes */
#define HN_LPIPS_MPAD 128         /* Mpad (packed output channels) is a multiple of it */
#define HN_LPIPS_MAX_KERNEL 15    /* kernel sides 1 .. 15: ky, kx take 4 bits each in the k table */
#define HN_LPIPS_MAX_CHANNELS 4096
#define HN_LPIPS_ALEX_MIN_SIDE 31
#define HN_LPIPS_VGG_MIN_SIDE 16
#define HN_LPIPS_LAYERS 5
#define HN_LPIPS_DIST_PIXELS 64   /* pixels per workgroup of the distance launch: one partial sum each */
#define HN_LPIPS_DIST_GROUPS 16   /* channel groups of that workgroup (group g owns the channels = g mod 16) */
#define HN_LPIPS_SUM_THREADS 256
#define HN_LPIPS_FILL_BLOCKS 256  /* a tile shape is taken when its grid has at least this many workgroups */

static const long long HN_LPIPS_MAX_ELEMS = 2147483647LL;

// ---------------------------------------------------------------------------------------------------------------
// input preparation
// ---------------------------------------------------------------------------------------------------------------
struct HnLpipsStrides {
  long long s[4];
};

__global__ __launch_bounds__(256) void hn_lpips_prepare_kernel(const float* pred, HnLpipsStrides ps, const float* gt,
                                                               HnLpipsStrides gs, int n, int h, int w, float* out) {
  const long long hw = (long long)h * w, total = 2LL * n * 3 * hw;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w), y = (int)((i / w) % h), c = (int)((i / hw) % 3), img = (int)(i / (3 * hw));
  const float* src = img < n ? pred : gt;
  const HnLpipsStrides& st = img < n ? ps : gs;
  const int b = img < n ? img : img - n;
  const float v = src[b * st.s[0] + c * st.s[1] + y * st.s[2] + x * st.s[3]];
  const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
  const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
  out[i] = ((2.0f * v - 1.0f) - shift) / scale;
}

// ---------------------------------------------------------------------------------------------------------------
// convolution
// ---------------------------------------------------------------------------------------------------------------
struct HnLpipsConv {
  const float* x;       // (imgs, cin, h, w)
  const float* wt;      // [kpad][mpad]
  const float* bias;    // [cout]
  const int32_t* ktab;  // [kpad]: ci << 8 | ky << 4 | kx, -1 for a padding row
  float* y;             // (imgs, cout, oh, ow)
  int imgs, cin, h, w, cout, oh, ow, stride, pad, relu, kpad, mpad;
  int np;               // imgs * oh * ow
};

template <int TM, int TN, int WM, int WN, int BK>
__global__ __launch_bounds__(64 * WM * WN) void hn_lpips_conv_kernel(HnLpipsConv a) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN, NT = 64 * WM * WN;
  // row strides = 32 mod 64 floats: the two k halves of a wave read different banks
  constexpr int SA = BM % 64 == 32 ? BM : BM + 32, SB = BN % 64 == 32 ? BN : BN + 32;
  constexpr int RA = NT / BM, RB = NT / BN;      // k rows covered per pass of all threads
  constexpr int PA = BK / RA, PB = BK / RB;      // passes = elements per thread and step
  static_assert(NT % BM == 0 && NT % BN == 0 && BK % RA == 0 && BK % RB == 0, "tile and thread counts must divide");
  static_assert(HN_LPIPS_BK % BK == 0, "Kpad must be a whole number of steps");
  __shared__ float As[BK * SA], Bs[BK * SB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hk = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.y * BM;

  // this thread's column of the weight tile and of the activation tile
  const int am = tid % BM, ak = tid / BM;
  const int bn = tid % BN, bk = tid / BN;
  const int ng = blockIdx.x * BN + bn;
  const bool pix_ok = ng < a.np;
  const int ohw = a.oh * a.ow;
  const int img = pix_ok ? ng / ohw : 0, rem = pix_ok ? ng % ohw : 0;
  const int iy0 = (rem / a.ow) * a.stride - a.pad, ix0 = (rem % a.ow) * a.stride - a.pad;
  const float* xin = a.x + (long long)img * a.cin * a.h * a.w;
  const float* wcol = a.wt + m0 + am;

  // The gather's addresses: once per step and workgroup, thread t < BK turns row k0 + t of the k table into
  // {ci * h * w + ky * w + kx, ky << 4 | kx} ({0, -1} for a padding row) in LDS; an element then costs a broadcast LDS read,
  // two adds and the bounds test.  The rows are read from memory one step before they are turned (e_pf), and turned one
  // step before they are used (two buffers), so no step waits for the table.
  __shared__ int2 tab[2][BK];
  static_assert(NT >= BK, "one thread per table row");
  const int pixoff = iy0 * a.w + ix0;
  int e_pf = a.ktab[min(tid, a.kpad - 1)];
  auto write_tab = [&](int k0, int buf) {      // rows k0 .. k0 + BK - 1, from e_pf; then e_pf = the rows of k0 + BK
    if (tid < BK) {
      const int e = k0 + tid < a.kpad ? e_pf : -1;
      const int ci = e >> 8, ky = (e >> 4) & 15, kx = e & 15;
      const bool ok = e >= 0 && ci < a.cin;
      tab[buf][tid] = ok ? make_int2((ci * a.h + ky) * a.w + kx, (ky << 4) | kx) : make_int2(0, -1);
      e_pf = a.ktab[min(k0 + BK + tid, a.kpad - 1)];
    }
  };
  float ra[PA], rb[PB];
  auto fetch = [&](int k0, int buf) {
#pragma unroll
    for (int j = 0; j < PA; ++j) ra[j] = wcol[(long long)(k0 + ak + j * RA) * a.mpad];
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const int2 t = tab[buf][bk + j * RB];
      const int iy = iy0 + (t.y >> 4), ix = ix0 + (t.y & 15);
      const bool ok = pix_ok && t.y >= 0 && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
      // every lane loads (element 0 where the tap is outside) and selects afterwards
      const float v = xin[ok ? pixoff + t.x : 0];
      rb[j] = ok ? v : 0.0f;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.0f;

  write_tab(0, 0);
  __syncthreads();
  fetch(0, 0);
  write_tab(BK, 1);
  for (int k0 = 0, step = 0; k0 < a.kpad; k0 += BK, ++step) {
#pragma unroll
    for (int j = 0; j < PA; ++j) As[(ak + j * RA) * SA + am] = ra[j];
#pragma unroll
    for (int j = 0; j < PB; ++j) Bs[(bk + j * RB) * SB + bn] = rb[j];
    __syncthreads();
    if (k0 + BK < a.kpad) {      // in flight while the matrix core works
      fetch(k0 + BK, (step + 1) & 1);
      write_tab(k0 + 2 * BK, step & 1);      // that buffer was last read by the fetch before the barrier above
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = As[(kk + hk) * SA + (wm * TM + i) * 32 + r];
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = Bs[(kk + hk) * SB + (wn * TN + j) * 32 + r];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = hn_mfma_f32(fa[i], fb[j], acc[i][j]);
    }
    __syncthreads();
  }

  // epilogue: accumulator register q of lane (r, hk) is [row rho(q, hk)][col r] of its tile
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = blockIdx.x * BN + (wn * TN + j) * 32 + r;
    if (n >= a.np) continue;
    const int oi = n / ohw, op = n % ohw;
    float* ycol = a.y + (long long)oi * a.cout * ohw + op;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = m0 + (wm * TM + i) * 32 + hn_rho(q, hk);
        if (m >= a.cout) continue;
        float v = acc[i][j][q] + a.bias[m];
        if (a.relu) v = fmaxf(v, 0.0f);
        ycol[(long long)m * ohw] = v;
      }
    }
  }
}

template <int TM, int TN, int WM, int WN, int BK>
static long long hn_lpips_conv_blocks(int cout, int np) {
  const long long bm = 32 * TM * WM, bn = 32 * TN * WN;
  return ((cout + bm - 1) / bm) * ((np + bn - 1) / bn);
}

template <int TM, int TN, int WM, int WN, int BK>
static void hn_lpips_conv_launch(const HnLpipsConv& a, hipStream_t stream) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  const dim3 grid((unsigned)((a.np + BN - 1) / BN), (unsigned)((a.cout + BM - 1) / BM));
  hipLaunchKernelGGL((hn_lpips_conv_kernel<TM, TN, WM, WN, BK>), grid, dim3(64 * WM * WN), 0, stream, a);
}

static int hn_lpips_out_side(int side, int kernel, int stride, int pad) {
  const int span = side + 2 * pad - kernel;
  return span < 0 ? 0 : span / stride + 1;
}

extern "C" int hn_lpips_conv(const float* x_dev, const float* wt_dev, const float* bias_dev, const int32_t* ktab_dev,
                             float* y_dev, int imgs, int cin, int h, int w, int cout, int kernel, int stride, int pad,
                             int relu, int tile, hnStream_t stream) {
  if (x_dev == nullptr || wt_dev == nullptr || bias_dev == nullptr || ktab_dev == nullptr || y_dev == nullptr) return -2;
  if (imgs <= 0 || cin <= 0 || h <= 0 || w <= 0 || cout <= 0 || stride <= 0 || pad < 0) return -2;
  if (cin > HN_LPIPS_MAX_CHANNELS || cout > HN_LPIPS_MAX_CHANNELS) return -2;
  if (kernel <= 0 || kernel > HN_LPIPS_MAX_KERNEL || pad >= kernel || tile < 0 || tile > 3) return -2;
  const int oh = hn_lpips_out_side(h, kernel, stride, pad), ow = hn_lpips_out_side(w, kernel, stride, pad);
  if (oh <= 0 || ow <= 0) return -2;
  const long long k = (long long)cin * kernel * kernel;
  const long long kpad = (k + HN_LPIPS_BK - 1) / HN_LPIPS_BK * HN_LPIPS_BK;
  const long long mpad = ((long long)cout + HN_LPIPS_MPAD - 1) / HN_LPIPS_MPAD * HN_LPIPS_MPAD;
  const long long np = (long long)imgs * oh * ow;
  if ((long long)imgs * cin * h * w > HN_LPIPS_MAX_ELEMS || np * cout > HN_LPIPS_MAX_ELEMS ||
      kpad * mpad > HN_LPIPS_MAX_ELEMS)
    return -2;
  HnLpipsConv a;
  a.x = x_dev; a.wt = wt_dev; a.bias = bias_dev; a.ktab = ktab_dev; a.y = y_dev;
  a.imgs = imgs; a.cin = cin; a.h = h; a.w = w; a.cout = cout; a.oh = oh; a.ow = ow;
  a.stride = stride; a.pad = pad; a.relu = relu != 0; a.kpad = (int)kpad; a.mpad = (int)mpad; a.np = (int)np;
  // tile 0: the largest shape whose grid fills the machine; 1 / 2 / 3 force 128 x 128 / 64 x 64 / 32 x 64 (tests, tools)
  if (tile == 0) {
    if (cout > 64 && hn_lpips_conv_blocks<2, 2, 2, 2, 16>(cout, a.np) >= HN_LPIPS_FILL_BLOCKS) tile = 1;
    else if (hn_lpips_conv_blocks<1, 1, 2, 2, 64>(cout, a.np) >= HN_LPIPS_FILL_BLOCKS) tile = 2;
    else tile = 3;
  }
  if (tile == 1) hn_lpips_conv_launch<2, 2, 2, 2, 16>(a, (hipStream_t)stream);
  else if (tile == 2) hn_lpips_conv_launch<1, 1, 2, 2, 64>(a, (hipStream_t)stream);
  else hn_lpips_conv_launch<1, 1, 1, 2, 64>(a, (hipStream_t)stream);
  HN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// max pool (floor mode, no padding)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_lpips_maxpool_kernel(const float* x, float* y, long long total, int h, int w,
                                                               int oh, int ow, int kernel, int stride) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % ow), oy = (int)((i / ow) % oh);
  const long long plane = i / ((long long)oh * ow);
  const float* p = x + (plane * h + (long long)oy * stride) * w + (long long)ox * stride;
  float m = p[0];
  for (int ky = 0; ky < kernel; ++ky)
    for (int kx = 0; kx < kernel; ++kx) m = fmaxf(m, p[ky * w + kx]);
  y[i] = m;
}

extern "C" int hn_lpips_maxpool(const float* x_dev, float* y_dev, int planes, int h, int w, int kernel, int stride,
                                hnStream_t stream) {
  if (x_dev == nullptr || y_dev == nullptr) return -2;
  if (planes <= 0 || h <= 0 || w <= 0 || kernel <= 0 || kernel > HN_LPIPS_MAX_KERNEL || stride <= 0) return -2;
  const int oh = hn_lpips_out_side(h, kernel, stride, 0), ow = hn_lpips_out_side(w, kernel, stride, 0);
  if (oh <= 0 || ow <= 0) return -2;
  const long long total = (long long)planes * oh * ow;
  if ((long long)planes * h * w > HN_LPIPS_MAX_ELEMS) return -2;
  hipLaunchKernelGGL(hn_lpips_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     x_dev, y_dev, total, h, w, oh, ow, kernel, stride);
  HN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// one tap's term of the metric
// ---------------------------------------------------------------------------------------------------------------
// lane 0 of a 64-lane wave ends up with the sum, in a fixed order
HN_DEV float hn_lpips_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One workgroup per 64 pixels of one image pair, 16 waves: wave g owns the channels g, g + 16, ... and lane p one pixel
// (consecutive lanes read consecutive pixels of a channel's plane).  Every sum over channels is 16 running sums, one per
// wave, added in ascending g by the first wave: the channel norms of both feature vectors first, then
// sum_c w[c] * (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2; the 64 pixels' values are added by a wave butterfly.
__global__ __launch_bounds__(HN_LPIPS_DIST_PIXELS* HN_LPIPS_DIST_GROUPS) void hn_lpips_distance_kernel(
    const float* feat, const float* lin, int n, int c, int hw, float* partials) {
  constexpr int PX = HN_LPIPS_DIST_PIXELS, G = HN_LPIPS_DIST_GROUPS;
  __shared__ float ra[G][PX], rb[G][PX], na[PX], nb[PX];
  const int pair = blockIdx.y, lane = threadIdx.x % PX, g = threadIdx.x / PX;
  const int p = blockIdx.x * PX + lane;
  const bool ok = p < hw;
  const float* fa = feat + (long long)pair * c * hw + p;
  const float* fb = feat + (long long)(pair + n) * c * hw + p;
  float sa = 0.0f, sb = 0.0f;
  if (ok)
    for (int ch = g; ch < c; ch += G) {
      const float va = fa[(long long)ch * hw], vb = fb[(long long)ch * hw];
      sa += va * va;
      sb += vb * vb;
    }
  ra[g][lane] = sa;
  rb[g][lane] = sb;
  __syncthreads();
  if (g == 0) {
    float ta = 0.0f, tb = 0.0f;
#pragma unroll
    for (int i = 0; i < G; ++i) {
      ta += ra[i][lane];
      tb += rb[i][lane];
    }
    na[lane] = sqrtf(ta) + 1e-10f;
    nb[lane] = sqrtf(tb) + 1e-10f;
  }
  __syncthreads();
  float sd = 0.0f;
  if (ok) {
    const float da = na[lane], db = nb[lane];
    for (int ch = g; ch < c; ch += G) {
      const float diff = fa[(long long)ch * hw] / da - fb[(long long)ch * hw] / db;
      sd += lin[ch] * (diff * diff);
    }
  }
  ra[g][lane] = sd;
  __syncthreads();
  if (g == 0) {
    float d = 0.0f;
#pragma unroll
    for (int i = 0; i < G; ++i) d += ra[i][lane];
    d = hn_lpips_wave_sum(d);
    if (lane == 0) partials[(long long)pair * gridDim.x + blockIdx.x] = d;
  }
}

// out[pair * 5 + layer] = (the pair's partial sums, added in order by one workgroup) / pixels
__global__ __launch_bounds__(HN_LPIPS_SUM_THREADS) void hn_lpips_distance_sum_kernel(const float* partials, int blocks,
                                                                                     int hw, int layer, float* out) {
  __shared__ float red[HN_LPIPS_SUM_THREADS / 64];
  const float* p = partials + (long long)blockIdx.x * blocks;
  float v = 0.0f;
  for (int i = threadIdx.x; i < blocks; i += HN_LPIPS_SUM_THREADS) v += p[i];
  v = hn_lpips_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.0f;
    for (int i = 0; i < HN_LPIPS_SUM_THREADS / 64; ++i) s += red[i];
    out[blockIdx.x * HN_LPIPS_LAYERS + layer] = s / (float)hw;
  }
}

static long long hn_lpips_dist_blocks(int h, int w) {
  return ((long long)h * w + HN_LPIPS_DIST_PIXELS - 1) / HN_LPIPS_DIST_PIXELS;
}

extern "C" int hn_lpips_workspace_bytes(int n, int h, int w, int64_t* bytes) {
  if (bytes == nullptr || n <= 0 || h <= 0 || w <= 0) return -2;
  if ((long long)n * h * w > HN_LPIPS_MAX_ELEMS) return -2;
  *bytes = (n * hn_lpips_dist_blocks(h, w) * 4 + 15) / 16 * 16;
  return 0;
}

extern "C" int hn_lpips_distance(const float* feat_dev, const float* lin_dev, int n, int c, int h, int w, int layer,
                                 float* out_dev, void* workspace, hnStream_t stream) {
  if (feat_dev == nullptr || lin_dev == nullptr || out_dev == nullptr || workspace == nullptr) return -2;
  if (n <= 0 || c <= 0 || c > HN_LPIPS_MAX_CHANNELS || h <= 0 || w <= 0 || layer < 0 || layer >= HN_LPIPS_LAYERS)
    return -2;
  if (2LL * n * c * h * w > HN_LPIPS_MAX_ELEMS) return -2;
  const long long blocks = hn_lpips_dist_blocks(h, w);
  if (n > 65535) return -2;      // the pair index is the grid's second dimension
  float* partials = static_cast<float*>(workspace);
  hipLaunchKernelGGL(hn_lpips_distance_kernel, dim3((unsigned)blocks, (unsigned)n),
                     dim3(HN_LPIPS_DIST_PIXELS * HN_LPIPS_DIST_GROUPS), 0,
                     (hipStream_t)stream, feat_dev, lin_dev, n, c, h * w, partials);
  HN_CHECK_LAUNCH();
  hipLaunchKernelGGL(hn_lpips_distance_sum_kernel, dim3((unsigned)n), dim3(HN_LPIPS_SUM_THREADS), 0,
                     (hipStream_t)stream, partials, (int)blocks, h * w, layer, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// entry point of the input preparation (net: 0 = alex, 1 = vgg; decides the smallest legal side)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int hn_lpips_prepare(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides,
                                int n, int h, int w, int net, float* out_dev, hnStream_t stream) {
  if (pred == nullptr || gt == nullptr || pred_strides == nullptr || gt_strides == nullptr || out_dev == nullptr) return -2;
  if (n <= 0 || h <= 0 || w <= 0 || net < 0 || net > 1) return -2;
  const int min_side = net == 0 ? HN_LPIPS_ALEX_MIN_SIDE : HN_LPIPS_VGG_MIN_SIDE;
  if (h < min_side || w < min_side) return -2;
  const long long total = 2LL * n * 3 * h * w;
  if (total > HN_LPIPS_MAX_ELEMS) return -2;
  HnLpipsStrides ps, gs;
  for (int i = 0; i < 4; ++i) {
    ps.s[i] = pred_strides[i];
    gs.s[i] = gt_strides[i];
  }
  hipLaunchKernelGGL(hn_lpips_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     pred, ps, gt, gs, n, h, w, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}
