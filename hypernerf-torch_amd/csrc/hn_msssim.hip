// Multi-scale SSIM (Wang, Simoncelli, Bovik 2003, as stated by the widely used NumPy `MultiScaleSSIM`): the numbers of one
// five-level pyramid per image, a metric without a backward.
//
// One launch per level.  A workgroup of 256 threads owns the 32 x 16 tile of INPUT pixels at (x0, y0) of one (n, c)
// plane; the tiles cover the input, so every pixel has exactly one owner.  The workgroup stages its tile plus the
// `size - 1` halo to the right and below (up to 42 x 26) of both images in LDS, coordinates clamped to the image at load
// time.  From that it does two things:
//   * the VALID correlation (no padding) of the five moments x, y, x^2, y^2, xy with the outer product of the 1-D
//     window, as a row pass into LDS and a column pass into registers, for the outputs (x0 + col, y0 + row) that lie
//     inside the (h - size + 1) x (w - size + 1) valid region; per output the two ratios
//       ssim = ((2 mu1 mu2 + c1) v1) / ((mu1^2 + mu2^2 + c1) v2),  cs = v1 / v2,  v1 = 2 s12 + c2,  v2 = s11 + s22 + c2
//     are summed over the tile in a fixed order and the two sums written to the workgroup's slot of the workspace;
//   * the next level's images: the 2 x 2 box mean of the tile's own pixels, out[i][j] = mean(in[2i..2i+1][2j..2j+1]),
//     an index past the edge replaced by the edge pixel (which the clamped staging already did), (h+1)/2 x (w+1)/2.
// Level 0 reads the caller's tensors through their element strides, levels 1 .. 4 the contiguous workspace planes.  The
// window size is a runtime value 1 .. 11 (min(11, h, w) of the level, even sizes included); 11 has an unrolled build.
//
// A last launch of one workgroup per (image, level) adds that pair's slots in a fixed order and divides by the number of
// valid positions of all channels.  No float atomics anywhere: the same bits run to run.
#include "hn_common.h"

#define HN_MS_TW 32
#define HN_MS_TH 16
#define HN_MS_THREADS 256
#define HN_MS_SW (HN_MS_TW + HN_MS_MAX_SIZE - 1)
#define HN_MS_SH (HN_MS_TH + HN_MS_MAX_SIZE - 1)

struct HnMsLevel {
  const float* x;
  const float* y;
  long long xs[4], ys[4];   // element strides of (n, c, h, w)
  int c, h, w, size;
  int tiles_x, tiles_y;
  float c1, c2;
  float taps[HN_MS_MAX_SIZE];
  float* next_x;            // (n, c, h2, w2) contiguous, or NULL on the last level
  float* next_y;
  int h2, w2;
  float* partials;          // [block][2]: sum of ssim, sum of cs
};

struct HnMsFinal {
  const float* partials[HN_MS_LEVELS];
  int blocks_per_image[HN_MS_LEVELS];
  float count[HN_MS_LEVELS];
};

// fixed-order workgroup sum (wave butterfly, then the four wave totals in order); the result is valid in thread 0
HN_DEV float hn_ms_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = 0.0f;
  if (threadIdx.x == 0)
    for (int i = 0; i < HN_MS_THREADS / 64; ++i) s += red[i];
  return s;
}

// SIZE = 11: the window of every level whose sides are at least 11, unrolled; SIZE = 0: `a.size` at run time
template <int SIZE>
__global__ __launch_bounds__(HN_MS_THREADS) void hn_msssim_level_kernel(HnMsLevel a) {
  __shared__ float sx[HN_MS_SH * HN_MS_SW], sy[HN_MS_SH * HN_MS_SW];
  __shared__ float hm[5 * HN_MS_SH * HN_MS_TW];
  __shared__ float red[HN_MS_THREADS / 64];
  const int size = SIZE > 0 ? SIZE : a.size;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  const int plane = b / a.tiles_y;
  const int n = plane / a.c, c = plane % a.c;
  const int y0 = ty * HN_MS_TH, x0 = tx * HN_MS_TW;
  const int rows = HN_MS_TH + size - 1, cols = HN_MS_TW + size - 1;     // staged extent in use

  const float* px = a.x + n * a.xs[0] + c * a.xs[1];
  const float* py = a.y + n * a.ys[0] + c * a.ys[1];
  for (int i = threadIdx.x; i < rows * cols; i += HN_MS_THREADS) {
    const int r = i / cols, q = i % cols;
    const int gy = min(y0 + r, a.h - 1), gx = min(x0 + q, a.w - 1);
    sx[r * HN_MS_SW + q] = px[gy * a.xs[2] + gx * a.xs[3]];
    sy[r * HN_MS_SW + q] = py[gy * a.ys[2] + gx * a.ys[3]];
  }
  __syncthreads();

  // the next level's pair: threads 0 .. 127 the first image, 128 .. 255 the second, one output pixel each
  if (a.next_x != nullptr) {
    const int t = threadIdx.x & 127;
    const int i = t / (HN_MS_TW / 2), j = t % (HN_MS_TW / 2);
    const int oy = y0 / 2 + i, ox = x0 / 2 + j;
    if (oy < a.h2 && ox < a.w2) {
      const float* s = (threadIdx.x < 128 ? sx : sy) + (2 * i) * HN_MS_SW + 2 * j;
      // the staged extent covers at least the tile itself (size >= 1), clamped at the image's edge
      const float v = ((s[0] + s[1]) + (s[HN_MS_SW] + s[HN_MS_SW + 1])) * 0.25f;
      float* o = threadIdx.x < 128 ? a.next_x : a.next_y;
      o[((long long)plane * a.h2 + oy) * a.w2 + ox] = v;
    }
  }

  // row pass: hm[k][row][col] for the staged rows and the tile's 32 output columns
  constexpr int PLANE = HN_MS_SH * HN_MS_TW;
  for (int i = threadIdx.x; i < rows * HN_MS_TW; i += HN_MS_THREADS) {
    const int r = i / HN_MS_TW, q = i % HN_MS_TW;
    const float* rx = sx + r * HN_MS_SW + q;
    const float* ry = sy + r * HN_MS_SW + q;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
    for (int k = 0; k < size; ++k) {
      const float wk = a.taps[k], xv = rx[k], yv = ry[k];
      m0 += wk * xv;
      m1 += wk * yv;
      m2 += wk * (xv * xv);
      m3 += wk * (yv * yv);
      m4 += wk * (xv * yv);
    }
    hm[i] = m0;
    hm[PLANE + i] = m1;
    hm[2 * PLANE + i] = m2;
    hm[3 * PLANE + i] = m3;
    hm[4 * PLANE + i] = m4;
  }
  __syncthreads();

  // column pass and the two ratios, for the outputs inside the valid region
  const int oh = a.h - size + 1, ow = a.w - size + 1;
  const int col = threadIdx.x % HN_MS_TW, gx = x0 + col;
  float acc_ssim = 0.0f, acc_cs = 0.0f;
  for (int row = threadIdx.x / HN_MS_TW; row < HN_MS_TH; row += HN_MS_THREADS / HN_MS_TW) {
    if (y0 + row >= oh || gx >= ow) continue;
    float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < size; ++k) {
      const float wk = a.taps[k];
      const float* p = hm + (row + k) * HN_MS_TW + col;
#pragma unroll
      for (int j = 0; j < 5; ++j) m[j] += wk * p[j * PLANE];
    }
    const float mu11 = m[0] * m[0], mu22 = m[1] * m[1], mu12 = m[0] * m[1];
    const float s11 = m[2] - mu11, s22 = m[3] - mu22, s12 = m[4] - mu12;
    const float v1 = 2.0f * s12 + a.c2;
    const float v2 = s11 + s22 + a.c2;
    acc_ssim += ((2.0f * mu12 + a.c1) * v1) / ((mu11 + mu22 + a.c1) * v2);
    acc_cs += v1 / v2;
  }
  const float s_ssim = hn_ms_block_sum(acc_ssim, red);
  const float s_cs = hn_ms_block_sum(acc_cs, red);
  if (threadIdx.x == 0) {
    a.partials[2 * (long long)blockIdx.x] = s_ssim;
    a.partials[2 * (long long)blockIdx.x + 1] = s_cs;
  }
}

// block (image, level): levels_out[image][level] = (sum ssim, sum cs) of the image's slots / count
__global__ __launch_bounds__(HN_MS_THREADS) void hn_msssim_final_kernel(HnMsFinal f, float* levels_out) {
  __shared__ float red[HN_MS_THREADS / 64];
  const int image = blockIdx.x / HN_MS_LEVELS, level = blockIdx.x % HN_MS_LEVELS;
  const int nb = f.blocks_per_image[level];
  const float* p = f.partials[level] + 2 * (long long)image * nb;
  float v_ssim = 0.0f, v_cs = 0.0f;
  for (int i = threadIdx.x; i < nb; i += HN_MS_THREADS) {
    v_ssim += p[2 * i];
    v_cs += p[2 * i + 1];
  }
  const float s_ssim = hn_ms_block_sum(v_ssim, red);
  const float s_cs = hn_ms_block_sum(v_cs, red);
  if (threadIdx.x == 0) {
    levels_out[2 * blockIdx.x] = s_ssim / f.count[level];
    levels_out[2 * blockIdx.x + 1] = s_cs / f.count[level];
  }
}

// The pyramid's host arithmetic: sides, tiles and the workspace layout in floats,
//   [level 1 .. 4: first image (n, c, h_l, w_l), second image] [level 0 .. 4: (n * c * tiles_l, 2) partial sums]
struct HnMsPlan {
  int h[HN_MS_LEVELS], w[HN_MS_LEVELS];
  long long tiles[HN_MS_LEVELS];          // per plane
  long long plane_off[HN_MS_LEVELS];      // first image of the level (level 0: unused); the second follows it
  long long partial_off[HN_MS_LEVELS];
  long long total;
};

static int hn_ms_plan(int n, int c, int h, int w, HnMsPlan* p) {
  if (n < 1 || c < 1 || h < 1 || w < 1) return -2;
  if ((long long)n * c * h * w > (1LL << 40)) return -2;
  long long off = 0;
  for (int l = 0; l < HN_MS_LEVELS; ++l) {
    p->h[l] = l == 0 ? h : (p->h[l - 1] + 1) / 2;
    p->w[l] = l == 0 ? w : (p->w[l - 1] + 1) / 2;
    p->tiles[l] = (long long)((p->w[l] + HN_MS_TW - 1) / HN_MS_TW) * ((p->h[l] + HN_MS_TH - 1) / HN_MS_TH);
    if (p->tiles[l] * n * c > 0x7fffffffLL) return -2;
    p->plane_off[l] = off;
    if (l > 0) off += 2LL * n * c * p->h[l] * p->w[l];
  }
  for (int l = 0; l < HN_MS_LEVELS; ++l) {
    p->partial_off[l] = off;
    off += 2LL * n * c * p->tiles[l];
  }
  p->total = off;
  return 0;
}

extern "C" int hn_msssim_workspace_bytes(int n, int c, int h, int w, int64_t* bytes) {
  HnMsPlan p;
  if (bytes == nullptr || hn_ms_plan(n, c, h, w, &p) != 0) return -2;
  *bytes = (p.total * 4 + 15) / 16 * 16;
  return 0;
}

extern "C" int hn_msssim_forward(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides,
                                 int n, int c, int h, int w, const float* taps_host, const int* sizes_host, float c1,
                                 float c2, float* levels_out, void* workspace, hnStream_t stream) {
  // every check comes before the first launch
  HnMsPlan p;
  if (hn_ms_plan(n, c, h, w, &p) != 0) return -2;
  if (pred == nullptr || gt == nullptr || pred_strides == nullptr || gt_strides == nullptr || taps_host == nullptr ||
      sizes_host == nullptr || levels_out == nullptr || workspace == nullptr)
    return -2;
  if ((long long)n * HN_MS_LEVELS > 0x7fffffffLL) return -2;
  for (int l = 0; l < HN_MS_LEVELS; ++l)
    if (sizes_host[l] < 1 || sizes_host[l] > HN_MS_MAX_SIZE || sizes_host[l] > p.h[l] || sizes_host[l] > p.w[l]) return -2;
  float* ws = static_cast<float*>(workspace);
  HnMsFinal f;
  for (int l = 0; l < HN_MS_LEVELS; ++l) {
    HnMsLevel a;
    const long long plane_elems = (long long)n * c * p.h[l] * p.w[l];
    if (l == 0) {
      a.x = pred;
      a.y = gt;
      for (int i = 0; i < 4; ++i) {
        a.xs[i] = pred_strides[i];
        a.ys[i] = gt_strides[i];
      }
    } else {
      a.x = ws + p.plane_off[l];
      a.y = a.x + plane_elems;
      a.xs[3] = a.ys[3] = 1;
      a.xs[2] = a.ys[2] = p.w[l];
      a.xs[1] = a.ys[1] = (long long)p.h[l] * p.w[l];
      a.xs[0] = a.ys[0] = a.xs[1] * c;
    }
    a.c = c;
    a.h = p.h[l];
    a.w = p.w[l];
    a.size = sizes_host[l];
    a.tiles_x = (p.w[l] + HN_MS_TW - 1) / HN_MS_TW;
    a.tiles_y = (p.h[l] + HN_MS_TH - 1) / HN_MS_TH;
    a.c1 = c1;
    a.c2 = c2;
    for (int i = 0; i < HN_MS_MAX_SIZE; ++i) a.taps[i] = i < a.size ? taps_host[l * HN_MS_MAX_SIZE + i] : 0.0f;
    if (l + 1 < HN_MS_LEVELS) {
      a.next_x = ws + p.plane_off[l + 1];
      a.next_y = a.next_x + (long long)n * c * p.h[l + 1] * p.w[l + 1];
      a.h2 = p.h[l + 1];
      a.w2 = p.w[l + 1];
    } else {
      a.next_x = a.next_y = nullptr;
      a.h2 = a.w2 = 0;
    }
    a.partials = ws + p.partial_off[l];
    const unsigned blocks = (unsigned)(p.tiles[l] * n * c);
    if (a.size == HN_MS_MAX_SIZE)
      hipLaunchKernelGGL(hn_msssim_level_kernel<HN_MS_MAX_SIZE>, dim3(blocks), dim3(HN_MS_THREADS), 0,
                         (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(hn_msssim_level_kernel<0>, dim3(blocks), dim3(HN_MS_THREADS), 0, (hipStream_t)stream, a);
    HN_CHECK_LAUNCH();
    f.partials[l] = a.partials;
    f.blocks_per_image[l] = (int)(p.tiles[l] * c);
    f.count[l] = (float)((double)c * (p.h[l] - a.size + 1) * (p.w[l] - a.size + 1));
  }
  hipLaunchKernelGGL(hn_msssim_final_kernel, dim3((unsigned)(n * HN_MS_LEVELS)), dim3(HN_MS_THREADS), 0,
                     (hipStream_t)stream, f, levels_out);
  HN_CHECK_LAUNCH();
  return 0;
}
