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
//
// The tile, the image pair, the two passes and the sums are hn_window.h's, shared with hn_metrics.hip.
#include "hn_window.h"

#define HN_MS_SW (HN_WIN_TW + HN_MS_MAX_SIZE - 1)
#define HN_MS_SH (HN_WIN_TH + HN_MS_MAX_SIZE - 1)

struct HnMsLevel : HnWinPair {
  int size;
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

// SIZE = 11: the window of every level whose sides are at least 11, unrolled; SIZE = 0: `a.size` at run time
template <int SIZE>
__global__ __launch_bounds__(HN_WIN_THREADS) void hn_msssim_level_kernel(HnMsLevel a) {
  __shared__ float sx[HN_MS_SH * HN_MS_SW], sy[HN_MS_SH * HN_MS_SW];
  __shared__ float hm[5 * HN_MS_SH * HN_WIN_TW];
  __shared__ float red[HN_WIN_THREADS / 64];
  const int size = SIZE > 0 ? SIZE : a.size;
  const HnWinTile t = hn_win_tile(a);
  const int plane = t.plane, y0 = t.y0, x0 = t.x0;
  const int rows = HN_WIN_TH + size - 1, cols = HN_WIN_TW + size - 1;     // staged extent in use

  const float* px = a.x + t.n * a.xs[0] + t.c * a.xs[1];
  const float* py = a.y + t.n * a.ys[0] + t.c * a.ys[1];
  for (int i = threadIdx.x; i < rows * cols; i += HN_WIN_THREADS) {
    const int r = i / cols, q = i % cols;
    const int gy = min(y0 + r, a.h - 1), gx = min(x0 + q, a.w - 1);
    sx[r * HN_MS_SW + q] = px[gy * a.xs[2] + gx * a.xs[3]];
    sy[r * HN_MS_SW + q] = py[gy * a.ys[2] + gx * a.ys[3]];
  }
  __syncthreads();

  // the next level's pair: threads 0 .. 127 the first image, 128 .. 255 the second, one output pixel each
  if (a.next_x != nullptr) {
    const int half = threadIdx.x & 127;
    const int i = half / (HN_WIN_TW / 2), j = half % (HN_WIN_TW / 2);
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
  constexpr int PLANE = HN_MS_SH * HN_WIN_TW;
  hn_win_row_pass<SIZE>(a.taps, size, sx, sy, HN_MS_SW, hm, rows, HN_WIN_TW, PLANE);
  __syncthreads();

  // column pass and the two ratios, for the outputs inside the valid region
  const int oh = a.h - size + 1, ow = a.w - size + 1;
  const int col = threadIdx.x % HN_WIN_TW, gx = x0 + col;
  float acc_ssim = 0.0f, acc_cs = 0.0f;
  for (int row = threadIdx.x / HN_WIN_TW; row < HN_WIN_TH; row += HN_WIN_THREADS / HN_WIN_TW) {
    if (y0 + row >= oh || gx >= ow) continue;
    float m[5];
    hn_win_col_pass<SIZE>(a.taps, size, hm, HN_WIN_TW, PLANE, row, col, m);
    const float mu11 = m[0] * m[0], mu22 = m[1] * m[1], mu12 = m[0] * m[1];
    const float s11 = m[2] - mu11, s22 = m[3] - mu22, s12 = m[4] - mu12;
    const float v1 = 2.0f * s12 + a.c2;
    const float v2 = s11 + s22 + a.c2;
    acc_ssim += ((2.0f * mu12 + a.c1) * v1) / ((mu11 + mu22 + a.c1) * v2);
    acc_cs += v1 / v2;
  }
  const float s_ssim = hn_block_sum<HN_WIN_THREADS>(acc_ssim, red);
  const float s_cs = hn_block_sum<HN_WIN_THREADS>(acc_cs, red);
  if (threadIdx.x == 0) {
    a.partials[2 * (long long)blockIdx.x] = s_ssim;
    a.partials[2 * (long long)blockIdx.x + 1] = s_cs;
  }
}

// block (image, level): levels_out[image][level] = (sum ssim, sum cs) of the image's slots / count
__global__ __launch_bounds__(HN_WIN_THREADS) void hn_msssim_final_kernel(HnMsFinal f, float* levels_out) {
  __shared__ float red[HN_WIN_THREADS / 64];
  const int image = blockIdx.x / HN_MS_LEVELS, level = blockIdx.x % HN_MS_LEVELS;
  const int nb = f.blocks_per_image[level];
  const float* p = f.partials[level] + 2 * (long long)image * nb;
  float v_ssim = 0.0f, v_cs = 0.0f;
  for (int i = threadIdx.x; i < nb; i += HN_WIN_THREADS) {
    v_ssim += p[2 * i];
    v_cs += p[2 * i + 1];
  }
  const float s_ssim = hn_block_sum<HN_WIN_THREADS>(v_ssim, red);
  const float s_cs = hn_block_sum<HN_WIN_THREADS>(v_cs, red);
  if (threadIdx.x == 0) {
    levels_out[2 * blockIdx.x] = s_ssim / f.count[level];
    levels_out[2 * blockIdx.x + 1] = s_cs / f.count[level];
  }
}

// The pyramid's host arithmetic: sides, tiles and the workspace layout in floats,
//   [level 1 .. 4: first image (n, c, h_l, w_l), second image] [level 0 .. 4: (n * c * tiles_l, 2) partial sums]
struct HnMsPlan {
  int h[HN_MS_LEVELS], w[HN_MS_LEVELS];
  long long blocks[HN_MS_LEVELS];         // tiles of all n * c planes
  long long plane_off[HN_MS_LEVELS];      // first image of the level (level 0: unused); the second follows it
  long long partial_off[HN_MS_LEVELS];
  long long total;
};

static int hn_ms_plan(int n, int c, int h, int w, HnMsPlan* p) {
  long long off = 0;
  for (int l = 0; l < HN_MS_LEVELS; ++l) {
    p->h[l] = l == 0 ? h : (p->h[l - 1] + 1) / 2;
    p->w[l] = l == 0 ? w : (p->w[l - 1] + 1) / 2;
    p->blocks[l] = hn_win_blocks(n, c, p->h[l], p->w[l]);
    if (p->blocks[l] == 0) return -2;
    p->plane_off[l] = off;
    if (l > 0) off += 2LL * n * c * p->h[l] * p->w[l];
  }
  for (int l = 0; l < HN_MS_LEVELS; ++l) {
    p->partial_off[l] = off;
    off += 2 * p->blocks[l];
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
    if (l == 0) {
      hn_win_pair(&a, pred, pred_strides, gt, gt_strides, c, h, w);
    } else {
      const float* x = ws + p.plane_off[l];
      hn_win_pair_contiguous(&a, x, x + (long long)n * c * p.h[l] * p.w[l], c, p.h[l], p.w[l]);
    }
    a.size = sizes_host[l];
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
    const unsigned blocks = (unsigned)p.blocks[l];
    if (a.size == HN_MS_MAX_SIZE)
      hipLaunchKernelGGL(hn_msssim_level_kernel<HN_MS_MAX_SIZE>, dim3(blocks), dim3(HN_WIN_THREADS), 0,
                         (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(hn_msssim_level_kernel<0>, dim3(blocks), dim3(HN_WIN_THREADS), 0, (hipStream_t)stream, a);
    HN_CHECK_LAUNCH();
    f.partials[l] = a.partials;
    f.blocks_per_image[l] = (int)(p.blocks[l] / n);
    f.count[l] = (float)((double)c * (p.h[l] - a.size + 1) * (p.w[l] - a.size + 1));
  }
  hipLaunchKernelGGL(hn_msssim_final_kernel, dim3((unsigned)(n * HN_MS_LEVELS)), dim3(HN_WIN_THREADS), 0,
                     (hipStream_t)stream, f, levels_out);
  HN_CHECK_LAUNCH();
  return 0;
}
