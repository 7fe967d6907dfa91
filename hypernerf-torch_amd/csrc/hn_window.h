// The windowed-moments core that SSIM (hn_metrics.hip) and MS-SSIM (hn_msssim.hip) share: one workgroup of 256 threads
// per 32 x 16 tile of one (n, c) plane of a pair of strided images, the five moments (x, y, x^2, y^2, xy) of a separable
// window as a row pass over the staged tile in LDS and a column pass into registers, and fixed-order sums without float
// atomics.  How a tile is staged (reflect or clamp), what is made of the moments and where the sums go is each metric's
// own.  The accumulation statements below ARE the metrics' rounding: zero-initialised accumulators, taps ascending,
// `m += wk * v` with the squares as `wk * (xv * xv)` (the library builds with -ffp-contract=off).
#pragma once
#include "hn_common.h"

#define HN_WIN_TW 32
#define HN_WIN_TH 16
#define HN_WIN_THREADS 256

struct HnWinPair {
  const float* x;
  const float* y;
  long long xs[4], ys[4];   // element strides of (n, c, h, w)
  int c, h, w;
  int tiles_x, tiles_y;
  float c1, c2;             // the constants of the SSIM ratios (set by the metric)
};

// workgroups (tiles of all n * c planes) of an (n, c, h, w) pair, or 0 for a shape the kernels refuse
static inline long long hn_win_blocks(int n, int c, int h, int w) {
  if (n < 1 || c < 1 || h < 1 || w < 1) return 0;
  const long long tiles = (long long)((w + HN_WIN_TW - 1) / HN_WIN_TW) * ((h + HN_WIN_TH - 1) / HN_WIN_TH);
  if (tiles * n * c > 0x7fffffffLL || (long long)n * c * h * w > (1LL << 40)) return 0;
  return tiles * n * c;
}

static inline void hn_win_pair(HnWinPair* a, const float* x, const int64_t* xs, const float* y, const int64_t* ys, int c,
                               int h, int w) {
  a->x = x;
  a->y = y;
  for (int i = 0; i < 4; ++i) {
    a->xs[i] = xs[i];
    a->ys[i] = ys[i];
  }
  a->c = c;
  a->h = h;
  a->w = w;
  a->tiles_x = (w + HN_WIN_TW - 1) / HN_WIN_TW;
  a->tiles_y = (h + HN_WIN_TH - 1) / HN_WIN_TH;
}

// both images contiguous (n, c, h, w)
static inline void hn_win_pair_contiguous(HnWinPair* a, const float* x, const float* y, int c, int h, int w) {
  const int64_t s[4] = {(int64_t)c * h * w, (int64_t)h * w, w, 1};
  hn_win_pair(a, x, s, y, s, c, h, w);
}

struct HnWinTile {
  int plane, n, c, y0, x0;
};

HN_DEV HnWinTile hn_win_tile(const HnWinPair& a) {
  HnWinTile t;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  t.plane = b / a.tiles_y;
  t.n = t.plane / a.c;
  t.c = t.plane % a.c;
  t.y0 = ty * HN_WIN_TH;
  t.x0 = tx * HN_WIN_TW;
  return t;
}

// Both passes: TAPS > 0 is the window's length at compile time (unrolled), TAPS == 0 takes `taps` at run time.

// row pass: hm[k * plane + row * OW + col] for `rows` staged rows (row stride SW) and OW output columns, the window
// starting at staged column `col`
template <int TAPS>
HN_DEV void hn_win_row_pass(const float* w, int taps, const float* sx, const float* sy, int SW, float* hm, int rows,
                            int OW, int plane) {
  const int n = TAPS > 0 ? TAPS : taps;
  for (int i = threadIdx.x; i < rows * OW; i += HN_WIN_THREADS) {
    const int row = i / OW, col = i % OW;
    const float* px = sx + row * SW + col;
    const float* py = sy + row * SW + col;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const float wk = w[k], xv = px[k], yv = py[k];
      m0 += wk * xv;
      m1 += wk * yv;
      m2 += wk * (xv * xv);
      m3 += wk * (yv * yv);
      m4 += wk * (xv * yv);
    }
    hm[i] = m0;
    hm[plane + i] = m1;
    hm[2 * plane + i] = m2;
    hm[3 * plane + i] = m3;
    hm[4 * plane + i] = m4;
  }
}

// column pass for one pixel: the five moments of the window whose first row-pass row is `row`, at column `col`
template <int TAPS>
HN_DEV void hn_win_col_pass(const float* w, int taps, const float* hm, int OW, int plane, int row, int col, float m[5]) {
  const int n = TAPS > 0 ? TAPS : taps;
#pragma unroll
  for (int j = 0; j < 5; ++j) m[j] = 0.0f;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const float wk = w[k];
    const float* p = hm + (row + k) * OW + col;
#pragma unroll
    for (int j = 0; j < 5; ++j) m[j] += wk * p[j * plane];
  }
}

// lane 0 of a 64-lane wave ends up with the sum, in a fixed order
HN_DEV float hn_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// fixed-order workgroup sum (wave butterfly, then the wave totals in order); the result is valid in thread 0
template <int THREADS>
HN_DEV float hn_block_sum(float v, float* red) {
  v = hn_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = 0.0f;
  if (threadIdx.x == 0)
    for (int i = 0; i < THREADS / 64; ++i) s += red[i];
  return s;
}
