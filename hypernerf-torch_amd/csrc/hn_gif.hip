// Eval-side image outputs (include/hn_kernels.h, "GIF of the evaluated frames"): colour quantisation of 8-bit frames for
// a GIF (histogram over 2^18 colour cells, nearest-of-256 palette search), the colour-mapped depth image of the
// validation step, and GIF's LZW coder (host code: a serial chain per stream).  Integer arithmetic throughout the
// quantiser, so every result is exact and independent of scheduling; the depth map is fp32 with every operation rounded
// on its own (the build sets -ffp-contract=off).
#include <float.h>
#include <string.h>

#include "hn_common.h"

// sum over the 64 lanes of a wave, in every lane (an xor butterfly: integer adds, any order gives the same bits)
HN_DEV unsigned long long hn_wave_sum_u64(unsigned long long x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), m, 64);
    x += ((unsigned long long)hi << 32) | lo;
  }
  return x;
}

// ------------------------------------------------------------------------------------------------
// hn_color_hist: hist[key] += {1, r, g, b} per pixel, key = (r>>2)<<12 | (g>>2)<<6 | b>>2, four 64-bit words per cell.
// A rendered frame on a white (or black) background puts most of its pixels into one cell, so equal keys are folded on
// chip before they reach memory, as hn_cc_sizes folds labels:
//   - the pixels of a workgroup's tile that carry the key of its first pixel are summed in registers, per wave through
//     the butterfly above, per workgroup through four LDS words, and leave as ONE group of four adds;
//   - the other pixels are folded per wave: the lanes that hold one key elect the lowest as leader (ballots), the
//     leader gets the group's sums, and after the election loop all leaders of the wave issue their adds together.
// Packed per-lane sums: r | g << 17 | b << 34 | count << 51.  A thread holds at most HN_HIST_PER_THREAD = 8 pixels of the
// common key, a wave 512: every colour sum stays below 512 * 255 < 2^17 and the count below 2^13.
// ------------------------------------------------------------------------------------------------
static_assert(HN_HIST_BINS == 1 << 18, "hn_kernels.h: HN_HIST_BINS is one cell per 18-bit colour key");
#define HN_HIST_PER_THREAD 8
#define HN_HIST_TILE (256 * HN_HIST_PER_THREAD)
#define HN_HIST_FIELD 17
#define HN_HIST_MASK ((1ull << HN_HIST_FIELD) - 1ull)

HN_DEV unsigned long long hn_hist_pack(unsigned r, unsigned g, unsigned b) {
  return (unsigned long long)r | ((unsigned long long)g << HN_HIST_FIELD) | ((unsigned long long)b << (2 * HN_HIST_FIELD)) |
         (1ull << (3 * HN_HIST_FIELD));
}

HN_DEV void hn_hist_add(unsigned long long* __restrict__ hist, int key, unsigned long long packed) {
  unsigned long long* cell = hist + 4 * (size_t)key;
  atomicAdd(cell + 0, packed >> (3 * HN_HIST_FIELD));
  atomicAdd(cell + 1, packed & HN_HIST_MASK);
  atomicAdd(cell + 2, (packed >> HN_HIST_FIELD) & HN_HIST_MASK);
  atomicAdd(cell + 3, (packed >> (2 * HN_HIST_FIELD)) & HN_HIST_MASK);
}

__global__ __launch_bounds__(256) void hn_color_hist_kernel(const uint8_t* __restrict__ rgb, long long n,
                                                            unsigned long long* __restrict__ hist) {
  __shared__ unsigned block_sum[4];
  const long long base = (long long)blockIdx.x * HN_HIST_TILE;                  // base < n: the grid's size
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 4) block_sum[threadIdx.x] = 0u;
  __syncthreads();
  const int common = ((rgb[3 * (size_t)base] >> 2) << 12) | ((rgb[3 * (size_t)base + 1] >> 2) << 6) |
                     (rgb[3 * (size_t)base + 2] >> 2);
  unsigned long long mine = 0ull;
  for (int j = 0; j < HN_HIST_PER_THREAD; ++j) {
    const long long i = base + (long long)j * 256 + threadIdx.x;
    int key = -1;
    unsigned long long px = 0ull;
    if (i < n) {
      const unsigned r = rgb[3 * (size_t)i], g = rgb[3 * (size_t)i + 1], b = rgb[3 * (size_t)i + 2];
      key = (int)(((r >> 2) << 12) | ((g >> 2) << 6) | (b >> 2));
      px = hn_hist_pack(r, g, b);
    }
    if (key == common) {
      mine += px;
      key = -1;
    }
    unsigned long long todo = __ballot(key >= 0);
    unsigned long long group = 0ull;                     // the sums of this lane's key, in the lane that leads it
    bool leads = false;
    while (todo != 0ull) {                               // wave-uniform: `todo` is the same in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int lead = __shfl(key, leader, 64);
      const bool in = key == lead;
      const unsigned long long same = __ballot(in) & todo;
      // `same` is wave-uniform.  A key held by one lane (the rule in a noisy frame) needs no sum; else at most 64 pixels
      // are added: no field overflows
      const unsigned long long total = (same & (same - 1ull)) == 0ull ? px : hn_wave_sum_u64(in ? px : 0ull);
      if (lane == leader) {
        group = total;
        leads = true;
      }
      todo &= ~same;
    }
    if (leads) hn_hist_add(hist, key, group);
  }
  mine = hn_wave_sum_u64(mine);
  if (lane == 0 && mine != 0ull) {
    atomicAdd(&block_sum[0], (unsigned)(mine >> (3 * HN_HIST_FIELD)));
    atomicAdd(&block_sum[1], (unsigned)(mine & HN_HIST_MASK));
    atomicAdd(&block_sum[2], (unsigned)((mine >> HN_HIST_FIELD) & HN_HIST_MASK));
    atomicAdd(&block_sum[3], (unsigned)((mine >> (2 * HN_HIST_FIELD)) & HN_HIST_MASK));
  }
  __syncthreads();
  if (threadIdx.x < 4 && block_sum[0] != 0u)
    atomicAdd(hist + 4 * (size_t)common + threadIdx.x, (unsigned long long)block_sum[threadIdx.x]);
}

extern "C" int hn_color_hist(const uint8_t* rgb_dev, long long n, unsigned long long* hist_dev, hnStream_t stream) {
  if (n <= 0 || n > 2147483648ll) return -2;
  if (rgb_dev == nullptr || hist_dev == nullptr) return -3;
  if ((uintptr_t)hist_dev % 8 != 0) return -4;
  hipLaunchKernelGGL(hn_color_hist_kernel, dim3((unsigned)((n + HN_HIST_TILE - 1) / HN_HIST_TILE)), dim3(256), 0,
                     (hipStream_t)stream, rgb_dev, n, hist_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_palette_map: index[i] = the palette entry nearest to pixel i in squared RGB distance (integers), the SMALLEST index
// among equals: entries are visited in index order and only a strictly smaller distance replaces the best so far.  The
// palette sits in LDS, one packed word per entry (every lane reads the same word: a broadcast); a thread carries
// HN_MAP_PER_THREAD pixels through the loop so that one LDS read serves four of them.
// ------------------------------------------------------------------------------------------------
#define HN_MAP_PER_THREAD 4
#define HN_MAP_TILE (256 * HN_MAP_PER_THREAD)

__global__ __launch_bounds__(256) void hn_palette_map_kernel(const uint8_t* __restrict__ rgb, long long n,
                                                             const uint8_t* __restrict__ palette, int n_colors,
                                                             uint8_t* __restrict__ index) {
  __shared__ uint32_t pal[256];
  if ((int)threadIdx.x < n_colors)
    pal[threadIdx.x] = (uint32_t)palette[3 * threadIdx.x] | ((uint32_t)palette[3 * threadIdx.x + 1] << 8) |
                       ((uint32_t)palette[3 * threadIdx.x + 2] << 16);
  __syncthreads();
  const long long base = (long long)blockIdx.x * HN_MAP_TILE + threadIdx.x;
  int r[HN_MAP_PER_THREAD], g[HN_MAP_PER_THREAD], b[HN_MAP_PER_THREAD], best[HN_MAP_PER_THREAD], arg[HN_MAP_PER_THREAD];
#pragma unroll
  for (int j = 0; j < HN_MAP_PER_THREAD; ++j) {
    const long long i = base + (long long)j * 256;
    const bool ok = i < n;
    r[j] = ok ? rgb[3 * (size_t)i] : 0;
    g[j] = ok ? rgb[3 * (size_t)i + 1] : 0;
    b[j] = ok ? rgb[3 * (size_t)i + 2] : 0;
    best[j] = 0x7fffffff;
    arg[j] = 0;
  }
  for (int k = 0; k < n_colors; ++k) {
    const uint32_t p = pal[k];
    const int pr = (int)(p & 255u), pg = (int)((p >> 8) & 255u), pb = (int)(p >> 16);
#pragma unroll
    for (int j = 0; j < HN_MAP_PER_THREAD; ++j) {
      const int dr = r[j] - pr, dg = g[j] - pg, db = b[j] - pb;
      const int d = dr * dr + dg * dg + db * db;
      if (d < best[j]) {
        best[j] = d;
        arg[j] = k;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < HN_MAP_PER_THREAD; ++j) {
    const long long i = base + (long long)j * 256;
    if (i < n) index[i] = (uint8_t)arg[j];
  }
}

extern "C" int hn_palette_map(const uint8_t* rgb_dev, long long n, const uint8_t* palette_dev, int n_colors,
                              uint8_t* index_dev, hnStream_t stream) {
  if (n <= 0 || n > 2147483648ll || n_colors < 1 || n_colors > 256) return -2;
  if (rgb_dev == nullptr || palette_dev == nullptr || index_dev == nullptr) return -3;
  hipLaunchKernelGGL(hn_palette_map_kernel, dim3((unsigned)((n + HN_MAP_TILE - 1) / HN_MAP_TILE)), dim3(256), 0,
                     (hipStream_t)stream, rgb_dev, n, palette_dev, n_colors, index_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Depth image of the validation step (utils/visualization.py:6-18).
// hn_depth_range: range[0] / range[1] = min / max of nan_to_num(depth).  Depth maps are image-sized, so ONE workgroup of
// 1024 threads strides over the map and reduces through LDS: no workspace, no atomics, nothing to zero first.  min and
// max do not depend on the order of their operands except for the sign of a zero (-0 and +0 compare equal); neither
// sign changes a pixel of hn_depth_colormap.
// ------------------------------------------------------------------------------------------------
HN_DEV float hn_nan_to_num(float d) {
  if (d != d) return 0.0f;
  if (d > FLT_MAX) return FLT_MAX;
  if (d < -FLT_MAX) return -FLT_MAX;
  return d;
}

__global__ __launch_bounds__(1024) void hn_depth_range_kernel(const float* __restrict__ depth, long long n,
                                                              float* __restrict__ range) {
  __shared__ float lo_s[16], hi_s[16];
  float lo = FLT_MAX, hi = -FLT_MAX;                    // n >= 1 and every value lies inside [-FLT_MAX, FLT_MAX]
  for (long long i = threadIdx.x; i < n; i += 1024) {
    const float d = hn_nan_to_num(depth[i]);
    lo = d < lo ? d : lo;
    hi = d > hi ? d : hi;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ol = __shfl_xor(lo, m, 64), oh = __shfl_xor(hi, m, 64);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    lo_s[threadIdx.x >> 6] = lo;
    hi_s[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) {
      lo = lo_s[w] < lo ? lo_s[w] : lo;
      hi = hi_s[w] > hi ? hi_s[w] : hi;
    }
    range[0] = lo;
    range[1] = hi;
  }
}

extern "C" int hn_depth_range(const float* depth_dev, long long n, float* range_dev, hnStream_t stream) {
  if (n <= 0 || n > 2147483648ll) return -2;
  if (depth_dev == nullptr || range_dev == nullptr) return -3;
  if ((uintptr_t)depth_dev % 4 != 0 || (uintptr_t)range_dev % 4 != 0) return -4;
  hipLaunchKernelGGL(hn_depth_range_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, depth_dev, n, range_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// hn_depth_colormap: out[i] = lut[k], k = (uint8)(255 * x) by truncation, x = (d - mi) / (ma - mi + 1e-8f) with
// d = nan_to_num(depth[i]) and (mi, ma) read from `range` on the device.  x lies in [0, 1] or is NaN (ma - mi overflowed
// to inf and d - mi did too); NaN gives k = 0.
__global__ __launch_bounds__(256) void hn_depth_colormap_kernel(const float* __restrict__ depth, long long n,
                                                                const float* __restrict__ range,
                                                                const uint8_t* __restrict__ lut,
                                                                uint8_t* __restrict__ out) {
  __shared__ uint8_t lut_s[768];
  for (int t = threadIdx.x; t < 768; t += 256) lut_s[t] = lut[t];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float mi = range[0], ma = range[1];
  const float d = hn_nan_to_num(depth[i]);
  const float x = __fdiv_rn(__fsub_rn(d, mi), __fadd_rn(__fsub_rn(ma, mi), 1e-8f));
  const float y = __fmul_rn(255.0f, x);
  int k = 0;
  if (y == y) k = y >= 255.0f ? 255 : (y > 0.0f ? (int)y : 0);
  out[3 * (size_t)i + 0] = lut_s[3 * k + 0];
  out[3 * (size_t)i + 1] = lut_s[3 * k + 1];
  out[3 * (size_t)i + 2] = lut_s[3 * k + 2];
}

extern "C" int hn_depth_colormap(const float* depth_dev, long long n, const float* range_dev, const uint8_t* lut_dev,
                                 uint8_t* out_dev, hnStream_t stream) {
  if (n <= 0 || n > 2147483648ll) return -2;
  if (depth_dev == nullptr || range_dev == nullptr || lut_dev == nullptr || out_dev == nullptr) return -3;
  if ((uintptr_t)depth_dev % 4 != 0 || (uintptr_t)range_dev % 4 != 0) return -4;
  hipLaunchKernelGGL(hn_depth_colormap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     depth_dev, n, range_dev, lut_dev, out_dev);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// hn_gif_lzw (host): GIF's variable-width LZW of an index stream with minimum code size 8.  Codes: 0..255 literals,
// 256 clear, 257 end, 258..4095 strings.  The stream opens with a clear code; a code is `width` bits (9 at a clear),
// packed least significant bit first.  After a code is sent the coder registers (sent string + next index) under the
// next free code; the decoder learns that entry one code later, so both widen after a code is sent / read when the next
// free code, counted BEFORE this code's registration, equals 1 << width (width < 12).  When all 4096 codes are taken the
// coder sends a clear code and starts over at width 9.  The dictionary is an open-addressed hash of (prefix code, index)
// pairs: 8192 slots for at most 3838 entries, emptied at every clear.
// ------------------------------------------------------------------------------------------------
namespace {
struct HnLzwOut {
  uint8_t* out;
  long long cap, len;
  uint64_t acc;
  int bits;
  bool full;
  void put(int code, int width) {
    acc |= (uint64_t)code << bits;
    bits += width;
    while (bits >= 8) {
      if (len < cap) out[len] = (uint8_t)(acc & 255u);
      else full = true;
      ++len;
      acc >>= 8;
      bits -= 8;
    }
  }
  void flush() {
    if (bits > 0) {
      if (len < cap) out[len] = (uint8_t)(acc & 255u);
      else full = true;
      ++len;
    }
    acc = 0;
    bits = 0;
  }
};
}  // namespace

extern "C" int hn_gif_lzw(const uint8_t* indices, long long n, uint8_t* out, long long capacity, long long* out_len) {
  constexpr int kClear = 256, kEnd = 257, kFirst = 258, kMaxCodes = 4096, kSlots = 8192;
  if (n < 0 || capacity < 0) return -2;
  if ((n > 0 && indices == nullptr) || (capacity > 0 && out == nullptr) || out_len == nullptr) return -3;
  static thread_local int32_t keys[kSlots];
  static thread_local int16_t vals[kSlots];
  HnLzwOut o = {out, capacity, 0, 0, 0, false};
  int width = 9, next = kFirst;
  memset(keys, 0xff, sizeof(keys));
  o.put(kClear, width);
  if (n > 0) {
    int cur = indices[0];
    for (long long i = 1; i < n; ++i) {
      const int c = indices[i];
      const int32_t key = (cur << 8) | c;
      unsigned slot = ((unsigned)key * 2654435761u) >> 19;                      // 13 bits
      while (keys[slot] != -1 && keys[slot] != key) slot = (slot + 1) & (kSlots - 1);
      if (keys[slot] == key) {
        cur = vals[slot];
        continue;
      }
      o.put(cur, width);
      if (next == (1 << width) && width < 12) ++width;
      if (next < kMaxCodes) {
        keys[slot] = key;
        vals[slot] = (int16_t)next;
        ++next;
      } else {
        o.put(kClear, width);
        memset(keys, 0xff, sizeof(keys));
        width = 9;
        next = kFirst;
      }
      cur = c;
    }
    o.put(cur, width);
    if (next == (1 << width) && width < 12) ++width;
  }
  o.put(kEnd, width);
  o.flush();
  *out_len = o.len;
  return o.full ? -6 : 0;
}
