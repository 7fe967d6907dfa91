// Data-path kernels of the GPU datasets (datasets/llff.py, blender.py, nerfies.py) for gfx950: ray generation for a
// whole image, the one-launch gather of a training batch, the blend onto white, and Pillow's premultiply and 8-bit
// resampling passes.  One thread per pixel or row; all of them are HBM bound.
#include "hn_common.h"

// ------------------------------------------------------------------------------------------------
// On-device ray generation (datasets/ray_utils.py:5-93 + the row layout of datasets/llff.py:244-264):
// pixel (col i, row j) -> camera direction ((i - W/2)/f, -(j - H/2)/f, -1) -> world (c2w 3x4) -> normalised;
// origin = c2w[:, 3]; optional NDC transform (near plane 1.0 in the reference's call); one thread per pixel writes
// the whole (8|9)-float ray row [o, d, near, far(, image id)] — 36 B/pixel, HBM bound.
// ------------------------------------------------------------------------------------------------
// One ray row [o, d, near, far(, id)]: `id` is read only for a 9-float row (the gather passes a null table otherwise).
__device__ __forceinline__ void hn_store_ray_row(float* r, int row_floats, const float o[3], const float d[3], float near,
                                                 float far, const float* id) {
  r[0] = o[0]; r[1] = o[1]; r[2] = o[2]; r[3] = d[0]; r[4] = d[1]; r[5] = d[2]; r[6] = near; r[7] = far;
  if (row_floats > 8) r[8] = *id;
}

// The pixel -> ray arithmetic, shared by hn_generate_rays_kernel and hn_ray_batch_kernel (one definition: a training
// batch gathers exactly the rows the whole-image launch writes).
__device__ __forceinline__ void hn_pixel_ray(int H, int W, float focal, const float* c2w, int ndc, float ndc_near, int i,
                                             int j, float o[3], float d[3]) {
  const float dx = __fdiv_rn(__fsub_rn((float)i, __fdiv_rn((float)W, 2.0f)), focal);
  const float dy = -__fdiv_rn(__fsub_rn((float)j, __fdiv_rn((float)H, 2.0f)), focal);
  const float dz = -1.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = __fadd_rn(__fadd_rn(__fmul_rn(dx, c2w[4 * k]), __fmul_rn(dy, c2w[4 * k + 1])), __fmul_rn(dz, c2w[4 * k + 2]));
    o[k] = c2w[4 * k + 3];
  }
  const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = __fdiv_rn(d[k], nrm);
  if (ndc) {   // get_ndc_rays, ray_utils.py:52-93
    const float t = __fdiv_rn(-__fadd_rn(ndc_near, o[2]), d[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = __fadd_rn(o[k], __fmul_rn(t, d[k]));
    const float ox_oz = __fdiv_rn(o[0], o[2]), oy_oz = __fdiv_rn(o[1], o[2]);
    const float sx = __fdiv_rn(-1.0f, __fdiv_rn((float)W, __fmul_rn(2.0f, focal)));
    const float sy = __fdiv_rn(-1.0f, __fdiv_rn((float)H, __fmul_rn(2.0f, focal)));
    const float o0 = __fmul_rn(sx, ox_oz), o1 = __fmul_rn(sy, oy_oz);
    const float o2 = __fadd_rn(1.0f, __fdiv_rn(__fmul_rn(2.0f, ndc_near), o[2]));
    const float d0 = __fmul_rn(sx, __fsub_rn(__fdiv_rn(d[0], d[2]), ox_oz));
    const float d1 = __fmul_rn(sy, __fsub_rn(__fdiv_rn(d[1], d[2]), oy_oz));
    const float d2 = __fsub_rn(1.0f, o2);
    o[0] = o0; o[1] = o1; o[2] = o2; d[0] = d0; d[1] = d1; d[2] = d2;
  }
}

__global__ void hn_generate_rays_kernel(int H, int W, float focal, const float* c2w, int ndc, float ndc_near,
                                        float near, float far, float image_id, int row_floats, float* rays) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int j = pix / W, i = pix - j * W;
  float d[3], o[3];
  hn_pixel_ray(H, W, focal, c2w, ndc, ndc_near, i, j, o, d);
  hn_store_ray_row(rays + (size_t)pix * row_floats, row_floats, o, d, near, far, &image_id);
}

extern "C" int hn_generate_rays(int H, int W, float focal, const float* c2w, int ndc, float ndc_near, float near,
                                float far, float image_id, int row_floats, float* rays, hnStream_t stream) {
  if (H <= 0 || W <= 0 || !(focal > 0.0f) || (row_floats != 8 && row_floats != 9)) return -2;
  if (c2w == nullptr || rays == nullptr) return -3;
  const int n = H * W;
  hipLaunchKernelGGL(hn_generate_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, H, W, focal,
                     c2w, ndc, ndc_near, near, far, image_id, row_floats, rays);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Rays of a Nerfies-format capture (datasets/nerfies.py): every image has its own camera with a principal point, skew,
// a pixel aspect ratio and radial + tangential lens distortion.  `cam` is that image's record of HN_NERFIES_CAM_FLOATS
// floats: orientation (9, world to camera, rows), position (3), f, aspect, skew, cx, cy, k1, k2, k3, p1, p2, two zeros.
// Pixel (col i, row j) has its centre at (i + 0.5, j + 0.5):
//   y = (j + 0.5 - cy) / (f aspect);  x = (i + 0.5 - cx - y skew) / f;  (x, y) <- undistort(x, y)
//   d = normalise(orientation^T normalise((x, y, 1)));  o = position
// undistort is 10 Newton steps from (x, y) = (xd, yd) on  D x + 2 p1 x y + p2 (r + 2 x^2) = xd,
// D y + 2 p2 x y + p1 (r + 2 y^2) = yd  with r = x^2 + y^2, D = 1 + r (k1 + r (k2 + k3 r)); a step whose determinant
// is within 1e-9 of zero moves nothing.  It is skipped for a camera without distortion (one branch per image).
// Shared by hn_generate_rays_nerfies_kernel and the Nerfies instance of hn_ray_batch_kernel; every operation is rounded
// on its own, so that both write the same bits whatever either inlining context would contract.
// ------------------------------------------------------------------------------------------------
#define HN_NERFIES_NEWTON_STEPS 10

__device__ __forceinline__ void hn_nerfies_pixel_ray(const float* cam, int i, int j, float o[3], float d[3]) {
  const float f = cam[12], aspect = cam[13], skew = cam[14], cx = cam[15], cy = cam[16];
  const float k1 = cam[17], k2 = cam[18], k3 = cam[19], p1 = cam[20], p2 = cam[21];
  float y = __fdiv_rn(__fsub_rn(__fadd_rn((float)j, 0.5f), cy), __fmul_rn(f, aspect));
  float x = __fdiv_rn(__fsub_rn(__fsub_rn(__fadd_rn((float)i, 0.5f), cx), __fmul_rn(y, skew)), f);
  if (k1 != 0.0f || k2 != 0.0f || k3 != 0.0f || p1 != 0.0f || p2 != 0.0f) {
    const float xd = x, yd = y;
    for (int it = 0; it < HN_NERFIES_NEWTON_STEPS; ++it) {
      const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), xy = __fmul_rn(x, y);
      const float r = __fadd_rn(xx, yy);
      const float D = __fadd_rn(1.0f, __fmul_rn(r, __fadd_rn(k1, __fmul_rn(r, __fadd_rn(k2, __fmul_rn(k3, r))))));
      const float fx = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(D, x), __fmul_rn(__fmul_rn(2.0f, p1), xy)),
                                           __fmul_rn(p2, __fadd_rn(r, __fmul_rn(2.0f, xx)))), xd);
      const float fy = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(D, y), __fmul_rn(__fmul_rn(2.0f, p2), xy)),
                                           __fmul_rn(p1, __fadd_rn(r, __fmul_rn(2.0f, yy)))), yd);
      const float D_r = __fadd_rn(k1, __fmul_rn(r, __fadd_rn(__fmul_rn(2.0f, k2), __fmul_rn(__fmul_rn(3.0f, k3), r))));
      const float D_x = __fmul_rn(__fmul_rn(2.0f, x), D_r), D_y = __fmul_rn(__fmul_rn(2.0f, y), D_r);
      const float fx_x = __fadd_rn(__fadd_rn(__fadd_rn(D, __fmul_rn(D_x, x)), __fmul_rn(__fmul_rn(2.0f, p1), y)),
                                   __fmul_rn(__fmul_rn(6.0f, p2), x));
      const float fx_y = __fadd_rn(__fadd_rn(__fmul_rn(D_y, x), __fmul_rn(__fmul_rn(2.0f, p1), x)),
                                   __fmul_rn(__fmul_rn(2.0f, p2), y));
      const float fy_x = __fadd_rn(__fadd_rn(__fmul_rn(D_x, y), __fmul_rn(__fmul_rn(2.0f, p2), y)),
                                   __fmul_rn(__fmul_rn(2.0f, p1), x));
      const float fy_y = __fadd_rn(__fadd_rn(__fadd_rn(D, __fmul_rn(D_y, y)), __fmul_rn(__fmul_rn(2.0f, p2), x)),
                                   __fmul_rn(__fmul_rn(6.0f, p1), y));
      const float den = __fsub_rn(__fmul_rn(fy_x, fx_y), __fmul_rn(fx_x, fy_y));
      if (fabsf(den) > 1e-9f) {
        x = __fadd_rn(x, __fdiv_rn(__fsub_rn(__fmul_rn(fx, fy_y), __fmul_rn(fy, fx_y)), den));
        y = __fadd_rn(y, __fdiv_rn(__fsub_rn(__fmul_rn(fy, fx_x), __fmul_rn(fx, fy_x)), den));
      }
    }
  }
  const float ln = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), 1.0f));
  const float lx = __fdiv_rn(x, ln), ly = __fdiv_rn(y, ln), lz = __fdiv_rn(1.0f, ln);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = __fadd_rn(__fadd_rn(__fmul_rn(cam[k], lx), __fmul_rn(cam[3 + k], ly)), __fmul_rn(cam[6 + k], lz));
    o[k] = cam[9 + k];
  }
  const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = __fdiv_rn(d[k], nrm);
}

__global__ void hn_generate_rays_nerfies_kernel(int H, int W, const float* cam, float near, float far, float image_id,
                                                int row_floats, float* rays) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int j = pix / W, i = pix - j * W;
  float d[3], o[3];
  hn_nerfies_pixel_ray(cam, i, j, o, d);
  hn_store_ray_row(rays + (size_t)pix * row_floats, row_floats, o, d, near, far, &image_id);
}

extern "C" int hn_generate_rays_nerfies(int H, int W, const float* cam, float near, float far, float image_id,
                                        int row_floats, float* rays, hnStream_t stream) {
  if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || (row_floats != 8 && row_floats != 9)) return -2;
  if (cam == nullptr || rays == nullptr) return -3;
  const int n = H * W;
  hipLaunchKernelGGL(hn_generate_rays_nerfies_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, H, W,
                     cam, near, far, image_id, row_floats, rays);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// One training batch of an LLFF dataset gathered on the device (datasets/llff.py's all_rays / all_rgbs rows, in the
// order a shuffled DataLoader reads them).  state[0] is the cursor into `perm`, state[1] an arrival counter, state[2]
// an error flag: every workgroup reads the cursor, then arrives; the last to arrive advances the cursor by `batch` and
// clears the counter, so nothing returns to the host and the launch replays inside a captured graph.  A ray index g
// decodes to training slot g / (H*W) and pixel g % (H*W); the row comes from hn_pixel_ray with that slot's c2w, the
// colour from the uint8 stack as u8 / 255 (torchvision's ToTensor: a division, rounded once).  A position past the end
// of `perm`, or an index outside the dataset, writes a NaN row and colour and sets the error flag (the host checks it
// once per epoch): nothing is read out of bounds and a bookkeeping error cannot pass as a plausible batch.
//
// CH = 3: the LLFF stack above.  CH = 4: a Blender stack of RGBA pixels (datasets/blender.py:57-58): the pixel is one
// aligned 32-bit load and the colour is its blend onto white, hn_blend_white — the definition hn_blend_white_u8 uses.
//
// NERFIES = true: a Nerfies capture (datasets/nerfies.py).  `c2w` is then the (n_images, HN_NERFIES_CAM_FLOATS) camera
// table and the row comes from hn_nerfies_pixel_ray with that slot's record; focal, ndc and ndc_near are not read.
// The cursor, the arrival counter, the error flag, the NaN rows and the colour are this one definition for all three.
// ------------------------------------------------------------------------------------------------
// An RGBA pixel (little endian: R in the low byte, A in the high one) blended onto white as the reference does on
// ToTensor values: x = c / 255 and al = a / 255 (divisions, rounded once), then x * al, 1 - al and their sum as three
// separately rounded operations (a fused multiply-add differs in the last bit for about one pixel in ten).
__device__ __forceinline__ void hn_blend_white(uint32_t px, float c[3]) {
  const float al = __fdiv_rn((float)(px >> 24), 255.0f);
  const float rest = __fsub_rn(1.0f, al);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = __fadd_rn(__fmul_rn(__fdiv_rn((float)((px >> (8 * k)) & 0xffu), 255.0f), al), rest);
}

template <int CH, bool NERFIES>
__global__ __launch_bounds__(256) void hn_ray_batch_kernel(const int64_t* perm, long long n_perm,
        unsigned long long* state, int batch, long long n_rays, int H, int W, float focal, const float* c2w,
        const float* image_ids, int ndc, float ndc_near, float near, float far, int row_floats, const uint8_t* rgb8,
        float* rays, float* rgbs) {
  __shared__ long long s_cur;
  if (threadIdx.x == 0) s_cur = (long long)state[0];
  __syncthreads();
  const long long cur = s_cur;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row < batch) {
    const long long p = cur + row;
    const long long g = (p >= 0 && p < n_perm) ? perm[p] : -1;
    float* r = rays + (size_t)row * row_floats;
    float* c = rgbs + (size_t)row * 3;
    if (g < 0 || g >= n_rays) {
      const float nan = __int_as_float(0x7fc00000);
      for (int k = 0; k < row_floats; ++k) r[k] = nan;
      c[0] = nan; c[1] = nan; c[2] = nan;
      __hip_atomic_store(&state[2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      const long long hw = (long long)H * W;
      const int slot = (int)(g / hw);
      const int pix = (int)(g - (long long)slot * hw);
      const int j = pix / W, i = pix - j * W;
      float d[3], o[3];
      if (NERFIES)
        hn_nerfies_pixel_ray(c2w + (size_t)HN_NERFIES_CAM_FLOATS * slot, i, j, o, d);
      else
        hn_pixel_ray(H, W, focal, c2w + 12 * slot, ndc, ndc_near, i, j, o, d);
      hn_store_ray_row(r, row_floats, o, d, near, far, image_ids + slot);
      if (CH == 4) {
        float col[3];
        hn_blend_white(reinterpret_cast<const uint32_t*>(rgb8)[g], col);
        c[0] = col[0]; c[1] = col[1]; c[2] = col[2];
      } else {
        const uint8_t* px = rgb8 + 3 * g;
        c[0] = __fdiv_rn((float)px[0], 255.0f);
        c[1] = __fdiv_rn((float)px[1], 255.0f);
        c[2] = __fdiv_rn((float)px[2], 255.0f);
      }
    }
  }
  __syncthreads();                 // every lane of this workgroup has consumed the cursor
  if (threadIdx.x == 0) {
    const unsigned long long arrived =
        __hip_atomic_fetch_add(&state[1], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == gridDim.x - 1) {                                        // the last workgroup: no one reads it now
      __hip_atomic_store(&state[1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&state[0], (unsigned long long)(cur + batch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int CH, bool NERFIES>
static int hn_ray_batch_launch(const int64_t* perm, long long n_perm, unsigned long long* state, int batch,
                               long long n_rays, int H, int W, float focal, const float* c2w, const float* image_ids,
                               int ndc, float ndc_near, float near, float far, int row_floats, const uint8_t* px8,
                               float* rays, float* rgbs, hnStream_t stream) {
  if (batch <= 0 || n_perm <= 0 || n_rays <= 0 || H <= 0 || W <= 0 || (!NERFIES && !(focal > 0.0f)) ||
      (row_floats != 8 && row_floats != 9))
    return -2;
  if (n_rays % ((long long)H * W) != 0) return -2;
  if (perm == nullptr || state == nullptr || c2w == nullptr || px8 == nullptr || rays == nullptr || rgbs == nullptr ||
      (row_floats == 9 && image_ids == nullptr))
    return -3;
  if (CH == 4 && (reinterpret_cast<uintptr_t>(px8) & 3u) != 0) return -3;      // pixels are read as 32-bit words
  hipLaunchKernelGGL((hn_ray_batch_kernel<CH, NERFIES>), dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, perm,
                     n_perm, state, batch, n_rays, H, W, focal, c2w, image_ids, ndc, ndc_near, near, far, row_floats,
                     px8, rays, rgbs);
  HN_CHECK_LAUNCH();
  return 0;
}

extern "C" int hn_ray_batch(const int64_t* perm, long long n_perm, unsigned long long* state, int batch,
                            long long n_rays, int H, int W, float focal, const float* c2w, const float* image_ids,
                            int ndc, float ndc_near, float near, float far, int row_floats, const uint8_t* rgb8,
                            float* rays, float* rgbs, hnStream_t stream) {
  return hn_ray_batch_launch<3, false>(perm, n_perm, state, batch, n_rays, H, W, focal, c2w, image_ids, ndc, ndc_near, near,
                                far, row_floats, rgb8, rays, rgbs, stream);
}

extern "C" int hn_ray_batch_rgba(const int64_t* perm, long long n_perm, unsigned long long* state, int batch,
                                 long long n_rays, int H, int W, float focal, const float* c2w,
                                 const float* image_ids, int ndc, float ndc_near, float near, float far,
                                 int row_floats, const uint8_t* rgba8, float* rays, float* rgbs, hnStream_t stream) {
  return hn_ray_batch_launch<4, false>(perm, n_perm, state, batch, n_rays, H, W, focal, c2w, image_ids, ndc, ndc_near, near,
                                far, row_floats, rgba8, rays, rgbs, stream);
}

extern "C" int hn_ray_batch_nerfies(const int64_t* perm, long long n_perm, unsigned long long* state, int batch,
                                    long long n_rays, int H, int W, const float* cams, const float* image_ids,
                                    float near, float far, int row_floats, const uint8_t* rgb8, float* rays,
                                    float* rgbs, hnStream_t stream) {
  return hn_ray_batch_launch<3, true>(perm, n_perm, state, batch, n_rays, H, W, 0.0f, cams, image_ids, 0, 0.0f, near,
                                      far, row_floats, rgb8, rays, rgbs, stream);
}

// ------------------------------------------------------------------------------------------------
// (N, 4) uint8 RGBA -> (N, 3) fp32 blended onto white (hn_blend_white) and, when `mask` is given, (N,) bytes a > 0
// (the reference's valid_mask, datasets/blender.py:93).  One thread per pixel, one aligned 32-bit load.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_blend_white_u8_kernel(const uint32_t* rgba, long long n, float* rgbs,
                                                                 uint8_t* mask) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n) return;
  const uint32_t px = rgba[id];
  float c[3];
  hn_blend_white(px, c);
  float* o = rgbs + 3 * id;
  o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  if (mask != nullptr) mask[id] = (uint8_t)((px >> 24) != 0u);
}

extern "C" int hn_blend_white_u8(const uint8_t* rgba8, long long n, float* rgbs, uint8_t* mask, hnStream_t stream) {
  if (n <= 0 || (n + 255) / 256 > 0x7fffffffLL) return -2;
  if (rgba8 == nullptr || rgbs == nullptr || (reinterpret_cast<uintptr_t>(rgba8) & 3u) != 0) return -3;
  hipLaunchKernelGGL(hn_blend_white_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(rgba8), n, rgbs, mask);
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Pillow's RGBA <-> RGBa conversions around a resize of an RGBA image (Image.resize converts to premultiplied alpha,
// resamples, converts back; Convert.c rgbA2rgba / rgba2rgbA).  inverse = 0: c' = MULDIV255(c, a) = ((t >> 8) + t) >> 8
// with t = c * a + 128.  inverse = 1: a == 0 or a == 255 keeps the bytes, else c = min(255, 255 * c' / a) (integer
// division).  Alpha is unchanged either way.  One thread per pixel, one aligned 32-bit load and store; in == out is
// allowed.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_premultiply_u8_kernel(const uint32_t* in, long long n, int inverse,
                                                                 uint32_t* out) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n) return;
  const uint32_t px = in[id];
  const uint32_t a = px >> 24;
  uint32_t res = px & 0xff000000u;
  if (!inverse) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t t = ((px >> (8 * k)) & 0xffu) * a + 128u;
      res |= ((((t >> 8) + t) >> 8) & 0xffu) << (8 * k);
    }
  } else if (a == 0u || a == 255u) {
    res = px;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t v = (255u * ((px >> (8 * k)) & 0xffu)) / a;
      res |= (v > 255u ? 255u : v) << (8 * k);
    }
  }
  out[id] = res;
}

extern "C" int hn_premultiply_u8(const uint8_t* in, long long n, int inverse, uint8_t* out, hnStream_t stream) {
  if (n <= 0 || (n + 255) / 256 > 0x7fffffffLL) return -2;
  if (in == nullptr || out == nullptr || ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) != 0)
    return -3;
  hipLaunchKernelGGL(hn_premultiply_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(in), n, inverse, reinterpret_cast<uint32_t*>(out));
  HN_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// One pass of Pillow's 8-bit resampling (Image.resize, ImagingResampleHorizontal_8bpc / Vertical_8bpc): out[x] =
// clamp(((1 << 21) + sum_k in[bounds[x].min + k] * kk[x][k]) >> 22, 0, 255) per channel, int32 coefficients with 22
// fraction bits from the host (the coefficient tables are float64 host math).  vertical = 0: (rows, cols, C) ->
// (rows, out_len, C) along the columns; vertical = 1: (rows, cols, C) -> (out_len, cols, C) along the rows.
// The sum wraps modulo 2^32 as Pillow's int32 does.  One thread per output pixel, all channels.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hn_resample_u8_kernel(const uint8_t* in, int rows, int cols, int channels,
        int out_len, int vertical, const int32_t* bounds, const int32_t* kk, int ksize, uint8_t* out) {
  const int out_rows = vertical ? out_len : rows, out_cols = vertical ? cols : out_len;
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)out_rows * out_cols) return;
  const int y = (int)(id / out_cols), x = (int)(id - (long long)y * out_cols);
  const int o = vertical ? y : x;
  const int lo = bounds[2 * o], n = bounds[2 * o + 1];
  const int32_t* k = kk + (size_t)o * ksize;
  const long long step = vertical ? (long long)cols * channels : channels;
  const uint8_t* src = vertical ? in + ((long long)lo * cols + x) * channels : in + ((long long)y * cols + lo) * channels;
  for (int c = 0; c < channels; ++c) {
    uint32_t ss = 1u << 21;
    for (int t = 0; t < n; ++t) ss += (uint32_t)src[t * step + c] * (uint32_t)k[t];
    const int v = ((int32_t)ss) >> 22;
    out[id * channels + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

extern "C" int hn_resample_u8(const uint8_t* in, int rows, int cols, int channels, int out_len, int vertical,
                              const int32_t* bounds, const int32_t* kk, int ksize, uint8_t* out, hnStream_t stream) {
  if (rows <= 0 || cols <= 0 || channels <= 0 || channels > 4 || out_len <= 0 || ksize <= 0) return -2;
  if (in == nullptr || bounds == nullptr || kk == nullptr || out == nullptr) return -3;
  const long long n = (long long)(vertical ? out_len : rows) * (vertical ? cols : out_len);
  hipLaunchKernelGGL(hn_resample_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in,
                     rows, cols, channels, out_len, vertical, bounds, kk, ksize, out);
  HN_CHECK_LAUNCH();
  return 0;
}
