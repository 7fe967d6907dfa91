// Device functions more than one geometry source file evaluates and whose bits they must agree on: the forward camera
// model of a 24-float camera record (hn_mesh_render.hip bins faces with it, hn_fusion.hip looks lattice points up in depth
// images with it) and the lattice every geometry kernel works on (hn_geometry.hip, hn_fusion.hip).  The library is built
// with contraction off: every product and sum below is rounded on its own, in the order written.
#pragma once
#include "hn_common.h"

#define HN_MESH_BEHIND 1           // point flag: z <= 1e-6 in the camera frame
#define HN_MESH_UNPROJECTABLE 2    // point flag: the radial map folds at its radius, or a coordinate is not finite

// ------------------------------------------------------------------------------------------------
// The forward camera model (the closed form of the system hn_nerfies_pixel_ray inverts by Newton steps): a world point
// to pixel coordinates (u, v), pixel (col i, row j) covering [i, i + 1) x [j, j + 1).  Returns the flags of the point.
// ------------------------------------------------------------------------------------------------
HN_DEV int hn_mr_project(const float* __restrict__ cam, float px, float py, float pz, float* u, float* v) {
  const float qx = px - cam[9], qy = py - cam[10], qz = pz - cam[11];
  const float xc = cam[0] * qx + cam[1] * qy + cam[2] * qz;
  const float yc = cam[3] * qx + cam[4] * qy + cam[5] * qz;
  const float zc = cam[6] * qx + cam[7] * qy + cam[8] * qz;
  *u = 0.0f;
  *v = 0.0f;
  if (zc <= 1e-6f) return HN_MESH_BEHIND;
  if (!(zc <= 3.402823466e38f)) return HN_MESH_UNPROJECTABLE;      // NaN or +inf
  const float f = cam[12], aspect = cam[13], skew = cam[14], cx = cam[15], cy = cam[16];
  const float k1 = cam[17], k2 = cam[18], k3 = cam[19], p1 = cam[20], p2 = cam[21];
  const float x = xc / zc, y = yc / zc;
  const float r = x * x + y * y;
  if (!(1.0f + r * (3.0f * k1 + r * (5.0f * k2 + r * 7.0f * k3)) > 0.0f)) return HN_MESH_UNPROJECTABLE;
  const float radial = 1.0f + r * (k1 + r * (k2 + k3 * r));
  const float xd = x * radial + 2.0f * p1 * x * y + p2 * (r + 2.0f * x * x);
  const float yd = y * radial + 2.0f * p2 * x * y + p1 * (r + 2.0f * y * y);
  const float uu = f * xd + skew * yd + cx, vv = f * aspect * yd + cy;
  if (!(fabsf(uu) <= 3.402823466e38f) || !(fabsf(vv) <= 3.402823466e38f)) return HN_MESH_UNPROJECTABLE;
  *u = uu;
  *v = vv;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Lattice: (nx, ny, nz) points over bounds (xmin, xmax, ymin, ymax, zmin, zmax), point index p = (i*ny + j)*nz + k at
// lo + (i, j, k) * step, step = (hi - lo) / (n - 1) taken once on the host.
// ------------------------------------------------------------------------------------------------
struct HnLattice {
  int nx, ny, nz;
  float lo[3], step[3];
};

// host: lo and step of a lattice; false when a side has fewer than 2 points, hi <= lo, or 7 * points overflow int32
static inline bool hn_lattice(int nx, int ny, int nz, const float* bounds, HnLattice* out) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  if ((long long)nx * ny * nz * 7 > 2147483647ll) return false;
  out->nx = nx; out->ny = ny; out->nz = nz;
  const int n[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c) {
    const float lo = bounds != nullptr ? bounds[2 * c] : 0.0f, hi = bounds != nullptr ? bounds[2 * c + 1] : 1.0f;
    if (!(hi > lo)) return false;
    out->lo[c] = lo;
    out->step[c] = (hi - lo) / (float)(n[c] - 1);
  }
  return true;
}

HN_DEV float hn_lattice_pos(const HnLattice& g, int c, int idx) { return __fadd_rn(g.lo[c], __fmul_rn((float)idx, g.step[c])); }
