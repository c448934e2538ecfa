// overlay_math.h -- the definition of the overlay rasteriser (overlay.hip): one primitive, the capsule, blended into
// an 8-bit RGB pixel.  float64 throughout and never contracted, so the kernel and the plain host loop execute the same
// IEEE operations and give the same bytes.  No HIP-only construct.
//
// A primitive is six floats (x0 y0 x1 y1 r a) and a colour word R | G << 8 | B << 16: the segment (x0,y0)-(x1,y1)
// widened by the radius r, at opacity a (clamped to [0, 1]).  A zero-length segment is a disc.  Pixel (x, y) has its
// centre at the integer coordinates.  For one pixel and one primitive:
//     t = clamp(((p - p0) . (p1 - p0)) / |p1 - p0|^2, 0, 1)       (0 for a zero-length segment)
//     d = |p - p0 - t (p1 - p0)|
//     c = antialias ? clamp(r + 0.5 - d, 0, 1) : (d <= r ? 1 : 0)
//     w = c a;   if w > 0, per channel:  v = floor(v + (col - v) w + 0.5), stored as uint8
// The pixel is 8-bit between primitives, so primitives applied in list order define the picture whatever the
// implementation's chunking.  A primitive with a non-finite field or r < 0 is dropped.
#pragma once
#include <math.h>
#include <stdint.h>
#include "pose_math.h"   // EGN_HD

#define EGN_OVERLAY_FIELDS 6

struct egn_overlay_prim {   // one primitive widened to double, with what does not depend on the pixel
  double x0, y0, dx, dy, len2, r, a;
  // the box outside which no pixel can get w > 0 (egn_overlay_reach)
  double xlo, xhi, ylo, yhi;
  uint32_t col;
};

EGN_HD inline bool egn_overlay_finite(float v) { return fabsf(v) <= 3.4028234e38f; }   // false for NaN and inf

EGN_HD inline bool egn_overlay_valid(const float* p) {
  for (int k = 0; k < EGN_OVERLAY_FIELDS; ++k)
    if (!egn_overlay_finite(p[k])) return false;
  return p[4] >= 0.0f;
}

// How far from its segment's bounding box a primitive can reach: w > 0 needs the COMPUTED distance below r + 0.5.  The
// computed distance differs from the true one by a few roundings of terms as large as the coordinates (pixel
// coordinates stay below 2^31: the "+ 1"), so the margin carries 1e-9 of their magnitudes -- a factor of 1e6 over
// float64's 1e-16 -- and every cull by this box is conservative: culled and unculled loops give the same bytes, also
// for end points at 1e9.  float32 fields cannot overflow any float64 product below.
EGN_HD inline double egn_overlay_reach(const float* p) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double mag = fabs((double)p[0]) + fabs((double)p[1]) + fabs((double)p[2]) + fabs((double)p[3]) + (double)p[4];
  return (double)p[4] + 0.5 + 1.0 + 1e-9 * mag;
}

EGN_HD inline egn_overlay_prim egn_overlay_load(const float* p, uint32_t col) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  egn_overlay_prim q;
  const double x1 = (double)p[2], y1 = (double)p[3];
  q.x0 = (double)p[0];
  q.y0 = (double)p[1];
  q.dx = x1 - q.x0;
  q.dy = y1 - q.y0;
  q.len2 = q.dx * q.dx + q.dy * q.dy;
  q.r = (double)p[4];
  const double a = (double)p[5];
  q.a = a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a);
  const double g = egn_overlay_reach(p);
  q.xlo = (q.x0 < x1 ? q.x0 : x1) - g;
  q.xhi = (q.x0 < x1 ? x1 : q.x0) + g;
  q.ylo = (q.y0 < y1 ? q.y0 : y1) - g;
  q.yhi = (q.y0 < y1 ? y1 : q.y0) + g;
  q.col = col;
  return q;
}

// can a pixel of the rectangle [xa, xb] x [ya, yb] (pixel coordinates as doubles) get w > 0 ?
EGN_HD inline bool egn_overlay_reaches(const egn_overlay_prim& q, double xa, double xb, double ya, double yb) {
  return q.xlo <= xb && q.xhi >= xa && q.ylo <= yb && q.yhi >= ya;
}

// w of pixel (x, y)
EGN_HD inline double egn_overlay_weight(const egn_overlay_prim& q, double x, double y, int antialias) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double px = x - q.x0, py = y - q.y0;
  double t = q.len2 > 0.0 ? (px * q.dx + py * q.dy) / q.len2 : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double ex = px - t * q.dx, ey = py - t * q.dy;
  const double d = sqrt(ex * ex + ey * ey);
  double c;
  if (antialias) {
    c = q.r + 0.5 - d;
    c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
  } else {
    c = d <= q.r ? 1.0 : 0.0;
  }
  return c * q.a;
}

// one channel: v (0..255) towards col (0..255) by w in (0, 1]
EGN_HD inline unsigned egn_overlay_blend(unsigned v, unsigned col, double w) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double vd = (double)v;
  const double out = vd + ((double)col - vd) * w;
  return (unsigned)floor(out + 0.5);
}
