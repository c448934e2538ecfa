// kitti_overlap_math.h -- the three box overlaps of the KITTI object evaluator (reference
// tools/kitti-eval/evaluate_object_3d_offline.cpp: imageBoxOverlap :227-261, toPolygon :268-291, groundBoxOverlap
// :294-314, box3DOverlap :317-344), shared by the host evaluator (kitti_eval.cpp) and the HIP kernels (kitti_eval.hip),
// in the style of pose_math.h / metric_math.h / kpt_metric_math.h.  float64 throughout, contraction off.
//
// A box is EGN_KITTI_BOX doubles: x1 y1 x2 y2 alpha h w l t1 t2 t3 ry (the numeric fields of a label line from the 2D
// box on, alpha moved behind it).
//
// The reference needs Boost.Geometry for one thing, the intersection area of two rotated rectangles.  Here the
// detection's four corners are expressed in the frame of the ground-truth box -- centred on it and turned by its ry,
// so the ground truth is the axis-aligned rectangle |x| <= |l|/2, |z| <= |w|/2 and every coordinate is at box scale,
// not scene scale -- and clipped against its four sides (Sutherland-Hodgman on a convex polygon: at most 8 vertices).
// The half-plane tests do not depend on the orientation of either corner list and the area is taken absolute, so
// labels with l = w = -1 (DontCare rows) are ordinary input.  Two identical boxes give the rectangle back exactly: the
// relative angle is 0, the clip keeps all four corners and the triangle fan sums l*w + l*w.
//
// Departures from the reference's arithmetic, each at most one rounding:
//   * the union of two rectangles is area_d + area_g - inter (Boost's union_ polygon has that area whenever the
//     intersection is not empty; with an empty one the overlap is 0 under every criterion)
//   * a volume is (l * w) * h, the same product order as inter_area * height, so that identical boxes give 1
#pragma once
#include "pose_math.h"

#define EGN_KITTI_BOX 12
#define EGN_KB_X1 0
#define EGN_KB_Y1 1
#define EGN_KB_X2 2
#define EGN_KB_Y2 3
#define EGN_KB_ALPHA 4
#define EGN_KB_H 5
#define EGN_KB_W 6
#define EGN_KB_L 7
#define EGN_KB_T1 8
#define EGN_KB_T2 9
#define EGN_KB_T3 10
#define EGN_KB_RY 11

// toPolygon: corners (l/2, w/2), (l/2, -w/2), (-l/2, -w/2), (-l/2, w/2) turned by [[cos ry, sin ry], [-sin ry, cos ry]]
// and moved by (t1, t3).  xy[4][2].
EGN_HD inline void egn_kitti_bev_corners(double l, double w, double t1, double t3, double ry, double* xy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double c = cos(ry), s = sin(ry);
  const double hl = l / 2, hw = w / 2;
  const double cx[4] = {hl, hl, -hl, -hl};
  const double cz[4] = {hw, -hw, -hw, hw};
  for (int k = 0; k < 4; ++k) {
    xy[2 * k] = c * cx[k] + s * cz[k] + t1;
    xy[2 * k + 1] = -s * cx[k] + c * cz[k] + t3;
  }
}

// Keeps the part of the convex polygon in[n][2] with sign * p[axis] <= h.  out holds up to n + 1 vertices.
EGN_HD inline int egn_kitti_clip_side(const double* in, int n, int axis, double sign, double h, double* out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  int m = 0;
  for (int k = 0; k < n; ++k) {
    const double* a = in + 2 * k;
    const double* b = in + 2 * (k + 1 == n ? 0 : k + 1);
    const double va = sign * a[axis], vb = sign * b[axis];
    const bool ina = va <= h, inb = vb <= h;
    if (ina) {
      out[2 * m] = a[0];
      out[2 * m + 1] = a[1];
      ++m;
    }
    if (ina != inb) {
      const double t = (h - va) / (vb - va);
      out[2 * m + axis] = sign * h;
      out[2 * m + 1 - axis] = a[1 - axis] + t * (b[1 - axis] - a[1 - axis]);
      ++m;
    }
  }
  return m;
}

// Area of the intersection of the bird's-eye-view rectangles of two boxes (>= 0).
EGN_HD inline double egn_kitti_bev_intersection(const double* d, const double* g) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double cg = cos(g[EGN_KB_RY]), sg = sin(g[EGN_KB_RY]);
  const double ox = d[EGN_KB_T1] - g[EGN_KB_T1], oz = d[EGN_KB_T3] - g[EGN_KB_T3];
  // the inverse of toPolygon's rotation by g's ry, applied to the offset of the centres
  const double px = cg * ox - sg * oz, pz = sg * ox + cg * oz;
  double p[16], q[16];
  egn_kitti_bev_corners(d[EGN_KB_L], d[EGN_KB_W], px, pz, d[EGN_KB_RY] - g[EGN_KB_RY], p);
  const double hl = fabs(g[EGN_KB_L] / 2), hw = fabs(g[EGN_KB_W] / 2);
  int n = egn_kitti_clip_side(p, 4, 0, 1.0, hl, q);
  n = egn_kitti_clip_side(q, n, 0, -1.0, hl, p);
  n = egn_kitti_clip_side(p, n, 1, 1.0, hw, q);
  n = egn_kitti_clip_side(q, n, 1, -1.0, hw, p);
  double twice = 0.0;                                   // triangle fan around the first vertex
  for (int k = 1; k + 1 < n; ++k) {
    const double ax = p[2 * k] - p[0], az = p[2 * k + 1] - p[1];
    const double bx = p[2 * k + 2] - p[0], bz = p[2 * k + 3] - p[1];
    twice = twice + (ax * bz - az * bx);
  }
  return fabs(twice) / 2;
}

// criterion -1: over the union; 0: over a (the detection); 1: over b (the ground truth)
EGN_HD inline double egn_kitti_ratio(double inter, double a, double b, int criterion) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (!(inter > 0)) return 0.0;
  return criterion == -1 ? inter / (a + b - inter) : (criterion == 0 ? inter / a : inter / b);
}

EGN_HD inline double egn_kitti_image_overlap(const double* a, const double* b, int criterion) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double w = fmin(a[EGN_KB_X2], b[EGN_KB_X2]) - fmax(a[EGN_KB_X1], b[EGN_KB_X1]);
  const double h = fmin(a[EGN_KB_Y2], b[EGN_KB_Y2]) - fmax(a[EGN_KB_Y1], b[EGN_KB_Y1]);
  if (w <= 0 || h <= 0) return 0.0;
  const double inter = w * h;
  const double area_a = (a[EGN_KB_X2] - a[EGN_KB_X1]) * (a[EGN_KB_Y2] - a[EGN_KB_Y1]);
  const double area_b = (b[EGN_KB_X2] - b[EGN_KB_X1]) * (b[EGN_KB_Y2] - b[EGN_KB_Y1]);
  return criterion == -1 ? inter / (area_a + area_b - inter) : (criterion == 0 ? inter / area_a : inter / area_b);
}

EGN_HD inline double egn_kitti_ground_overlap_from(double inter, const double* d, const double* g, int criterion) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return egn_kitti_ratio(inter, d[EGN_KB_L] * d[EGN_KB_W], g[EGN_KB_L] * g[EGN_KB_W], criterion);
}

EGN_HD inline double egn_kitti_box3d_overlap_from(double inter, const double* d, const double* g, int criterion) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double ymax = fmin(d[EGN_KB_T2], g[EGN_KB_T2]);
  const double ymin = fmax(d[EGN_KB_T2] - d[EGN_KB_H], g[EGN_KB_T2] - g[EGN_KB_H]);
  const double vol = inter * fmax(0.0, ymax - ymin);
  return egn_kitti_ratio(vol, d[EGN_KB_L] * d[EGN_KB_W] * d[EGN_KB_H], g[EGN_KB_L] * g[EGN_KB_W] * g[EGN_KB_H],
                         criterion);
}

// All of it for one (detection, ground truth) pair: out[0] image, out[1] ground, out[2] 3D overlap under the
// criterion, out[3] the bird's-eye-view intersection area.
EGN_HD inline void egn_kitti_overlaps(const double* d, const double* g, int criterion, double* out) {
  const double inter = egn_kitti_bev_intersection(d, g);
  out[0] = egn_kitti_image_overlap(d, g, criterion);
  out[1] = egn_kitti_ground_overlap_from(inter, d, g, criterion);
  out[2] = egn_kitti_box3d_overlap_from(inter, d, g, criterion);
  out[3] = inter;
}
