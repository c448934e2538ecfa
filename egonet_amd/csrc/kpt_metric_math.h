// kpt_metric_math.h -- per-instance math of the key-point model's source-image metric (reference
// libs/metric/criterions.py:17-37 get_distance, :57-66 get_PCK, :68-143 get_distance_src; the crop affine of
// libs/common/img_proc.py:26-78), shared by the HIP kernel (kpt_metrics.hip) and by the host-compiled unit harness
// (tests/kpt_metric_math_harness.cpp, built with g++), in the style of metric_math.h.
//
// Per labelled instance: centre [2], scale [2] (x 200 px), rotation in degrees, K annotated joints [K][3] (x, y,
// visibility), all float64; per joint a float32 prediction in the pixels of the crop window (img_w x img_h).
//   1. the INVERSE crop affine (window -> image), float64, from the reference's three point pairs held in float32
//   2. the source point of the prediction, its distance to the annotated joint
//   3. per visible joint (visibility != 0): count, distance and distance < {0.1, 0.2, 0.3} x denominator, where the
//      denominator is (max y - min y) / 3 over ALL K annotated joints of the instance, invisible ones too (get_PCK)
// Every float64 function switches contraction off: products and sums round separately, like numpy's, on both builds.
#pragma once
#include "pose_math.h"

#define EGN_KPT_METRIC_STATS 5          // count, sum of distances, pck[3]

// get_affine_transform(center, scale, rot, (img_h, img_w), inv=1) in closed form: T[6] = row-major 2 x 3.
// The three-point construction with the points in float32 (img_proc.py:45-60): the centre, the point half a source
// width "above" it turned by rot, and the right-angle completion b + perp(a - b) of the two -- in the image (src) and
// in the window (dst).  cv2.getAffineTransform solves the 6 x 6 system; with A = [p1 - p0, p2 - p0] of the window and
// B the same of the image, the map is L = B A^-1, t = b0 - L a0 (Cramer on the 2 x 2).
EGN_HD inline void egn_kpt_inv_affine(const double* center, const double* scale, double rot_deg, double img_w,
                                      double img_h, double* T) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double rad = 3.141592653589793 * rot_deg / 180.0;
  const double up = -0.5 * (scale[0] * 200.0);
  const double dir_x = -up * sin(rad), dir_y = up * cos(rad);
  // image triangle, float32
  const float s0x = (float)center[0], s0y = (float)center[1];
  const float s1x = (float)(center[0] + dir_x), s1y = (float)(center[1] + dir_y);
  const float sdx = s0x - s1x, sdy = s0y - s1y;
  const float s2x = s1x + (-sdy), s2y = s1y + sdx;
  // window triangle, float32
  const float d0x = (float)(img_w * 0.5), d0y = (float)(img_h * 0.5);
  const float d1x = (float)(img_w * 0.5 + (double)0.0f), d1y = (float)(img_h * 0.5 + (double)(float)(img_w * -0.5));
  const float ddx = d0x - d1x, ddy = d0y - d1y;
  const float d2x = d1x + (-ddy), d2y = d1y + ddx;
  // window -> image, float64
  const double a00 = (double)d1x - (double)d0x, a10 = (double)d1y - (double)d0y;     // A = [u v], columns
  const double a01 = (double)d2x - (double)d0x, a11 = (double)d2y - (double)d0y;
  const double b00 = (double)s1x - (double)s0x, b10 = (double)s1y - (double)s0y;
  const double b01 = (double)s2x - (double)s0x, b11 = (double)s2y - (double)s0y;
  const double det = a00 * a11 - a01 * a10;
  const double i00 = a11 / det, i01 = -a01 / det, i10 = -a10 / det, i11 = a00 / det;
  const double l00 = b00 * i00 + b01 * i10, l01 = b00 * i01 + b01 * i11;
  const double l10 = b10 * i00 + b11 * i10, l11 = b10 * i01 + b11 * i11;
  T[0] = l00;
  T[1] = l01;
  T[2] = (double)s0x - (l00 * (double)d0x + l01 * (double)d0y);
  T[3] = l10;
  T[4] = l11;
  T[5] = (double)s0y - (l10 * (double)d0x + l11 * (double)d0y);
}

// affine_transform_modified (img_proc.py:71-78) of one float32 point
EGN_HD inline void egn_kpt_to_source(const double* T, float x, float y, double* src) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  src[0] = T[0] * (double)x + T[1] * (double)y + T[2];
  src[1] = T[3] * (double)x + T[4] * (double)y + T[5];
}

// One joint: out[EGN_KPT_METRIC_STATS] = (1, distance, distance < 0.1 den, < 0.2 den, < 0.3 den) when the joint is
// visible, else zeros.  den: the instance's PCK denominator.
EGN_HD inline void egn_kpt_joint_stats(const double* src, const double* gt, double den, double* out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dx = gt[0] - src[0], dy = gt[1] - src[1];
  const double dist = sqrt(dx * dx + dy * dy);
  const bool vis = gt[2] != 0.0;
  out[0] = vis ? 1.0 : 0.0;
  out[1] = vis ? dist : 0.0;
  out[2] = (vis && dist < 0.1 * den) ? 1.0 : 0.0;
  out[3] = (vis && dist < 0.2 * den) ? 1.0 : 0.0;
  out[4] = (vis && dist < 0.3 * den) ? 1.0 : 0.0;
}

// (max y - min y) / 3 from the extremes over all K annotated joints
EGN_HD inline double egn_kpt_pck_denominator(double max_y, double min_y) { return (max_y - min_y) / 3.0; }

// One instance on one thread: what the kernel's K wavefronts do, joint by joint.  src [K][2], gt [K][3];
// out[EGN_KPT_METRIC_STATS] is ADDED to, joints in order.
EGN_HD inline void egn_kpt_instance_stats(const double* src, const double* gt, int K, double* out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double mx = gt[1], mn = gt[1];
  for (int k = 1; k < K; ++k) {
    mx = fmax(mx, gt[3 * k + 1]);
    mn = fmin(mn, gt[3 * k + 1]);
  }
  const double den = egn_kpt_pck_denominator(mx, mn);
  for (int k = 0; k < K; ++k) {
    double s[EGN_KPT_METRIC_STATS];
    egn_kpt_joint_stats(src + 2 * k, gt + 3 * k, den, s);
    for (int c = 0; c < EGN_KPT_METRIC_STATS; ++c) out[c] = out[c] + s[c];
  }
}
