// cuboid_math.h -- the canonical key-point cuboid of a labelled car (car_instance.py:730-747 construct_box_3d,
// :724-728 interpolate).  Shared by lifter_pairs.hip (egn_lifter_pairs_f64) and pose_annot.hip
// (egn_pose2d_annot_f64), so there is ONE cuboid.
//
// Contraction to FMA is off inside the two functions (the pragma at the head of each body), so that every product and
// sum of the cuboid rounds where numpy's does whatever the including file's setting is; the header changes nothing
// outside them.
#pragma once
#include <hip/hip_runtime.h>
#include "pose_math.h"

// canonical cuboid point j (car_instance.py:730-747): centre, 8 corners, 12 edges x ncoef interpolated points;
// the centring offsets are float32-rounded, so the centre is not exactly zero
__device__ inline void canon_corner(int k, double l, double h, double w, double* p) {   // k = 0..8
#pragma clang fp contract(off)
  const double ox = -(double)((float)l / 2.0f), oy = -(double)(float)h, oz = -(double)((float)w / 2.0f);
  const int c = k - 1;
  p[0] = (k == 0 ? 0.5 * l : (c < 4 ? l : 0.0)) + ox;
  p[1] = (k == 0 ? 0.5 * h : ((c & 1) ? h : 0.0)) + oy;
  p[2] = (k == 0 ? 0.5 * w : (((c >> 1) & 1) ? 0.0 : w)) + oz;
}

__device__ inline void canon_point(int j, double l, double h, double w, const double* coef, double* p) {
#pragma clang fp contract(off)
  if (j < 9) {
    canon_corner(j, l, h, w, p);
    return;
  }
  const int e = (j - 9) % 12, k = (j - 9) / 12;
  double a[3], b[3];
  canon_corner(1 + egn_edge_parent(e), l, h, w, a);
  canon_corner(1 + egn_edge_child(e), l, h, w, b);
  for (int d = 0; d < 3; ++d) p[d] = a[d] + coef[k] * (b[d] - a[d]);
}
