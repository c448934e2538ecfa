// metric_math.h -- per-row math of the lifter's 3-D validation metrics (reference libs/metric/criterions.py:241-301:
// update_joints_3d_error style 'direct', update_rotation_error style 'euler'), shared by the HIP kernel
// (lifter_metrics.hip) and by the host-compiled unit harness (tests/metric_math_harness.cpp, built with g++), in the
// style of pose_math.h.
//
// A row is a predicted and a target cuboid, float32: 32 points relative to the root ('R3d', 96 values) or the root
// followed by them ('R3d+T', 99 values).  Its result columns, float64:
//   [0, 32)   _rT     distance of every point, sqrt(sum((gt - pred)^2))
//   [32, 35)  _R      |Euler angles 'xyz' (extrinsic), degrees| of the Kabsch rotation pred -> gt
//   [35]      _T      distance of the root            ('R3d+T' only)
//   [36, 39)  _T_xyz  |gt - pred| of the root         ('R3d+T' only)
// The optional unnormalise is the one float32 step (operations.py:50-52 on float32 arrays: a product and a sum, each
// rounded); everything after it is float64.  The reference does the distances, H and the SVD in float32.
//
// Degenerate rows.  H = 0 (every predicted point equal, or every target point equal) gives the rotation error
// (0, 0, 0): numpy's SVD of a zero matrix returns identity U and V.  For H of rank 1 the reference's result depends on
// the SVD implementation; here the numbers are finite and UNSPECIFIED (the identity when the second singular direction
// cannot be normalised, else whatever direction the rounding noise leaves).  Finite inputs never give a NaN.
#pragma once
#include "pose_math.h"

#define EGN_METRIC_JOINTS 32
#define EGN_METRIC_COLS_R3D 35
#define EGN_METRIC_COLS_R3DT 39
#define EGN_METRIC_COL_R 32
#define EGN_METRIC_COL_T 35

// x * std + mean in float32, two roundings: never contracted into an fma
EGN_HD inline float egn_metric_unnorm_f32(float x, float stdv, float mean) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float p = x * stdv;
  return p + mean;
}

EGN_HD inline double egn_metric_dist3(const double* g, const double* p) {
  const double dx = g[0] - p[0], dy = g[1] - p[1], dz = g[2] - p[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// |Rotation.from_matrix(R).as_euler('xyz', degrees=True)|: lower case = extrinsic, R = Rz(c) Ry(b) Rx(a), returned
// (a, b, c).  b from sin b = -R20 and cos b = |(R00, R10)| (asin alone loses half the digits near +-90 deg).  Gimbal
// lock: scipy sets the third angle to zero and puts the whole turn into the first; its test is |b -+ pi/2| <= 1e-7
// rad, which is cos b <= 1e-7.
EGN_HD inline void egn_metric_euler_xyz_abs_deg(const double R[3][3], double e[3]) {
  const double cb = sqrt(R[0][0] * R[0][0] + R[1][0] * R[1][0]);
  const double b = atan2(-R[2][0], cb);
  double a, c;
  if (cb > 1e-7) {
    a = atan2(R[2][1], R[2][2]);
    c = atan2(R[1][0], R[0][0]);
  } else {
    c = 0.0;
    a = atan2(-R[1][2], R[1][1]);
  }
  const double deg = 180.0 / 3.14159265358979323846;
  e[0] = fabs(a * deg);
  e[1] = fabs(b * deg);
  e[2] = fabs(c * deg);
}

// H = (pred - mean)(gt - mean)^T -> the three rotation error columns (compute_rigid_transform(pred.T, gt.T),
// transformation.py:99-134, then the Euler angles)
EGN_HD inline void egn_metric_rotation_error(const double H[3][3], double e[3]) {
  double R[3][3];
  egn_kabsch_rotation(H, R);
  bool ok = true;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) ok = ok && (fabs(R[r][c]) <= 2.0);     // false for NaN
  if (!ok)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r][c] = (r == c) ? 1.0 : 0.0;
  egn_metric_euler_xyz_abs_deg(R, e);
}

// sum of 32 values in the order of the kernel's cross-lane butterfly (partner distance 16, 8, 4, 2, 1); v is destroyed
EGN_HD inline double egn_metric_tree_sum32(double* v) {
  for (int m = 16; m >= 1; m >>= 1)
    for (int i = 0; i < m; ++i) v[i] = v[i] + v[i + m];
  return v[0];
}

// One row on one thread: what the kernel's 32 lanes do together.  pred / gt: 96 ('R3d', layout 0) or 99 ('R3d+T',
// layout 1) float32; mean / stdv: as many float32, or both NULL; out: 35 or 39 columns.
EGN_HD inline void egn_metric_row(const float* pred, const float* gt, const float* mean, const float* stdv, int layout,
                                  double* out) {
  const int off = layout ? 3 : 0;
  const int D = 3 * EGN_METRIC_JOINTS + off;
  double P[3 * EGN_METRIC_JOINTS + 3], G[3 * EGN_METRIC_JOINTS + 3];
  for (int k = 0; k < D; ++k) {
    P[k] = (double)(mean ? egn_metric_unnorm_f32(pred[k], stdv[k], mean[k]) : pred[k]);
    G[k] = (double)(mean ? egn_metric_unnorm_f32(gt[k], stdv[k], mean[k]) : gt[k]);
  }
  double mp[3], mg[3], t[EGN_METRIC_JOINTS];
  for (int d = 0; d < 3; ++d) {
    for (int j = 0; j < EGN_METRIC_JOINTS; ++j) t[j] = P[off + 3 * j + d];
    mp[d] = egn_metric_tree_sum32(t) / 32.0;
    for (int j = 0; j < EGN_METRIC_JOINTS; ++j) t[j] = G[off + 3 * j + d];
    mg[d] = egn_metric_tree_sum32(t) / 32.0;
  }
  double H[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      for (int j = 0; j < EGN_METRIC_JOINTS; ++j) t[j] = (P[off + 3 * j + r] - mp[r]) * (G[off + 3 * j + c] - mg[c]);
      H[r][c] = egn_metric_tree_sum32(t);
    }
  for (int j = 0; j < EGN_METRIC_JOINTS; ++j) out[j] = egn_metric_dist3(G + off + 3 * j, P + off + 3 * j);
  egn_metric_rotation_error(H, out + EGN_METRIC_COL_R);
  if (layout) {
    out[EGN_METRIC_COL_T] = egn_metric_dist3(G, P);
    for (int d = 0; d < 3; ++d) out[EGN_METRIC_COL_T + 1 + d] = fabs(G[d] - P[d]);
  }
}
