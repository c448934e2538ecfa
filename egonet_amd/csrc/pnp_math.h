// pnp_math.h -- per-instance float64 math of the reprojection refinement of a lifted cuboid against its own 2-D key
// points (the reference's pnp_refine, libs/common/transformation.py:143-157, and its flow in
// tools/inference_legacy.py:518-547): a rigid pose (R, T) that minimises
//     sum_i w_i | pi(R X_i + T) - k_i |^2,   X_0 = 0 (the root), X_i = S_{i-1},   pi = pinhole (fx, fy, cx, cy)
// by Levenberg-Marquardt from R = I.  No distortion, no scale.  No HIP-only construct: pnp_refine.hip instantiates
// the same templates for one wave per instance (lane i owns correspondence i) and for a plain host loop.
//
// The templates take a "lanes" policy P that says which correspondences the caller owns and how partial sums are
// combined:
//   int  first(), stride()        the caller handles i = first(), first() + stride(), ... < J
//   void sum(double (&v)[N])      afterwards every caller holds the same total of v over all callers
//   bool leader()                 the one caller that stores the per-instance scalars
// All control flow below depends only on totals, so it is uniform over the callers of one instance.
#pragma once
#include "pose_math.h"

#define EGN_PNP_MAX_ITERS 64      // cap on LM trial steps (accepted + rejected)
#define EGN_PNP_STEP_TOL 1e-10    // terminate on a step with |delta|_inf below this (rad, m)
#define EGN_PNP_LAMBDA0 1e-3      // initial damping
#define EGN_PNP_LAMBDA_MIN 1e-12
#define EGN_PNP_LAMBDA_MAX 1e12   // damping past this: the system is treated as singular
#define EGN_PNP_LAMBDA_CONV 1.0   // a small step only counts as convergence while the damping is at most this
// "The cost does not increase" can only be decided down to the resolution of the cost's own evaluation: pixel
// coordinates of the order of 1e3 round at 1e-13, against residuals of about a pixel that is 1e-13 of the cost.  The
// last steps change the cost by less (1e-6 m in depth at 60 m), so the comparison would take or refuse them by chance
// and the iteration would stall short of the optimum that the gradient still resolves.  A step whose decrease as the
// quadratic model predicts it is below this fraction of the cost is therefore taken on the model's word.
#define EGN_PNP_COST_RES 1e-11

struct egn_pnp_serial {   // one caller owns every correspondence
  EGN_HD int first() const { return 0; }
  EGN_HD int stride() const { return 1; }
  EGN_HD bool leader() const { return true; }
  template <int N>
  EGN_HD void sum(double (&)[N]) const {}
};

struct egn_pnp_in {
  const double* S;    // [J-1][3] shape relative to the root
  const double* k;    // [J][2] screen key points, k[0] = the root's projection
  const double* w;    // [J] weights or NULL (ones); a weight that is not > 0 drops the correspondence
  const double* T0;   // [3] initial root or NULL (weak-perspective start)
  double fx, fy, cx, cy;
  double max_shift;
  int J;
};

EGN_HD inline bool egn_pnp_finite(double x) { return fabs(x) <= 1.7e308; }   // false for NaN

EGN_HD inline double egn_pnp_weight(const egn_pnp_in& in, int i) { return in.w ? in.w[i] : 1.0; }

// q = R X_i, p = q + T
EGN_HD inline void egn_pnp_point(const egn_pnp_in& in, const double R[9], const double T[3], int i, double q[3],
                                 double p[3]) {
  if (i == 0) {
    q[0] = q[1] = q[2] = 0.0;
  } else {
    const double* s = in.S + 3 * (size_t)(i - 1);
    for (int r = 0; r < 3; ++r) q[r] = R[3 * r] * s[0] + R[3 * r + 1] * s[1] + R[3 * r + 2] * s[2];
  }
  for (int r = 0; r < 3; ++r) p[r] = q[r] + T[r];
}

// acc[0] = weighted squared pixel error at (R, T), acc[1] = number of used points that are not in front of the camera
template <class P>
EGN_HD inline void egn_pnp_cost(const P& par, const egn_pnp_in& in, const double R[9], const double T[3],
                                double* cost, double* behind) {
  double acc[2] = {0.0, 0.0};
  for (int i = par.first(); i < in.J; i += par.stride()) {
    const double wi = egn_pnp_weight(in, i);
    if (!(wi > 0.0)) continue;
    double q[3], p[3];
    egn_pnp_point(in, R, T, i, q, p);
    if (!(p[2] > 0.0)) {
      acc[1] += 1.0;
      continue;
    }
    const double du = in.fx * p[0] / p[2] + in.cx - in.k[2 * i];
    const double dv = in.fy * p[1] / p[2] + in.cy - in.k[2 * i + 1];
    acc[0] += wi * (du * du + dv * dv);
  }
  par.sum(acc);
  *cost = acc[0];
  *behind = acc[1];
}

// E = exp([d]x) (Rodrigues), R <- E R
EGN_HD inline void egn_pnp_rotate_left(const double d[3], const double R[9], double out[9]) {
  const double t2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  double a, b;   // E = I + a [d]x + b [d]x^2
  if (t2 < 1e-8) {
    a = 1.0 - t2 / 6.0;
    b = 0.5 - t2 / 24.0;
  } else {
    const double t = sqrt(t2);
    a = sin(t) / t;
    b = (1.0 - cos(t)) / t2;
  }
  double E[9];
  E[0] = 1.0 - b * (d[1] * d[1] + d[2] * d[2]);
  E[4] = 1.0 - b * (d[0] * d[0] + d[2] * d[2]);
  E[8] = 1.0 - b * (d[0] * d[0] + d[1] * d[1]);
  E[1] = b * d[0] * d[1] - a * d[2];
  E[3] = b * d[0] * d[1] + a * d[2];
  E[2] = b * d[0] * d[2] + a * d[1];
  E[6] = b * d[0] * d[2] - a * d[1];
  E[5] = b * d[1] * d[2] - a * d[0];
  E[7] = b * d[1] * d[2] + a * d[0];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out[3 * r + c] = E[3 * r] * R[c] + E[3 * r + 1] * R[3 + c] + E[3 * r + 2] * R[6 + c];
}

// delta = -(A + lambda diag(A))^-1 g by Cholesky; A as the upper triangle ne[idx(a, b)], g = ne[21..26].
// false: a pivot is not positive (or not finite)
EGN_HD inline bool egn_pnp_solve6(const double ne[27], double lambda, double delta[6]) {
  double L[6][6];
  int t = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      L[b][a] = ne[t];
      L[a][b] = ne[t];
      ++t;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a) L[a][a] += lambda * L[a][a];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int m = 0; m < j; ++m) d -= L[j][m] * L[j][m];
    if (!(d > 0.0) || !egn_pnp_finite(d)) {
      ok = false;
      d = 1.0;
    }
    const double inv = 1.0 / sqrt(d);
    L[j][j] = d * inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
#pragma unroll
      for (int m = 0; m < j; ++m) s -= L[i][m] * L[j][m];
      L[i][j] = s * inv;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {   // L y = -g
    double s = -ne[21 + i];
#pragma unroll
    for (int m = 0; m < i; ++m) s -= L[i][m] * y[m];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {   // L^T delta = y
    double s = y[i];
#pragma unroll
    for (int m = i + 1; m < 6; ++m) s -= L[m][i] * delta[m];
    delta[i] = s / L[i][i];
  }
  return ok;
}

// J^T J (upper triangle, 21) and J^T r (6) at (R, T); every used point is in front of the camera there.
// Left-multiplicative update p' = exp([dw]x) q + T + dt ~ p + dw x q + dt:
//   dp/d(dw) = -[q]x, dp/d(dt) = I;  du/dp = (fx/z, 0, -fx x/z^2), dv/dp = (0, fy/z, -fy y/z^2)
template <class P>
EGN_HD inline void egn_pnp_normal_equations(const P& par, const egn_pnp_in& in, const double R[9], const double T[3],
                                            double (&ne)[27]) {
#pragma unroll
  for (int t = 0; t < 27; ++t) ne[t] = 0.0;
  for (int i = par.first(); i < in.J; i += par.stride()) {
    const double wi = egn_pnp_weight(in, i);
    if (!(wi > 0.0)) continue;
    double q[3], p[3];
    egn_pnp_point(in, R, T, i, q, p);
    const double iz = 1.0 / p[2];
    const double a = in.fx * iz, c = -in.fx * p[0] * iz * iz;
    const double b = in.fy * iz, d = -in.fy * p[1] * iz * iz;
    const double ru = in.fx * p[0] * iz + in.cx - in.k[2 * i];
    const double rv = in.fy * p[1] * iz + in.cy - in.k[2 * i + 1];
    const double ju[6] = {c * q[1], a * q[2] - c * q[0], -a * q[1], a, 0.0, c};
    const double jv[6] = {d * q[1] - b * q[2], -d * q[0], b * q[0], 0.0, b, d};
    int t = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int s = r; s < 6; ++s) ne[t++] += wi * (ju[r] * ju[s] + jv[r] * jv[s]);
#pragma unroll
    for (int r = 0; r < 6; ++r) ne[21 + r] += wi * (ju[r] * ru + jv[r] * rv);
  }
  par.sum(ne);
}

// The fit.  Returns the status (1 refined, 0 converged but moved more than max_shift from T0, -1 not usable) and
// the pose of the RETURNED placement: the optimum for status 1, else (I, start T).  cost[0] = cost at the start,
// cost[1] = cost of the returned placement (both 0 when a used point is not in front of the camera at the start).
template <class P>
EGN_HD inline int egn_pnp_solve(const P& par, const egn_pnp_in& in, double R[9], double T[3], double cost[2],
                                int* iters) {
  for (int t = 0; t < 9; ++t) R[t] = (t % 4 == 0) ? 1.0 : 0.0;
  *iters = 0;
  cost[0] = cost[1] = 0.0;
  if (in.T0) {
    for (int d = 0; d < 3; ++d) T[d] = in.T0[d];
  } else {
    // weak perspective: z0 = sqrt(sum w (Sx^2 + Sy^2) / sum w |(k_i - k_0) / fx|^2), T = z0 K^-1 (k_0, 1)
    double acc[2] = {0.0, 0.0};
    for (int i = par.first(); i < in.J; i += par.stride()) {
      const double wi = egn_pnp_weight(in, i);
      if (i == 0 || !(wi > 0.0)) continue;
      const double* s = in.S + 3 * (size_t)(i - 1);
      const double dx = (in.k[2 * i] - in.k[0]) / in.fx, dy = (in.k[2 * i + 1] - in.k[1]) / in.fx;
      acc[0] += wi * (s[0] * s[0] + s[1] * s[1]);
      acc[1] += wi * (dx * dx + dy * dy);
    }
    par.sum(acc);
    const double z0 = sqrt(acc[0] / acc[1]);
    T[0] = z0 * (in.k[0] - in.cx) / in.fx;
    T[1] = z0 * (in.k[1] - in.cy) / in.fy;
    T[2] = z0;
  }
  if (!(egn_pnp_finite(T[0]) && egn_pnp_finite(T[1]) && egn_pnp_finite(T[2]))) {
    T[0] = T[1] = T[2] = 0.0;
    return -1;
  }
  const double Ts[3] = {T[0], T[1], T[2]};
  double c0, behind;
  egn_pnp_cost(par, in, R, T, &c0, &behind);
  if (behind != 0.0 || !egn_pnp_finite(c0)) return -1;
  cost[0] = cost[1] = c0;

  double c = c0, lambda = EGN_PNP_LAMBDA0;
  int it = 0;
  bool converged = false, stop = false;
  while (!stop && it < EGN_PNP_MAX_ITERS) {
    double ne[27];
    egn_pnp_normal_equations(par, in, R, T, ne);
    bool accepted = false;
    while (!accepted && !stop && it < EGN_PNP_MAX_ITERS) {
      ++it;
      double delta[6];
      if (!egn_pnp_solve6(ne, lambda, delta)) {
        lambda *= 10.0;
        stop = lambda > EGN_PNP_LAMBDA_MAX;
        continue;
      }
      double step = 0.0;
      for (int d = 0; d < 6; ++d) step = fmax(step, fabs(delta[d]));
      double Rn[9], Tn[3], cn, bn;
      egn_pnp_rotate_left(delta, R, Rn);
      for (int d = 0; d < 3; ++d) Tn[d] = T[d] + delta[3 + d];
      egn_pnp_cost(par, in, Rn, Tn, &cn, &bn);
      const double used = lambda;
      // decrease of the model c + 2 g^T d + d^T A d
      double pred = 0.0;
      {
        int t = 0;
        for (int r = 0; r < 6; ++r)
          for (int q = r; q < 6; ++q) pred -= (q == r ? 1.0 : 2.0) * ne[t++] * delta[r] * delta[q];
        for (int r = 0; r < 6; ++r) pred -= 2.0 * ne[21 + r] * delta[r];
      }
      if (bn == 0.0 && (cn <= c || pred <= EGN_PNP_COST_RES * c)) {   // a step is taken only if the cost does not increase
        for (int t = 0; t < 9; ++t) R[t] = Rn[t];
        for (int d = 0; d < 3; ++d) T[d] = Tn[d];
        c = cn;
        lambda = fmax(lambda * 0.1, EGN_PNP_LAMBDA_MIN);
        accepted = true;
      } else {
        lambda *= 10.0;
      }
      // a step this small is the optimum to rounding whether or not rounding let the cost fall, unless the damping
      // made it small
      if (step < EGN_PNP_STEP_TOL && used <= EGN_PNP_LAMBDA_CONV) {
        converged = true;
        stop = true;
      } else if (lambda > EGN_PNP_LAMBDA_MAX) {
        stop = true;
      }
    }
  }
  *iters = it;
  int status = converged ? 1 : -1;
  if (converged && in.T0 && egn_pnp_finite(in.max_shift)) {
    const double dx = T[0] - Ts[0], dy = T[1] - Ts[1], dz = T[2] - Ts[2];
    if (sqrt(dx * dx + dy * dy + dz * dz) > in.max_shift) status = 0;
  }
  if (status == 1 && c <= c0) {
    cost[1] = c;
  } else {   // also a start that already is the optimum to rounding (rounding let the cost creep up): it is returned
    for (int t = 0; t < 9; ++t) R[t] = (t % 4 == 0) ? 1.0 : 0.0;
    for (int d = 0; d < 3; ++d) T[d] = Ts[d];
  }
  return status;
}

// returned point i: R X_i + T when refined, else the unrefined placement T + X_i with no rotation arithmetic
EGN_HD inline void egn_pnp_placed(const egn_pnp_in& in, int status, const double R[9], const double T[3], int i,
                                  double p[3]) {
  if (status == 1) {
    double q[3];
    egn_pnp_point(in, R, T, i, q, p);
  } else {
    for (int d = 0; d < 3; ++d) p[d] = (i == 0) ? T[d] : T[d] + in.S[3 * (size_t)(i - 1) + d];
  }
}

// One instance end to end.  refined [J][3], rt [12] = R row-major then T, cost [2], dims [3] = (l, h, w): mean edge
// lengths of the returned cuboid by the rule of egn_pose_solve_one (corners = points 1..8; zeros when J < 9).
template <class P>
EGN_HD inline void egn_pnp_refine_one(const P& par, const egn_pnp_in& in, double* refined, double* rt, double* cost,
                                      int* iters, int* status, double* dims) {
  double R[9], T[3], c[2];
  int it;
  const int st = egn_pnp_solve(par, in, R, T, c, &it);
  for (int i = par.first(); i < in.J; i += par.stride()) {
    double p[3];
    egn_pnp_placed(in, st, R, T, i, p);
    for (int d = 0; d < 3; ++d) refined[3 * (size_t)i + d] = p[d];
  }
  if (!par.leader()) return;
  double len[3] = {0.0, 0.0, 0.0};
  if (in.J >= 9)
    for (int e = 0; e < 12; ++e) {
      double a[3], b[3];
      egn_pnp_placed(in, st, R, T, 1 + egn_edge_parent(e), a);
      egn_pnp_placed(in, st, R, T, 1 + egn_edge_child(e), b);
      const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
      len[e >> 2] += sqrt(dx * dx + dy * dy + dz * dz);
    }
  dims[0] = len[1] / 4;   // l
  dims[1] = len[0] / 4;   // h
  dims[2] = len[2] / 4;   // w
  for (int t = 0; t < 9; ++t) rt[t] = R[t];
  for (int d = 0; d < 3; ++d) rt[9 + d] = T[d];
  cost[0] = c[0];
  cost[1] = c[1];
  *iters = it;
  *status = st;
}
