// Host build (g++) of the per-instance float64 math the HIP kernel in kpt_metrics.hip runs
// (egonet_amd/csrc/kpt_metric_math.h), exposed with a C ABI for the CPU test-suite.
// TEST INFRASTRUCTURE: not linked into the product library.
#include "../egonet_amd/csrc/kpt_metric_math.h"

// the inverse crop affines [n][2][3] of n instances
extern "C" void harness_kpt_inv_affine(const double* center, const double* scale, const double* rot, int n,
                                       double img_w, double img_h, double* T) {
  for (int i = 0; i < n; ++i) egn_kpt_inv_affine(center + 2 * i, scale + 2 * i, rot[i], img_w, img_h, T + 6 * i);
}

// m float32 points [m][2] through one affine -> [m][2] float64
extern "C" void harness_kpt_to_source(const double* T, const float* pts, int m, double* out) {
  for (int j = 0; j < m; ++j) egn_kpt_to_source(T, pts[2 * j], pts[2 * j + 1], out + 2 * j);
}

// n instances of K joints: out[5] = count, sum of distances, pck[3]
extern "C" void harness_kpt_stats(const double* src, const double* gt, int n, int K, double* out) {
  for (int c = 0; c < EGN_KPT_METRIC_STATS; ++c) out[c] = 0.0;
  for (int i = 0; i < n; ++i) egn_kpt_instance_stats(src + (long)2 * K * i, gt + (long)3 * K * i, K, out);
}
