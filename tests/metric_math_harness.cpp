// Host build (g++) of the per-row float64 math the HIP kernel in lifter_metrics.hip runs
// (egonet_amd/csrc/metric_math.h), exposed with a C ABI for the CPU test-suite.
// TEST INFRASTRUCTURE: not linked into the product library.
#include "../egonet_amd/csrc/metric_math.h"

extern "C" void harness_metric_rows(const float* pred, const float* gt, int n, int layout, const float* mean,
                                    const float* stdv, double* out) {
  const int D = layout ? 99 : 96, cols = layout ? EGN_METRIC_COLS_R3DT : EGN_METRIC_COLS_R3D;
  for (int i = 0; i < n; ++i) egn_metric_row(pred + (long)D * i, gt + (long)D * i, mean, stdv, layout, out + (long)cols * i);
}

// |as_euler('xyz', degrees=True)| of n row-major 3x3 matrices
extern "C" void harness_euler_xyz(const double* R, int n, double* out) {
  for (int i = 0; i < n; ++i) {
    double M[3][3];
    for (int k = 0; k < 9; ++k) M[k / 3][k % 3] = R[9 * i + k];
    egn_metric_euler_xyz_abs_deg(M, out + 3 * i);
  }
}

extern "C" void harness_rotation_error(const double* H, double* out) {
  double M[3][3];
  for (int k = 0; k < 9; ++k) M[k / 3][k % 3] = H[k];
  egn_metric_rotation_error(M, out);
}
