// angle_metrics.hip -- the direct-regression baselines' metric (get_angle_error / AngleError), folded into an
// accumulator that stays on the device.
//
// Reference: libs/metric/criterions.py:40-55 (get_angle_error: atan2 of the predicted [cos, sin], |gt - pred| in
// degrees, wrapped into [0, 180]) and its running form AngleError (:145-171).  The reference copies every batch's
// prediction to the host; here
//   angle_metrics_rows_kernel  one thread per row: the two float32 of the row, atan2 in float64, the wrapped
//                              difference; the wave adds its 64 rows by a fixed xor tree, the block its four waves in
//                              wave order; one {count, sum} partial per block, written with plain stores
//   angle_metrics_fold_kernel  the block partials added to the accumulator: lane l takes blocks l, l + 64, ... in
//                              order, then the same xor tree
// No atomics and no hand-off between blocks: the same input gives the same bits.  A few bytes per row; nothing here
// is worth tuning -- the point is that no batch is read back.
#include "egn_internal.h"

namespace {

constexpr int AT = 256;                 // threads (= rows) per block
constexpr int AWAVES = AT / 64;
constexpr int APS = EGN_ANGLE_METRICS_ACC_DOUBLES;      // doubles per partial: count, sum of errors in degrees

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(AT) void angle_metrics_rows_kernel(const float* __restrict__ pred, long N, int ld,
                                                                const double* __restrict__ angles_gt,
                                                                double* __restrict__ part) {
  __shared__ double s_part[AWAVES][APS];
  const long i = (long)blockIdx.x * AT + threadIdx.x;
  double cnt = 0.0, err = 0.0;
  if (i < N) {
    const float* p = pred + (size_t)i * ld;
    const double a = atan2((double)p[1], (double)p[0]);
    const double d = fabs(angles_gt[i] - a) * 180.0 / 3.141592653589793;      // numpy's order: (x * 180) / pi
    err = d > 180.0 ? 360.0 - d : d;
    cnt = 1.0;
  }
  cnt = wave_sum(cnt);
  err = wave_sum(err);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_part[wave][0] = cnt;
    s_part[wave][1] = err;
  }
  __syncthreads();
  if (threadIdx.x < APS) {                          // the block's waves, in wave order
    double s = s_part[0][threadIdx.x];
    for (int w = 1; w < AWAVES; ++w) s = s + s_part[w][threadIdx.x];
    part[(size_t)blockIdx.x * APS + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void angle_metrics_fold_kernel(const double* __restrict__ part, long blocks,
                                                                double* __restrict__ acc) {
  double s[APS];
#pragma unroll
  for (int c = 0; c < APS; ++c) s[c] = 0.0;
  for (long b = threadIdx.x; b < blocks; b += 64) {
#pragma unroll
    for (int c = 0; c < APS; ++c) s[c] = s[c] + part[(size_t)b * APS + c];
  }
#pragma unroll
  for (int c = 0; c < APS; ++c) s[c] = wave_sum(s[c]);
  if (threadIdx.x == 0) {                           // every lane holds the same sums after the tree
#pragma unroll
    for (int c = 0; c < APS; ++c) acc[c] = acc[c] + s[c];
  }
}

__global__ __launch_bounds__(64) void angle_metrics_reset_kernel(double* __restrict__ acc) {
  if (threadIdx.x < EGN_ANGLE_METRICS_ACC_DOUBLES) acc[threadIdx.x] = 0.0;
}

inline long angle_blocks(long N) { return N < 1 ? 1 : (N + AT - 1) / AT; }

}  // namespace

extern "C" long egn_angle_metrics_ws_bytes(long N) {
  if (N < 0 || N > 0x7fffffffL) return EGN_E_BADARG;
  return angle_blocks(N) * APS * (long)sizeof(double);
}

extern "C" int egn_angle_metrics_reset(double* acc, void* stream) {
  if (!acc) return EGN_E_BADARG;
  hipLaunchKernelGGL(angle_metrics_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_angle_metrics_update_f32(const float* pred, long N, int ld, const double* angles_gt, void* ws,
                                            long ws_bytes, double* acc, void* stream) {
  if (N < 0 || N > 0x7fffffffL || ld < 2 || !acc) return EGN_E_BADARG;
  if (N == 0) return 0;
  if (!pred || !angles_gt || !ws || ws_bytes < egn_angle_metrics_ws_bytes(N)) return EGN_E_BADARG;
  const long blocks = angle_blocks(N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(angle_metrics_rows_kernel, dim3((unsigned)blocks), dim3(AT), 0, s, pred, N, ld, angles_gt,
                     (double*)ws);
  hipLaunchKernelGGL(angle_metrics_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, blocks, acc);
  egn_count_launches(2);
  return (int)hipGetLastError();
}
