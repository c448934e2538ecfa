// lifter_metrics.hip -- the lifter's 3-D validation metrics, folded into an accumulator that stays on the device.
//
// Reference: libs/metric/criterions.py:223-301 (update_statistics, update_rotation_error style 'euler',
// update_joints_3d_error style 'direct') as RError3D / RTError3D call them (:390-538), after the unnormalise of
// libs/trainer/trainer.py:474-481.  The reference copies every batch to the host and loops over its rows in Python
// (one np.linalg.svd and one scipy Rotation per row); here
//   metrics_rows_kernel   one point per lane, two rows per wave: unnormalise (float32), distances, the centroids and H
//                         by a butterfly over the row's 32 lanes, the Kabsch rotation and its Euler angles
//                         (metric_math.h), column sum / max / min in registers over a grid-stride loop, one partial
//                         per block, written with plain stores
//   metrics_fold_kernel   the block partials added to the accumulator in block order
// No atomics and no hand-off between blocks: the same input gives the same bits.  Contraction to FMA is off for this
// file: the unnormalise is a float32 product and a float32 sum like numpy's, and the float64 sums round where the
// host build of metric_math.h rounds.
#include "egn_internal.h"
#include "metric_math.h"
#pragma clang fp contract(off)

namespace {

constexpr int MT = 256;                 // threads per block: 4 waves, 8 rows per pass
constexpr int MROWS = MT / 32;          // row slots of a block
constexpr int MAX_BLOCKS = 256;         // one per CU; a batch of 2048 rows is one pass of 256 blocks
constexpr int CS = 40;                  // column stride of partials and accumulator (>= 39)
constexpr int ACC_SUM = 8, ACC_MAX = ACC_SUM + CS, ACC_MIN = ACC_MAX + CS;
static_assert(ACC_MIN + CS == EGN_LIFTER_METRICS_ACC_DOUBLES, "accumulator layout");
static_assert(CS >= EGN_METRIC_COLS_R3DT && CS - EGN_METRIC_JOINTS <= 32, "column stride");
// the reference's initial max / min (criterions.py:405-411); neutral for the non-negative error columns
constexpr double MAX0 = -1.0, MIN0 = 1e16;

struct MetricArgs {
  const float* pred;
  const float* gt;
  long long n;
  int ld, layout;
  const float* mean;      // [D] or NULL
  const float* stdv;
  double* part;           // [blocks][3][CS]
  double* rows_out;       // [n][cols] or NULL
};

// sum over the 32 lanes of a row (a half wave): every lane gets the same bits (egn_metric_tree_sum32 on the host)
__device__ inline double row_sum32(double v) {
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(MT) void metrics_rows_kernel(MetricArgs a) {
  __shared__ double s_part[MROWS][3][CS];
  const int tid = threadIdx.x;
  const int slot = tid >> 5;                    // (wave, half): the row slot of this lane
  const int j = tid & 31;                       // the point of this lane
  const int off = a.layout ? 3 : 0;
  const int cols = a.layout ? EGN_METRIC_COLS_R3DT : EGN_METRIC_COLS_R3D;
  const int nextra = cols - EGN_METRIC_JOINTS;  // lanes 0..2: _R, lane 3: _T, lanes 4..6: _T_xyz
  const bool unnorm = a.mean != nullptr;

  float sj[3] = {1.f, 1.f, 1.f}, mj[3] = {0.f, 0.f, 0.f}, sr[3] = {1.f, 1.f, 1.f}, mr[3] = {0.f, 0.f, 0.f};
  if (unnorm)
    for (int d = 0; d < 3; ++d) {
      sj[d] = a.stdv[off + 3 * j + d];
      mj[d] = a.mean[off + 3 * j + d];
      if (a.layout) {
        sr[d] = a.stdv[d];
        mr[d] = a.mean[d];
      }
    }

  double sum0 = 0.0, max0 = MAX0, min0 = MIN0;  // column j
  double sum1 = 0.0, max1 = MAX0, min1 = MIN0;  // column 32 + j, j < nextra
  // `base` is the same for the 64 lanes of a wave: all of them reach every shuffle
  for (long long base = (long long)blockIdx.x * MROWS + (slot & ~1); base < a.n; base += (long long)gridDim.x * MROWS) {
    const long long row = base + (slot & 1);
    const bool valid = row < a.n;
    const size_t r = (size_t)(valid ? row : a.n - 1);       // a half-empty wave re-reads the last row
    const float* pp = a.pred + r * (size_t)a.ld;
    const float* gp = a.gt + r * (size_t)a.ld;
    double P[3], G[3];
    for (int d = 0; d < 3; ++d) {
      float p = pp[off + 3 * j + d], g = gp[off + 3 * j + d];
      if (unnorm) {
        p = egn_metric_unnorm_f32(p, sj[d], mj[d]);
        g = egn_metric_unnorm_f32(g, sj[d], mj[d]);
      }
      P[d] = (double)p;
      G[d] = (double)g;
    }
    const double dist = egn_metric_dist3(G, P);
    double mp[3], mg[3];
    for (int d = 0; d < 3; ++d) {
      mp[d] = row_sum32(P[d]) / 32.0;
      mg[d] = row_sum32(G[d]) / 32.0;
    }
    double H[3][3];
    for (int rr = 0; rr < 3; ++rr)
      for (int c = 0; c < 3; ++c) H[rr][c] = row_sum32((P[rr] - mp[rr]) * (G[c] - mg[c]));
    double e[3];
    egn_metric_rotation_error(H, e);            // every lane of the row: the same H, the same result
    double extra = (j == 0) ? e[0] : (j == 1 ? e[1] : e[2]);
    if (a.layout) {
      double RP[3], RG[3];
      for (int d = 0; d < 3; ++d) {
        float p = pp[d], g = gp[d];
        if (unnorm) {
          p = egn_metric_unnorm_f32(p, sr[d], mr[d]);
          g = egn_metric_unnorm_f32(g, sr[d], mr[d]);
        }
        RP[d] = (double)p;
        RG[d] = (double)g;
      }
      if (j == 3) extra = egn_metric_dist3(RG, RP);
      if (j == 4) extra = fabs(RG[0] - RP[0]);
      if (j == 5) extra = fabs(RG[1] - RP[1]);
      if (j == 6) extra = fabs(RG[2] - RP[2]);
    }
    if (valid) {
      sum0 += dist;
      max0 = fmax(max0, dist);
      min0 = fmin(min0, dist);
      if (j < nextra) {
        sum1 += extra;
        max1 = fmax(max1, extra);
        min1 = fmin(min1, extra);
      }
      if (a.rows_out) {
        double* o = a.rows_out + (size_t)row * cols;
        o[j] = dist;
        if (j < nextra) o[EGN_METRIC_JOINTS + j] = extra;
      }
    }
  }

  s_part[slot][0][j] = sum0;
  s_part[slot][1][j] = max0;
  s_part[slot][2][j] = min0;
  if (j < CS - EGN_METRIC_JOINTS) {             // columns past `cols` carry the neutral values
    s_part[slot][0][EGN_METRIC_JOINTS + j] = sum1;
    s_part[slot][1][EGN_METRIC_JOINTS + j] = max1;
    s_part[slot][2][EGN_METRIC_JOINTS + j] = min1;
  }
  __syncthreads();
  if (tid < CS) {                               // the block's 8 row slots, in slot order
    double s = s_part[0][0][tid], mx = s_part[0][1][tid], mn = s_part[0][2][tid];
    for (int k = 1; k < MROWS; ++k) {
      s += s_part[k][0][tid];
      mx = fmax(mx, s_part[k][1][tid]);
      mn = fmin(mn, s_part[k][2][tid]);
    }
    double* o = a.part + (size_t)blockIdx.x * 3 * CS;
    o[tid] = s;
    o[CS + tid] = mx;
    o[2 * CS + tid] = mn;
  }
}

__global__ __launch_bounds__(64) void metrics_fold_kernel(const double* __restrict__ part, int blocks, long long n,
                                                          double* __restrict__ acc) {
  const int c = threadIdx.x;
  if (c >= CS) return;
  double s = 0.0, mx = MAX0, mn = MIN0;
#pragma unroll 16                 // the loads of 16 partials in flight; the additions stay in block order
  for (int b = 0; b < blocks; ++b) {
    const double* p = part + (size_t)b * 3 * CS;
    s += p[c];
    mx = fmax(mx, p[CS + c]);
    mn = fmin(mn, p[2 * CS + c]);
  }
  acc[ACC_SUM + c] = acc[ACC_SUM + c] + s;
  acc[ACC_MAX + c] = fmax(acc[ACC_MAX + c], mx);
  acc[ACC_MIN + c] = fmin(acc[ACC_MIN + c], mn);
  if (c == 0) acc[0] = acc[0] + (double)n;
}

__global__ __launch_bounds__(128) void metrics_reset_kernel(double* __restrict__ acc, int layout) {
  const int t = threadIdx.x;
  double v = 0.0;
  if (t == 1) v = (double)layout;
  if (t >= ACC_MAX && t < ACC_MIN) v = MAX0;
  if (t >= ACC_MIN) v = MIN0;
  acc[t] = v;
}

inline int metric_blocks(long long n) {
  const long long b = (n + MROWS - 1) / MROWS;
  return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

}  // namespace

extern "C" long egn_lifter_metrics_ws_bytes(long n) {
  if (n < 0) return EGN_E_BADARG;
  return (long)((size_t)metric_blocks(n) * 3 * CS * sizeof(double));
}

extern "C" int egn_lifter_metrics_reset(double* acc, int layout, void* stream) {
  if (!acc || (layout != 0 && layout != 1)) return EGN_E_BADARG;
  hipLaunchKernelGGL(metrics_reset_kernel, dim3(1), dim3(EGN_LIFTER_METRICS_ACC_DOUBLES), 0, (hipStream_t)stream, acc,
                     layout);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_lifter_metrics_update_f32(const float* pred, const float* gt, long n, int D, int ld,
                                             const float* mean_out, const float* std_out, int layout, void* ws,
                                             long ws_bytes, double* acc, double* rows_out, void* stream) {
  if (!pred || !gt || !ws || !acc || n < 0 || (layout != 0 && layout != 1) ||
      D != 3 * EGN_METRIC_JOINTS + (layout ? 3 : 0) || ld < D || (mean_out == nullptr) != (std_out == nullptr))
    return EGN_E_BADARG;
  if (n == 0) return 0;
  if (ws_bytes < egn_lifter_metrics_ws_bytes(n)) return EGN_E_BADARG;
  MetricArgs a;
  a.pred = pred;
  a.gt = gt;
  a.n = n;
  a.ld = ld;
  a.layout = layout;
  a.mean = mean_out;
  a.stdv = std_out;
  a.part = (double*)ws;
  a.rows_out = rows_out;
  const int blocks = metric_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(metrics_rows_kernel, dim3(blocks), dim3(MT), 0, s, a);
  hipLaunchKernelGGL(metrics_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)a.part, blocks, (long long)n, acc);
  egn_count_launches(2);
  return (int)hipGetLastError();
}
