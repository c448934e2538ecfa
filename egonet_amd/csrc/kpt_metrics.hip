// kpt_metrics.hip -- the key-point model's source-image metric (get_distance_src / JointDistance2DSIP), folded into an
// accumulator that stays on the device.
//
// Reference: libs/metric/criterions.py:68-143 (get_distance_src: decode, rescale to the crop window, inverse crop
// affine per instance, get_distance :17-37, get_PCK :57-66) and its running form JointDistance2DSIP (:173-224).  The
// reference decodes, copies coordinates and maxima to the host and loops over the instances in Python (one 3 x 3
// solve, a 33-point product and four distance passes each); here
//   kpt_metrics_maps_kernel  one wavefront per (n,k) map, four per block like decode_kernel: the decode of
//                            decode_map.h (or the coordinate head's value), the float32 rescale, then in float64
//                            (kpt_metric_math.h) the instance's inverse crop affine, the source point, its distance to
//                            the annotated joint and the three PCK tests against the instance's denominator, which
//                            the wave reduces over the K annotated joints itself; one partial per block, written with
//                            plain stores
//   kpt_metrics_fold_kernel  the block partials added to the accumulator in block order
// No atomics and no hand-off between blocks: the same input gives the same bits.  HBM-bound: every map element is
// read once.  The decoder is compiled under the default contraction, like in decode.hip; the float64 functions of
// kpt_metric_math.h switch contraction off for themselves.
#include "egn_internal.h"
#include "decode_map.h"
#include "kpt_metric_math.h"

namespace {

constexpr int KT = 256;                 // threads per block
constexpr int KWAVES = KT / 64;         // maps per block
constexpr int PS = 8;                   // doubles per partial (>= EGN_KPT_METRIC_STATS): one 64-byte line each
static_assert(PS >= EGN_KPT_METRIC_STATS && PS <= EGN_KPT_METRICS_ACC_DOUBLES, "partial stride");

struct KptArgs {
  const float* hm;          // [N][K][H][W] or NULL
  const float* coords;      // [N][K][2] in [0,1] or NULL
  int nmaps, K, H, W, mode;
  const double* center;     // [n][2]
  const double* scale;      // [n][2]
  const double* rotation;   // [n] degrees, or NULL = 0
  const double* joints;     // [n][K][3]
  int n;                    // labelled instances, <= N
  double img_w, img_h;
  double* part;             // [blocks][PS]
  double* src_coord;        // [n][K][2] or NULL
  float* joints_pred;       // [N][K][2] or NULL
  float* max_vals;          // [N][K] or NULL (heat-maps only)
};

__global__ __launch_bounds__(KT) void kpt_metrics_maps_kernel(KptArgs a) {
  __shared__ double s_part[KWAVES][PS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int map = blockIdx.x * KWAVES + wave;       // the same for the 64 lanes of a wave
  double st[EGN_KPT_METRIC_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (map < a.nmaps) {
    float px, py;
    if (a.hm) {
      float ox, oy, best;
      int bidx;
      egn_decode_map(a.hm + (size_t)map * ((size_t)a.H * a.W), a.H, a.W, a.mode, lane, ox, oy, best, bidx);
      const float f = (float)(a.img_w / (double)a.W);         // numpy: float32 array x Python float
      px = ox * f;
      py = oy * f;
      if (a.max_vals && lane == 0) a.max_vals[map] = best;
    } else {
      px = a.coords[2 * (size_t)map] * (float)a.img_w;
      py = a.coords[2 * (size_t)map + 1] * (float)a.img_h;
    }
    if (a.joints_pred && lane == 0) {
      a.joints_pred[2 * (size_t)map] = px;
      a.joints_pred[2 * (size_t)map + 1] = py;
    }
    const int inst = map / a.K;
    const int k = map - inst * a.K;
    if (inst < a.n) {                               // extra predictions belong to unlabelled data
      const double* gt = a.joints + (size_t)inst * a.K * 3;
      double mx = -INFINITY, mn = INFINITY;         // over ALL K annotated joints, like get_PCK
      for (int j = lane; j < a.K; j += 64) {
        const double y = gt[3 * j + 1];
        mx = fmax(mx, y);
        mn = fmin(mn, y);
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, m));
        mn = fmin(mn, __shfl_xor(mn, m));
      }
      double T[6], src[2];
      egn_kpt_inv_affine(a.center + 2 * (size_t)inst, a.scale + 2 * (size_t)inst,
                         a.rotation ? a.rotation[inst] : 0.0, a.img_w, a.img_h, T);
      egn_kpt_to_source(T, px, py, src);
      egn_kpt_joint_stats(src, gt + 3 * k, egn_kpt_pck_denominator(mx, mn), st);
      if (a.src_coord && lane == 0) {
        a.src_coord[2 * (size_t)map] = src[0];      // map < n * K here
        a.src_coord[2 * (size_t)map + 1] = src[1];
      }
    }
  }
  if (lane == 0) {                                  // every lane of the wave holds the same five values
#pragma unroll
    for (int c = 0; c < PS; ++c) s_part[wave][c] = c < EGN_KPT_METRIC_STATS ? st[c < EGN_KPT_METRIC_STATS ? c : 0] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < PS) {                           // the block's waves, in wave order
    double s = s_part[0][threadIdx.x];
    for (int w = 1; w < KWAVES; ++w) s = s + s_part[w][threadIdx.x];
    a.part[(size_t)blockIdx.x * PS + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void kpt_metrics_fold_kernel(const double* __restrict__ part, int blocks,
                                                              double* __restrict__ acc) {
  const int c = threadIdx.x;
  if (c >= PS) return;
  double s = 0.0;
#pragma unroll 16                 // the loads of 16 partials in flight; the additions stay in block order
  for (int b = 0; b < blocks; ++b) s = s + part[(size_t)b * PS + c];
  acc[c] = acc[c] + s;
}

__global__ __launch_bounds__(64) void kpt_metrics_reset_kernel(double* __restrict__ acc) {
  if (threadIdx.x < EGN_KPT_METRICS_ACC_DOUBLES) acc[threadIdx.x] = 0.0;
}

inline long long kpt_blocks(long long nmaps) { return nmaps < 1 ? 1 : (nmaps + KWAVES - 1) / KWAVES; }

}  // namespace

extern "C" long egn_kpt_metrics_ws_bytes(int N, int K) {
  if (N < 0 || K <= 0 || (long long)N * K > 0x7fffffffLL) return EGN_E_BADARG;
  return (long)(kpt_blocks((long long)N * K) * PS * (long long)sizeof(double));
}

extern "C" int egn_kpt_metrics_reset(double* acc, void* stream) {
  if (!acc) return EGN_E_BADARG;
  hipLaunchKernelGGL(kpt_metrics_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_kpt_metrics_update_f32(const float* hm, const float* coords, int N, int K, int H, int W, int mode,
                                          const double* center, const double* scale, const double* rotation,
                                          const double* original_joints, int n, double img_w, double img_h, void* ws,
                                          long ws_bytes, double* acc, double* src_coord, float* joints_pred,
                                          float* max_vals, void* stream) {
  if ((hm == nullptr) == (coords == nullptr) || N < 0 || K <= 0 || n < 0 || n > N || !ws || !acc ||
      (long long)N * K > 0x7fffffffLL || !(img_w > 0.0) || !(img_h > 0.0))
    return EGN_E_BADARG;
  if (hm && (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || mode < 0 || mode > 2)) return EGN_E_BADARG;
  if (n > 0 && (!center || !scale || !original_joints)) return EGN_E_BADARG;
  if (N == 0) return 0;
  if (ws_bytes < egn_kpt_metrics_ws_bytes(N, K)) return EGN_E_BADARG;
  KptArgs a;
  a.hm = hm;
  a.coords = coords;
  a.nmaps = N * K;
  a.K = K;
  a.H = H;
  a.W = W;
  a.mode = mode;
  a.center = center;
  a.scale = scale;
  a.rotation = rotation;
  a.joints = original_joints;
  a.n = n;
  a.img_w = img_w;
  a.img_h = img_h;
  a.part = (double*)ws;
  a.src_coord = src_coord;
  a.joints_pred = joints_pred;
  a.max_vals = hm ? max_vals : nullptr;
  const int blocks = (int)kpt_blocks(a.nmaps);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kpt_metrics_maps_kernel, dim3(blocks), dim3(KT), 0, s, a);
  hipLaunchKernelGGL(kpt_metrics_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)a.part, blocks, acc);
  egn_count_launches(2);
  return (int)hipGetLastError();
}
