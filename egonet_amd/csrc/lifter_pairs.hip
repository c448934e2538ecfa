// lifter_pairs.hip -- the lifter's (2-D key points, 3-D cuboid) training pairs, built and kept on the device.
//
// Reference: libs/dataset/KITTI/car_instance.py:611-644 (augment_pose_vector), :730-790 (construct_box_3d, interpolate,
// get_cam_cord), :902-1010 (get_2d_3d_pair: projection, visibility, the 0.3 filter), :646-686 (get_representation),
// :1051-1086, then libs/dataset/basic/basic_classes.py:26-44 + normalization/operations.py (statistics, normalise).
// The reference does this per label in Python on the host; here
//   pairs_kernel<false>   every sample's visibility count -> keep flag, per-block kept counts
//   pairs_scan_kernel     exclusive scan of the block counts (one block, fixed order) + the total
//   pairs_kernel<true>    the same points again, rows staged in LDS and stored at their COMPACTED position
//   colsum / finalize     column mean and population deviation, float64 from the first add, fixed order
//   normalize_rows        (x - mean) / std in float32, correctly rounded
//   gather_rows           dst[i] = src[idx[i]]: the per-batch fetch
// All point arithmetic is float64 with one rounding to float32 at the LDS store; contraction to FMA is off for this
// file so that every product and sum rounds where numpy's does (the reference's BLAS / libm may still differ in the
// last float64 bit).  No fast-math: the float32 division of normalize_rows must be the IEEE one.
#include "egn_internal.h"
#include "pose_math.h"
#include "cuboid_math.h"       // canon_point
#include "compact_scan.h"      // pairs_scan_kernel
#pragma clang fp contract(off)

namespace {

constexpr int PG = 32;            // samples per block
constexpr int PJ_MAX = 33;        // 9 + 12 * 2 key points
constexpr int PT = 256;           // threads per block
constexpr int ST_BLOCKS = 2048;   // most partial rows of a column reduction
constexpr int ST_T = 128;         // threads of the column reduction (>= columns)

struct PairArgs {
  const double* labels;      // [A][7]  l h w x y z rot_y
  const int* label_frame;    // [A]
  const double* frames;      // [F][14] K (row major), shift, width, height
  const double* draws;       // [A][7T+1] or NULL: T x 3 rotation, T x 3 translation, T + 1 yaw draws
  int F, T, J, out_root;             // out_root: 1 = 'R3d+T' (root first, 3J values), 0 = 'R3d' (3(J-1))
  double coef[2];
  double std_rot_y;          // 50 deg, as the reference computes it
  long long NS;              // A * (T + 1)
  unsigned char* keep;       // [NS]
  int* block_count;          // [nblk]; after the scan: the exclusive offsets
  float* in2d;               // [N][2J]
  float* out3d;              // [N][3(J-1) | 3J]
  double* roots;             // [N][3]
};

template <bool WRITE>
__global__ __launch_bounds__(PT) void pairs_kernel(PairArgs a) {
  __shared__ double s_pose[PG][8];                 // cos, sin, tx, ty, tz of a sample; 5 = label, 6 = frame
  __shared__ unsigned char s_vis[PG][PJ_MAX + 3];
  __shared__ int s_slot[PG + 1];                   // WRITE: row of the sample among the block's kept rows
  __shared__ double s_cam[WRITE ? PG : 1][PJ_MAX][3];
  __shared__ __align__(16) float s_in[WRITE ? PG * 2 * PJ_MAX : 4];
  __shared__ __align__(16) float s_out[WRITE ? PG * 3 * PJ_MAX : 4];
  __shared__ double s_root[WRITE ? PG * 3 : 1];

  const int S = a.T + 1, J = a.J;
  const long long s0 = (long long)blockIdx.x * PG;
  const int ng = (int)min((long long)PG, a.NS - s0);
  const int tid = threadIdx.x;

  if (tid < ng) {                                  // the pose of sample s0 + tid (car_instance.py:630-643, 759-768)
    const long long s = s0 + tid;
    const int lab = (int)(s / S), i = (int)(s % S);
    const double* L = a.labels + (size_t)lab * 7;
    double tx = L[3], ty = L[4], tz = L[5], ry = L[6];
    const double* d = a.draws ? a.draws + (size_t)lab * (7 * a.T + 1) : nullptr;
    if (i > 0) {                                   // the x / z rotation draws are consumed and unused (rot_xz False)
      ry = d[(i - 1) * 3 + 1] * a.std_rot_y + ry;
      const double* t = d + 3 * a.T + (i - 1) * 3;
      tx = (1.0 + t[0] * 0.2) * tx;
      ty = (1.0 + t[1] * 0.01) * ty;
      tz = (1.0 + t[2] * 0.2) * tz;
    }
    if (d) ry += d[6 * a.T + i] * 3.141592653589793;
    double sn, cs;
    sincos(ry, &sn, &cs);
    s_pose[tid][0] = cs;
    s_pose[tid][1] = sn;
    s_pose[tid][2] = tx;
    s_pose[tid][3] = ty;
    s_pose[tid][4] = tz;
    s_pose[tid][5] = (double)lab;
    // an index outside [0, F) is the caller's error (the Python builder refuses it); clamped so that it cannot read
    // outside the frame table
    s_pose[tid][6] = (double)min(max(a.label_frame[lab], 0), a.F - 1);
    if (WRITE) s_slot[tid] = a.keep[s];
  }
  __syncthreads();
  if (WRITE && tid == 0) {                         // exclusive scan of <= 32 flags
    int run = 0;
    for (int g = 0; g < ng; ++g) {
      const int k = s_slot[g];
      s_slot[g] = k ? run : -1;
      run += k;
    }
    s_slot[PG] = run;
  }
  if (WRITE) __syncthreads();

  for (int it = tid; it < ng * J; it += PT) {
    const int g = it / J, j = it % J;
    if (WRITE && s_slot[g] < 0) continue;
    const double* L = a.labels + (size_t)s_pose[g][5] * 7;
    const double* Fm = a.frames + (size_t)s_pose[g][6] * 14;
    double p[3];
    canon_point(j, L[0], L[1], L[2], a.coef, p);
    const double cs = s_pose[g][0], sn = s_pose[g][1];
    // rot_maty @ corners, + location, + shift (car_instance.py:785-788)
    double x = cs * p[0] + sn * p[2];
    double y = p[1];
    double z = -sn * p[0] + cs * p[2];
    x = (x + s_pose[g][2]) + Fm[9];
    y = (y + s_pose[g][3]) + Fm[10];
    z = (z + s_pose[g][4]) + Fm[11];
    const double pu = Fm[0] * x + Fm[1] * y + Fm[2] * z;
    const double pv = Fm[3] * x + Fm[4] * y + Fm[5] * z;
    const double pw = Fm[6] * x + Fm[7] * y + Fm[8] * z;
    const double u = pu / pw, v = pv / pw;
    if (!WRITE) {
      s_vis[g][j] = (u > 0.0 && u < Fm[12] && v > 0.0 && v < Fm[13]) ? 1 : 0;
    } else {
      const int k = s_slot[g];
      s_in[(k * J + j) * 2 + 0] = (float)u;
      s_in[(k * J + j) * 2 + 1] = (float)v;
      s_cam[g][j][0] = x;
      s_cam[g][j][1] = y;
      s_cam[g][j][2] = z;
    }
  }
  __syncthreads();

  if (!WRITE) {
    if (tid < ng) {
      int cnt = 0;
      for (int j = 0; j < J; ++j) cnt += s_vis[tid][j];
      const int k = ((double)cnt / (double)J >= 0.3) ? 1 : 0;     // get_inlier_indices, threshold 0.3
      a.keep[s0 + tid] = (unsigned char)k;
      s_slot[tid] = k;
    }
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int g = 0; g < ng; ++g) run += s_slot[g];
      a.block_count[blockIdx.x] = run;
    }
    return;
  }

  // 3-D rows (get_representation, car_instance.py:663-683): relative to the root, the root itself kept aside
  const int OC = a.out_root ? 3 * J : 3 * (J - 1);
  for (int it = tid; it < ng * J; it += PT) {
    const int g = it / J, j = it % J;
    const int k = s_slot[g];
    if (k < 0) continue;
    if (j == 0) {
      for (int d = 0; d < 3; ++d) {
        s_root[k * 3 + d] = s_cam[g][0][d];
        if (a.out_root) s_out[k * OC + d] = (float)s_cam[g][0][d];
      }
    } else {
      const int o = k * OC + (a.out_root ? j : j - 1) * 3;
      for (int d = 0; d < 3; ++d) s_out[o + d] = (float)(s_cam[g][j][d] - s_cam[g][0][d]);
    }
  }
  __syncthreads();

  // the block's kept rows are one contiguous span of the compacted arrays: lane-consecutive vector stores
  const int cnt = s_slot[PG];
  const size_t row0 = (size_t)a.block_count[blockIdx.x];
  {
    // 2J floats per row: the span starts on an 8-byte boundary
    float2* dst = reinterpret_cast<float2*>(a.in2d + row0 * 2 * J);
    const float2* src = reinterpret_cast<const float2*>(s_in);
    for (int e = tid; e < cnt * J; e += PT) dst[e] = src[e];
  }
  if (OC % 4 == 0) {                               // 96 floats: 16-byte stores
    float4* dst = reinterpret_cast<float4*>(a.out3d + row0 * OC);
    const float4* src = reinterpret_cast<const float4*>(s_out);
    for (int e = tid; e < cnt * (OC / 4); e += PT) dst[e] = src[e];
  } else {                                         // 99 floats: a span may start on any 4-byte boundary
    float* dst = a.out3d + row0 * OC;
    for (int e = tid; e < cnt * OC; e += PT) dst[e] = s_out[e];
  }
  {
    double* dst = a.roots + row0 * 3;
    for (int e = tid; e < cnt * 3; e += PT) dst[e] = s_root[e];
  }
}

// column sums of x [N][C] float32 in float64: block b adds rows b, b + B, ... in that order, thread c owns column c.
// center != NULL: sums of (x - center)^2.  part [B][C].
__global__ __launch_bounds__(ST_T) void colsum_kernel(const float* __restrict__ x, long long N, int C,
                                                      const double* __restrict__ center, double* __restrict__ part) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const double m = center ? center[c] : 0.0;
  double acc = 0.0;
#pragma unroll 4
  for (long long r = blockIdx.x; r < N; r += gridDim.x) {
    const double v = (double)x[(size_t)r * C + c];
    if (center) {
      const double d = v - m;
      acc += d * d;
    } else {
      acc += v;
    }
  }
  part[(size_t)blockIdx.x * C + c] = acc;
}

// mode 0: mean64[c] = sum / N.  mode 1: std = sqrt(sum / N) (np.std, ddof 0); writes the float32 mean and deviation
__global__ __launch_bounds__(ST_T) void colstat_finalize_kernel(const double* __restrict__ part, int B, int C,
                                                                long long N, int mode, double* __restrict__ mean64,
                                                                float* __restrict__ mean, float* __restrict__ stdv) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc += part[(size_t)b * C + c];
  if (mode == 0) {
    mean64[c] = acc / (double)N;
  } else {
    mean[c] = (float)mean64[c];
    stdv[c] = (float)sqrt(acc / (double)N);
  }
}

template <typename V> struct VecOps;
template <> struct VecOps<float> {
  static constexpr int W = 1;
  __device__ static float norm(float x, const float* m, const float* s, int c) { return (x - m[c]) / s[c]; }
};
template <> struct VecOps<float2> {
  static constexpr int W = 2;
  __device__ static float2 norm(float2 x, const float* m, const float* s, int c) {
    return make_float2((x.x - m[c]) / s[c], (x.y - m[c + 1]) / s[c + 1]);
  }
};
template <> struct VecOps<float4> {
  static constexpr int W = 4;
  __device__ static float4 norm(float4 x, const float* m, const float* s, int c) {
    return make_float4((x.x - m[c]) / s[c], (x.y - m[c + 1]) / s[c + 1], (x.z - m[c + 2]) / s[c + 2],
                       (x.w - m[c + 3]) / s[c + 3]);
  }
};

// operations.py:47 on float32 arrays: a float32 subtraction, then a float32 division, both correctly rounded
template <typename V>
__global__ __launch_bounds__(256) void normalize_rows_kernel(V* __restrict__ x, size_t nvec, int cv,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ stdv) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nvec; e += (size_t)gridDim.x * blockDim.x)
    x[e] = VecOps<V>::norm(x[e], mean, stdv, (int)(e % cv) * VecOps<V>::W);
}

// dst[i][:] = src[idx[i]][:]; an index outside [0, nrows) gives a row of zeros (never an out-of-bounds read)
template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(const V* __restrict__ src, long long nrows, int cv,
                                                          const long long* __restrict__ idx, size_t nvec,
                                                          V* __restrict__ dst) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nvec; e += (size_t)gridDim.x * blockDim.x) {
    const size_t i = e / cv;
    const int c = (int)(e % cv);
    const long long r = idx[i];
    V v = {};
    if (r >= 0 && r < nrows) v = src[(size_t)r * cv + c];
    dst[e] = v;
  }
}

inline unsigned grid_for(size_t n, unsigned cap) {
  size_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// widest vector (floats) that divides the row and keeps every row start aligned
inline int vec_width(int C, const void* a, const void* b) {
  const uintptr_t p = (uintptr_t)a | (uintptr_t)b;
  if (C % 4 == 0 && p % 16 == 0) return 4;
  if (C % 2 == 0 && p % 8 == 0) return 2;
  return 1;
}

}  // namespace

static inline long long pairs_blocks(long long NS) { return (NS + PG - 1) / PG; }

extern "C" long egn_lifter_pairs_ws_bytes(int A, int T) {
  if (A <= 0 || T < 0) return EGN_E_BADARG;
  const long long NS = (long long)A * (T + 1);
  if (NS > 0x7fffffffLL) return EGN_E_BADARG;
  // [8] total (int64) | [nblk] block counts -> offsets (int32), 8-byte rounded | [NS] keep flags
  return (long)(8 + ((pairs_blocks(NS) * 4 + 7) / 8) * 8 + NS);
}

extern "C" int egn_lifter_pairs_f64(const double* labels, const int* label_frame, int A, const double* frames, int F,
                                    const double* draws, int T, double coef0, double coef1, int ncoef, int out_root,
                                    void* ws, long ws_bytes, float* in2d, float* out3d, double* roots,
                                    void* stream) {
  if (!labels || !label_frame || !frames || !ws || !in2d || !out3d || !roots || A <= 0 || F <= 0 || T < 0 ||
      ncoef < 1 || ncoef > 2 || (T > 0 && !draws))
    return EGN_E_BADARG;
  const long need = egn_lifter_pairs_ws_bytes(A, T);
  if (need < 0 || ws_bytes < need) return EGN_E_BADARG;     // more than 2^31 - 1 samples: build in parts
  PairArgs a;
  a.labels = labels;
  a.label_frame = label_frame;
  a.frames = frames;
  a.draws = draws;
  a.F = F;
  a.T = T;
  a.J = 9 + 12 * ncoef;
  a.out_root = out_root ? 1 : 0;
  a.coef[0] = coef0;
  a.coef[1] = coef1;
  a.std_rot_y = 50.0 * 3.141592653589793 / 180.0;           // (np.array([15., 50., 15.]) * np.pi / 180.)[1]
  a.NS = (long long)A * (T + 1);
  const long long nblk = pairs_blocks(a.NS);
  char* w = (char*)ws;
  long long* total = (long long*)w;
  a.block_count = (int*)(w + 8);
  a.keep = (unsigned char*)(w + 8 + ((nblk * 4 + 7) / 8) * 8);
  a.in2d = in2d;
  a.out3d = out3d;
  a.roots = roots;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pairs_kernel<false>, dim3((unsigned)nblk), dim3(PT), 0, s, a);
  hipLaunchKernelGGL(pairs_scan_kernel, dim3(1), dim3(1024), 0, s, a.block_count, (int)nblk, total);
  hipLaunchKernelGGL(pairs_kernel<true>, dim3((unsigned)nblk), dim3(PT), 0, s, a);
  egn_count_launches(3);
  return (int)hipGetLastError();
}

extern "C" long egn_col_mean_std_ws_bytes(int C) {
  if (C <= 0 || C > ST_T) return EGN_E_BADARG;
  return (long)((size_t)(ST_BLOCKS + 1) * C * sizeof(double));
}

extern "C" int egn_col_mean_std_f32(const float* x, long N, int C, void* ws, long ws_bytes, float* mean, float* stdv,
                                    void* stream) {
  if (!x || !ws || !mean || !stdv || N <= 0 || C <= 0 || C > ST_T || ws_bytes < egn_col_mean_std_ws_bytes(C))
    return EGN_E_BADARG;
  double* part = (double*)ws;
  double* mean64 = part + (size_t)ST_BLOCKS * C;
  const int B = (int)((N + 63) / 64 < ST_BLOCKS ? (N + 63) / 64 : ST_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_kernel, dim3(B), dim3(ST_T), 0, s, x, (long long)N, C, (const double*)nullptr, part);
  hipLaunchKernelGGL(colstat_finalize_kernel, dim3(1), dim3(ST_T), 0, s, part, B, C, (long long)N, 0, mean64, mean,
                     stdv);
  hipLaunchKernelGGL(colsum_kernel, dim3(B), dim3(ST_T), 0, s, x, (long long)N, C, (const double*)mean64, part);
  hipLaunchKernelGGL(colstat_finalize_kernel, dim3(1), dim3(ST_T), 0, s, part, B, C, (long long)N, 1, mean64, mean,
                     stdv);
  egn_count_launches(4);
  return (int)hipGetLastError();
}

extern "C" int egn_normalize_rows_f32(float* x, long N, int C, const float* mean, const float* stdv, void* stream) {
  if (!x || !mean || !stdv || N <= 0 || C <= 0) return EGN_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int W = vec_width(C, x, x);
  const size_t nvec = (size_t)N * (C / W);
  const unsigned g = grid_for(nvec, 16384);
  if (W == 4)
    hipLaunchKernelGGL(normalize_rows_kernel<float4>, dim3(g), dim3(256), 0, s, (float4*)x, nvec, C / 4, mean, stdv);
  else if (W == 2)
    hipLaunchKernelGGL(normalize_rows_kernel<float2>, dim3(g), dim3(256), 0, s, (float2*)x, nvec, C / 2, mean, stdv);
  else
    hipLaunchKernelGGL(normalize_rows_kernel<float>, dim3(g), dim3(256), 0, s, x, nvec, C, mean, stdv);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_gather_rows_f32(const float* src, long nrows, int C, const int64_t* idx, int n, float* dst,
                                   void* stream) {
  if (!src || !idx || !dst || nrows <= 0 || C <= 0 || n <= 0) return EGN_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int W = vec_width(C, src, dst);
  const size_t nvec = (size_t)n * (C / W);
  const unsigned g = grid_for(nvec, 16384);
  const long long* ix = (const long long*)idx;
  if (W == 4)
    hipLaunchKernelGGL(gather_rows_kernel<float4>, dim3(g), dim3(256), 0, s, (const float4*)src, (long long)nrows,
                       C / 4, ix, nvec, (float4*)dst);
  else if (W == 2)
    hipLaunchKernelGGL(gather_rows_kernel<float2>, dim3(g), dim3(256), 0, s, (const float2*)src, (long long)nrows,
                       C / 2, ix, nvec, (float2*)dst);
  else
    hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(g), dim3(256), 0, s, src, (long long)nrows, C, ix, nvec, dst);
  egn_count_launches(1);
  return (int)hipGetLastError();
}
