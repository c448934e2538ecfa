// pose_annot.hip -- the 2-D pose annotations of the key-point model (crop box, key points, angles per labelled car),
// built on the device from KITTI label rows and the frames' calibration.
//
// Reference: libs/dataset/KITTI/car_instance.py:221-262 (_prepare_key_points_custom -> get_2d_3d_pair :902-1010 with
// augment False, add_visibility, filter_outlier, add_rotation), :304-346 (_prepare_2d_pose_annot), and
// libs/common/img_proc.py:485-540 (cs2bbox, kpts2cs method 'boundary', target_ar None).  The reference does this per
// label in Python on the host; here, with the structure of lifter_pairs.hip,
//   annot_kernel<false>   every label's visibility count -> the two keep flags, per-block and per-frame counts
//   pairs_scan_kernel     exclusive scan of the block counts + the total, once per level (compact_scan.h)
//   annot_kernel<true>    the same points again, stored at their COMPACTED position; the box from all J points
// The cuboid is the lifter pairs' own (cuboid_math.h); the pose, projection and visibility below restate
// pairs_kernel's arithmetic in its operation order.  All of it is float64 with contraction to FMA off for this file,
// so that every product and sum rounds where numpy's does.
#include "egn_internal.h"
#include "cuboid_math.h"
#include "compact_scan.h"
#pragma clang fp contract(off)

namespace {

constexpr int AG = 32;            // labels per block
constexpr int AJ_MAX = 33;        // 9 + 12 * 2 key points
constexpr int AT = 256;           // threads per block

struct AnnotArgs {
  const double* labels;      // [A][7]  l h w x y z rot_y
  const double* alpha;       // [A]
  const int* label_frame;    // [A]
  const double* frames;      // [F][14] K (row major), shift, width, height
  int A, F, J, min_visible;
  double coef[2];
  double inlier_share, enlarge;
  unsigned char* flags;      // [A]: bit 0 = raw (level 1), bit 1 = kept (level 2)
  int* count_raw;            // [nblk]; after the scan: the exclusive offsets
  int* count_kept;           // [nblk]; likewise
  double* raw_kpts;          // [Nraw][J][3]
  double* kpts;              // [N][J][2]
  int* boxes;                // [N][4]
  double* rots;              // [N][2]
  int* src;                  // [N]
  int* frame_raw;            // [F]
  int* frame_kept;           // [F]
};

// point j of a label through rot_maty, + location, + shift (car_instance.py:785-788), then K (:561-562) and the strict
// visibility test (:862-867): the operation order of pairs_kernel
__device__ inline bool project_point(const double* L, const double* Fm, const double* coef, int j, double cs,
                                     double sn, double& u, double& v) {
  double p[3];
  canon_point(j, L[0], L[1], L[2], coef, p);
  double x = cs * p[0] + sn * p[2];
  double y = p[1];
  double z = -sn * p[0] + cs * p[2];
  x = (x + L[3]) + Fm[9];
  y = (y + L[4]) + Fm[10];
  z = (z + L[5]) + Fm[11];
  const double pu = Fm[0] * x + Fm[1] * y + Fm[2] * z;
  const double pv = Fm[3] * x + Fm[4] * y + Fm[5] * z;
  const double pw = Fm[6] * x + Fm[7] * y + Fm[8] * z;
  u = pu / pw;
  v = pv / pw;
  return u > 0.0 && u < Fm[12] && v > 0.0 && v < Fm[13];
}

// int() of a box corner: toward zero; outside the int32 range (a point next to the camera plane) it saturates
__device__ inline int trunc_i32(double x) {
  if (!(x > -2147483648.0)) return x == x ? (int)0x80000000 : 0;
  if (x >= 2147483647.0) return 0x7fffffff;
  return (int)x;
}

template <bool WRITE>
__global__ __launch_bounds__(AT) void annot_kernel(AnnotArgs a) {
  __shared__ double s_cs[AG], s_sn[AG];
  __shared__ int s_frame[AG];
  __shared__ unsigned char s_vis[AG][AJ_MAX + 3];
  __shared__ int s_raw[AG + 1], s_kept[AG + 1];    // WRITE: row among the block's rows of the level, -1 = dropped
  __shared__ double s_uv[WRITE ? AG : 1][AJ_MAX][2];

  const int J = a.J;
  const int l0 = blockIdx.x * AG;                  // A < 2^31 - 32: no overflow
  const int ng = min(AG, a.A - l0);
  const int tid = threadIdx.x;

  if (tid < ng) {
    const int lab = l0 + tid;
    double sn, cs;
    sincos(a.labels[(size_t)lab * 7 + 6], &sn, &cs);
    s_cs[tid] = cs;
    s_sn[tid] = sn;
    // an index outside [0, F) is the caller's error (the Python builder refuses it); clamped so that it cannot read
    // outside the frame table
    s_frame[tid] = min(max(a.label_frame[lab], 0), a.F - 1);
    if (WRITE) {
      const int f = a.flags[lab];
      s_raw[tid] = f & 1;
      s_kept[tid] = (f >> 1) & 1;
    }
  }
  __syncthreads();
  if (WRITE && tid == 0) {                         // exclusive scans of <= 32 flags
    int r = 0, k = 0;
    for (int g = 0; g < ng; ++g) {
      const int fr = s_raw[g], fk = s_kept[g];
      s_raw[g] = fr ? r : -1;
      s_kept[g] = fk ? k : -1;
      r += fr;
      k += fk;
    }
    s_raw[AG] = r;
    s_kept[AG] = k;
  }
  if (WRITE) __syncthreads();

  const size_t row_raw = WRITE ? (size_t)a.count_raw[blockIdx.x] : 0;
  const size_t row_kept = WRITE ? (size_t)a.count_kept[blockIdx.x] : 0;
  for (int it = tid; it < ng * J; it += AT) {
    const int g = it / J, j = it % J;
    if (WRITE && s_raw[g] < 0) continue;
    const double* L = a.labels + (size_t)(l0 + g) * 7;
    const double* Fm = a.frames + (size_t)s_frame[g] * 14;
    double u, v;
    const bool vis = project_point(L, Fm, a.coef, j, s_cs[g], s_sn[g], u, v);
    if (!WRITE) {
      s_vis[g][j] = vis ? 1 : 0;
    } else {
      double* r = a.raw_kpts + ((row_raw + s_raw[g]) * J + j) * 3;
      r[0] = u;
      r[1] = v;
      r[2] = vis ? 1.0 : 0.0;
      if (s_kept[g] >= 0) {
        double* k = a.kpts + ((row_kept + s_kept[g]) * J + j) * 2;
        k[0] = u;
        k[1] = v;
        s_uv[g][j][0] = u;
        s_uv[g][j][1] = v;
      }
    }
  }
  __syncthreads();

  if (!WRITE) {
    if (tid < ng) {
      int cnt = 0;
      for (int j = 0; j < J; ++j) cnt += s_vis[tid][j];
      const int raw = ((double)cnt / (double)J >= a.inlier_share) ? 1 : 0;   // get_inlier_indices (:870-879)
      const int kept = (raw && cnt >= a.min_visible) ? 1 : 0;               // _prepare_2d_pose_annot (:323-325)
      a.flags[l0 + tid] = (unsigned char)(raw | (kept << 1));
      s_raw[tid] = raw;
      s_kept[tid] = kept;
      // integer adds: the counts do not depend on the order the blocks arrive in
      if (raw) atomicAdd(a.frame_raw + s_frame[tid], 1);
      if (kept) atomicAdd(a.frame_kept + s_frame[tid], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int r = 0, k = 0;
      for (int g = 0; g < ng; ++g) {
        r += s_raw[g];
        k += s_kept[g];
      }
      a.count_raw[blockIdx.x] = r;
      a.count_kept[blockIdx.x] = k;
    }
    return;
  }

  // the crop box of a kept label from ALL J points (every point counts as visible from here on, :327-331):
  // kpts2cs 'boundary' (img_proc.py:524-527), cs2bbox (:489-492), int()
  if (tid < ng && s_kept[tid] >= 0) {
    double mn[2] = {s_uv[tid][0][0], s_uv[tid][0][1]}, mx[2] = {mn[0], mn[1]};
    for (int j = 1; j < J; ++j)
      for (int d = 0; d < 2; ++d) {
        const double c = s_uv[tid][j][d];
        mn[d] = c < mn[d] ? c : mn[d];
        mx[d] = c > mx[d] ? c : mx[d];
      }
    const size_t row = row_kept + s_kept[tid];
    int4 box;
    {
      const double cx = (mn[0] + mx[0]) / 2.0, cy = (mn[1] + mx[1]) / 2.0;
      const double hx = (mx[0] - mn[0]) * a.enlarge / 2.0, hy = (mx[1] - mn[1]) * a.enlarge / 2.0;
      box.x = trunc_i32(cx - hx);
      box.y = trunc_i32(cy - hy);
      box.z = trunc_i32(cx + hx);
      box.w = trunc_i32(cy + hy);
    }
    reinterpret_cast<int4*>(a.boxes)[row] = box;   // [N][4] int32: every row starts on a 16-byte boundary
    a.rots[row * 2 + 0] = a.alpha[l0 + tid];
    a.rots[row * 2 + 1] = a.labels[(size_t)(l0 + tid) * 7 + 6];
    a.src[row] = l0 + tid;
  }
}

inline long round8(long n) { return (n + 7) / 8 * 8; }
inline long annot_blocks(long A) { return (A + AG - 1) / AG; }

}  // namespace

extern "C" long egn_pose2d_annot_ws_bytes(int A) {
  if (A < 0 || A > 0x7fffffff - AG) return EGN_E_BADARG;
  // [nblk] raw block counts -> offsets (int32) | [nblk] kept block counts | [A] flags; each 8-byte rounded, and
  // never empty, so that a caller always has a buffer to pass
  return 8 + 2 * round8(annot_blocks(A) * 4) + round8(A);
}

extern "C" int egn_pose2d_annot_f64(const double* labels, const double* alpha, const int* label_frame, int A,
                                    const double* frames, int F, double coef0, double coef1, int J,
                                    double inlier_share, int min_visible, double enlarge, void* ws, long ws_bytes,
                                    double* raw_kpts, double* kpts, int* boxes, double* rots, int* src, int* frame_raw,
                                    int* frame_kept, int64_t* totals, void* stream) {
  if (A < 0 || F < 0 || (J != 21 && J != AJ_MAX) || !ws || !totals || (F > 0 && (!frame_raw || !frame_kept)))
    return EGN_E_BADARG;
  const long need = egn_pose2d_annot_ws_bytes(A);
  if (need < 0 || ws_bytes < need) return EGN_E_BADARG;
  if (A > 0 && (!labels || !alpha || !label_frame || !frames || F <= 0 || !raw_kpts || !kpts || !boxes || !rots ||
                !src || ((uintptr_t)boxes & 15)))
    return EGN_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (F > 0) {
    EGN_CHECK_HIP(hipMemsetAsync(frame_raw, 0, (size_t)F * sizeof(int), s));
    EGN_CHECK_HIP(hipMemsetAsync(frame_kept, 0, (size_t)F * sizeof(int), s));
  }
  if (A == 0) {
    EGN_CHECK_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s));
    return 0;
  }
  AnnotArgs a;
  a.labels = labels;
  a.alpha = alpha;
  a.label_frame = label_frame;
  a.frames = frames;
  a.A = A;
  a.F = F;
  a.J = J;
  a.min_visible = min_visible;
  a.coef[0] = coef0;
  a.coef[1] = coef1;
  a.inlier_share = inlier_share;
  a.enlarge = enlarge;
  const long nblk = annot_blocks(A);
  char* w = (char*)ws;
  a.count_raw = (int*)w;
  a.count_kept = (int*)(w + round8(nblk * 4));
  a.flags = (unsigned char*)(w + 2 * round8(nblk * 4));
  a.raw_kpts = raw_kpts;
  a.kpts = kpts;
  a.boxes = boxes;
  a.rots = rots;
  a.src = src;
  a.frame_raw = frame_raw;
  a.frame_kept = frame_kept;
  long long* tot = reinterpret_cast<long long*>(totals);
  hipLaunchKernelGGL(annot_kernel<false>, dim3((unsigned)nblk), dim3(AT), 0, s, a);
  hipLaunchKernelGGL(pairs_scan_kernel, dim3(1), dim3(1024), 0, s, a.count_raw, (int)nblk, tot);
  hipLaunchKernelGGL(pairs_scan_kernel, dim3(1), dim3(1024), 0, s, a.count_kept, (int)nblk, tot + 1);
  hipLaunchKernelGGL(annot_kernel<true>, dim3((unsigned)nblk), dim3(AT), 0, s, a);
  egn_count_launches(4);
  return (int)hipGetLastError();
}
