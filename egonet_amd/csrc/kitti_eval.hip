// kitti_eval.hip -- the KITTI object evaluator (2D AP / AOS, bird's-eye-view AP, 3D AP) on the device.
//
// Reference: tools/kitti-eval/evaluate_object_3d_offline.cpp.  The reference recomputes the overlap of a (detection,
// ground truth) pair inside computeStatistics (:503, :582), which eval_class (:622-706) calls once per frame for the
// recall pass and once per frame and score threshold (up to 41) for the precision pass, for 3 levels, 3 classes and 3
// metrics.  Here
//   kitti_overlap_kernel    one thread per (detection, ground truth) pair of all frames: the three overlaps of
//                           kitti_overlap_math.h, over the union -- over the detection where the row is a DontCare
//                           area, the only criterion such a row is ever asked for -- into one table [3][pairs]
//   kitti_recall_kernel     one thread per (frame, combination): computeStatistics without false positives over that
//                           table; the true-positive scores and the number of counted ground truths
//   (host)                  one read-back of the scores; getThresholds per combination, as on the host path
//   kitti_precision_kernel  one wavefront per (frame, combination), lane = score threshold (at most 41): every lane
//                           runs its own greedy loop with its own assigned-detection set.  tp / fp / fn are added to
//                           the combination's integer totals; the similarity sum of the frame is stored per lane
//   kitti_fold_kernel       one thread per (class, level, threshold): the per-frame similarity partials added in
//                           frame order, the order of the host loop
// The matching loop itself is egn_kitti_match of kitti_eval_core.h, the function the host path runs.
//
// No capacity: an assigned-detection set is ceil(n_det / 32) words per lane in the workspace, interleaved by lane so
// that the 64 lanes of a wave touch one 256-byte line per word; any number of detections and ground truths per frame
// works, zero included.  Integer totals use integer atomics and the similarity is folded in a fixed order, so equal
// inputs give equal bits.  Launches (4) and synchronisations (2) do not depend on the number of frames.  The orientation
// similarity of a pair is evaluated on the host (similarity_table) and travels with the packed copy: the device cos()
// and the host's differ in the last place, and the sums are compared bit for bit.
#include <string.h>

#include <vector>

#include "egn_internal.h"
#include "kitti_eval_core.h"

namespace {

constexpr int KT = 256;
constexpr int KWAVES = KT / 64;
constexpr int COMBOS = EGN_KITTI_COMBOS;
constexpr int SAMPLES = EGN_KITTI_SAMPLES;

struct EvalArgs {
  EgnKittiView v;
  unsigned active;          // bit per combination
  int with_aos;
  double* ov;               // [3][pairs], written by the overlap kernel
  unsigned* taken;          // [word_off[nf] * COMBOS][64]
  double* tp_scores;        // [COMBOS][n_gt]: frame f's at gt_off[f] ...
  int* tp_count;            // [COMBOS][nf]
  int* gt_count;            // [COMBOS][nf]
  const double* thresholds; // [COMBOS][SAMPLES]
  const int* n_thresholds;  // [COMBOS]
  int* counts;              // [COMBOS][SAMPLES][3]
  double* sim_part;         // [9][nf][SAMPLES]
  double* sim_sum;          // [9][SAMPLES]
};

__global__ __launch_bounds__(KT) void kitti_overlap_kernel(EvalArgs a) {
  const long long p = (long long)blockIdx.x * KT + threadIdx.x;
  if (p >= a.v.pairs) return;
  int lo = 0, hi = a.v.nf - 1;                   // the frame with pair_off[f] <= p < pair_off[f + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.v.pair_off[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  const int f = lo;
  const int nd = a.v.det_off[f + 1] - a.v.det_off[f];
  const long long r = p - a.v.pair_off[f];
  const int i = (int)(r / nd), j = (int)(r - (long long)i * nd);
  const int gi = a.v.gt_off[f] + i;
  double o[4];
  egn_kitti_overlaps(a.v.det_box + (long long)(a.v.det_off[f] + j) * EGN_KITTI_BOX,
                     a.v.gt_box + (long long)gi * EGN_KITTI_BOX, a.v.gt_type[gi] == EGN_KT_DONTCARE ? 0 : -1, o);
  a.ov[p] = o[0];
  a.ov[a.v.pairs + p] = o[1];
  a.ov[2 * a.v.pairs + p] = o[2];
}

// the assigned-detection words of (frame f, combination), lane 0
__device__ inline unsigned* taken_words(const EvalArgs& a, int f, int combo) {
  const int nw = a.v.word_off[f + 1] - a.v.word_off[f];
  return a.taken + ((long long)a.v.word_off[f] * COMBOS + (long long)combo * nw) * 64;
}

__global__ __launch_bounds__(KT) void kitti_recall_kernel(EvalArgs a) {
  const long long task = (long long)blockIdx.x * KT + threadIdx.x;
  if (task >= (long long)a.v.nf * COMBOS) return;
  const int f = (int)(task / COMBOS), combo = (int)(task - (long long)f * COMBOS);
  if (!(a.active >> combo & 1u)) return;
  const int metric = combo / 9, cls = combo / 3 % 3, level = combo % 3;
  const long long n_gt = a.v.gt_off[a.v.nf];
  EgnKittiCounts c;
  egn_kitti_match<false>(a.v, f, cls, level, metric, false, 0.0, taken_words(a, f, combo), 64,
                         a.tp_scores + combo * n_gt + a.v.gt_off[f], c);
  a.tp_count[(long long)combo * a.v.nf + f] = c.tp;
  a.gt_count[(long long)combo * a.v.nf + f] = c.n_gt;
}

__global__ __launch_bounds__(KT) void kitti_precision_kernel(EvalArgs a) {
  const int lane = threadIdx.x & 63;
  const long long task = (long long)blockIdx.x * KWAVES + (threadIdx.x >> 6);
  if (task >= (long long)a.v.nf * COMBOS) return;
  const int f = (int)(task / COMBOS), combo = (int)(task - (long long)f * COMBOS);
  if (!(a.active >> combo & 1u) || lane >= a.n_thresholds[combo]) return;
  const int metric = combo / 9, cls = combo / 3 % 3, level = combo % 3;
  const bool with_aos = metric == 0 && a.with_aos;
  EgnKittiCounts c;
  egn_kitti_match<true>(a.v, f, cls, level, metric, with_aos, a.thresholds[combo * SAMPLES + lane],
                        taken_words(a, f, combo) + lane, 64, nullptr, c);
  int* counts = a.counts + (combo * SAMPLES + lane) * 3;
  if (c.tp) atomicAdd(counts, c.tp);
  if (c.fp) atomicAdd(counts + 1, c.fp);
  if (c.fn) atomicAdd(counts + 2, c.fn);
  if (with_aos) a.sim_part[((long long)combo * a.v.nf + f) * SAMPLES + lane] = c.similarity != -1 ? c.similarity : 0.0;
}

__global__ __launch_bounds__(KT) void kitti_fold_kernel(EvalArgs a) {
  const int k = blockIdx.x * KT + threadIdx.x;          // (class * 3 + level) * SAMPLES + threshold: IMAGE combinations
  if (k >= 9 * SAMPLES) return;
  const int combo = k / SAMPLES, t = k - combo * SAMPLES;
  double s = 0.0;
  if (a.with_aos && (a.active >> combo & 1u) && t < a.n_thresholds[combo]) {
    const double* part = a.sim_part + (long long)combo * a.v.nf * SAMPLES + t;
#pragma unroll 8                  // eight loads in flight; the additions stay in frame order
    for (int f = 0; f < a.v.nf; ++f) s = s + part[(long long)f * SAMPLES];
  }
  a.sim_sum[k] = s;
}

__global__ __launch_bounds__(KT) void kitti_overlap_pairs_kernel(const double* __restrict__ det,
                                                                 const double* __restrict__ gt, long n, int criterion,
                                                                 double* __restrict__ out) {
  const long k = (long)blockIdx.x * KT + threadIdx.x;
  if (k >= n) return;
  double o[4];
  egn_kitti_overlaps(det + k * EGN_KITTI_BOX, gt + k * EGN_KITTI_BOX, criterion, o);
  for (int c = 0; c < 4; ++c) out[4 * k + c] = o[c];
}

// Carves the device workspace: every region starts on a 256-byte line.
struct Carver {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  }
};

int evaluate_device(const egn_kitti::Packed& p, int metrics, hipStream_t stream, egn_kitti::Result& r) {
  egn_kitti::scored(p, metrics, r);
  const int nf = p.nf();
  const long long n_gt = p.gt_off.back(), n_det = p.det_off.back(), pairs = p.pair_off.back();
  const long long words = p.word_off.back();
  unsigned active = 0;
  for (int combo = 0; combo < COMBOS; ++combo)
    if (r.evaluated[combo / 3]) active |= 1u << combo;
  if (!active || nf == 0) return 0;
  const bool with_aos = r.aos_valid && (active & 0x1ffu);
  std::vector<double> sim;
  if (with_aos) sim = egn_kitti::similarity_table(p);

  // one staging buffer, one copy up
  Carver in;
  const size_t o_gt_off = in.take(sizeof(int) * (nf + 1)), o_det_off = in.take(sizeof(int) * (nf + 1));
  const size_t o_pair_off = in.take(sizeof(long long) * (nf + 1)), o_word_off = in.take(sizeof(int) * (nf + 1));
  const size_t o_gt_box = in.take(sizeof(double) * n_gt * EGN_KITTI_BOX), o_gt_trunc = in.take(sizeof(double) * n_gt);
  const size_t o_gt_type = in.take(sizeof(int) * n_gt), o_gt_occ = in.take(sizeof(int) * n_gt);
  const size_t o_det_box = in.take(sizeof(double) * n_det * EGN_KITTI_BOX);
  const size_t o_det_score = in.take(sizeof(double) * n_det), o_det_type = in.take(sizeof(int) * n_det);
  const size_t o_sim = in.take(with_aos ? sizeof(double) * pairs : 0);
  Carver ws = in;
  const size_t o_ov = ws.take(sizeof(double) * 3 * pairs);
  const size_t o_taken = ws.take(sizeof(unsigned) * words * COMBOS * 64);
  const size_t o_back = ws.at;                                     // read back after the recall pass, in one copy
  const size_t o_scores = ws.take(sizeof(double) * COMBOS * n_gt);
  const size_t o_tp_count = ws.take(sizeof(int) * COMBOS * nf), o_gt_count = ws.take(sizeof(int) * COMBOS * nf);
  const size_t back_bytes = ws.at - o_back;
  const size_t o_thr = ws.take(sizeof(double) * COMBOS * SAMPLES + sizeof(int) * COMBOS);   // one copy up
  const size_t o_out = ws.at;                                      // read back at the end, in one copy
  const size_t o_counts = ws.take(sizeof(int) * COMBOS * SAMPLES * 3);
  const size_t o_sim_sum = ws.take(sizeof(double) * 9 * SAMPLES);
  const size_t out_bytes = ws.at - o_out;
  const size_t o_sim_part = ws.take(with_aos ? sizeof(double) * 9 * nf * SAMPLES : 0);

  std::vector<char> stage(in.at);
  auto put = [&](size_t at, const void* src, size_t bytes) {
    if (bytes) memcpy(stage.data() + at, src, bytes);
  };
  put(o_gt_off, p.gt_off.data(), sizeof(int) * (nf + 1));
  put(o_det_off, p.det_off.data(), sizeof(int) * (nf + 1));
  put(o_pair_off, p.pair_off.data(), sizeof(long long) * (nf + 1));
  put(o_word_off, p.word_off.data(), sizeof(int) * (nf + 1));
  put(o_gt_box, p.gt_box.data(), sizeof(double) * p.gt_box.size());
  put(o_gt_trunc, p.gt_trunc.data(), sizeof(double) * n_gt);
  put(o_gt_type, p.gt_type.data(), sizeof(int) * n_gt);
  put(o_gt_occ, p.gt_occ.data(), sizeof(int) * n_gt);
  put(o_det_box, p.det_box.data(), sizeof(double) * p.det_box.size());
  put(o_det_score, p.det_score.data(), sizeof(double) * n_det);
  put(o_det_type, p.det_type.data(), sizeof(int) * n_det);
  if (with_aos) put(o_sim, sim.data(), sizeof(double) * pairs);

  char* dev = nullptr;
  EGN_CHECK_HIP(hipMalloc((void**)&dev, ws.at));
  struct Free {
    char* p;
    ~Free() { (void)hipFree(p); }
  } guard{dev};

  EvalArgs a;
  a.v.nf = nf;
  a.v.gt_off = (const int*)(dev + o_gt_off);
  a.v.det_off = (const int*)(dev + o_det_off);
  a.v.pair_off = (const long long*)(dev + o_pair_off);
  a.v.word_off = (const int*)(dev + o_word_off);
  a.v.gt_box = (const double*)(dev + o_gt_box);
  a.v.gt_trunc = (const double*)(dev + o_gt_trunc);
  a.v.gt_type = (const int*)(dev + o_gt_type);
  a.v.gt_occ = (const int*)(dev + o_gt_occ);
  a.v.det_box = (const double*)(dev + o_det_box);
  a.v.det_score = (const double*)(dev + o_det_score);
  a.v.det_type = (const int*)(dev + o_det_type);
  a.v.ov = (const double*)(dev + o_ov);
  a.v.sim = with_aos ? (const double*)(dev + o_sim) : nullptr;
  a.v.pairs = pairs;
  a.active = active;
  a.with_aos = with_aos ? 1 : 0;
  a.ov = (double*)(dev + o_ov);
  a.taken = (unsigned*)(dev + o_taken);
  a.tp_scores = (double*)(dev + o_scores);
  a.tp_count = (int*)(dev + o_tp_count);
  a.gt_count = (int*)(dev + o_gt_count);
  a.thresholds = (const double*)(dev + o_thr);
  a.n_thresholds = (const int*)(dev + o_thr + sizeof(double) * COMBOS * SAMPLES);
  a.counts = (int*)(dev + o_counts);
  a.sim_part = (double*)(dev + o_sim_part);
  a.sim_sum = (double*)(dev + o_sim_sum);

  const long long tasks = (long long)nf * COMBOS;
  EGN_CHECK_HIP(hipMemcpyAsync(dev, stage.data(), in.at, hipMemcpyHostToDevice, stream));
  EGN_CHECK_HIP(hipMemsetAsync(dev + o_back, 0, ws.at - o_back, stream));   // counts of skipped combinations read 0
  if (pairs > 0) {
    hipLaunchKernelGGL(kitti_overlap_kernel, dim3((unsigned)((pairs + KT - 1) / KT)), dim3(KT), 0, stream, a);
    egn_count_launches(1);
  }
  hipLaunchKernelGGL(kitti_recall_kernel, dim3((unsigned)((tasks + KT - 1) / KT)), dim3(KT), 0, stream, a);
  egn_count_launches(1);
  EGN_CHECK_HIP(hipGetLastError());
  std::vector<char> back(back_bytes);
  EGN_CHECK_HIP(hipMemcpyAsync(back.data(), dev + o_back, back_bytes, hipMemcpyDeviceToHost, stream));
  EGN_CHECK_HIP(hipStreamSynchronize(stream));

  // getThresholds per combination, on the host as on the host path
  const double* scores = (const double*)back.data();
  const int* tp_count = (const int*)(back.data() + (o_tp_count - o_back));
  const int* gt_count = (const int*)(back.data() + (o_gt_count - o_back));
  std::vector<char> thr_stage(sizeof(double) * COMBOS * SAMPLES + sizeof(int) * COMBOS, 0);
  double* thr = (double*)thr_stage.data();
  int* n_thr = (int*)(thr_stage.data() + sizeof(double) * COMBOS * SAMPLES);
  for (int combo = 0; combo < COMBOS; ++combo) {
    if (!(active >> combo & 1u)) continue;
    std::vector<double> v;
    int total_gt = 0;
    for (int f = 0; f < nf; ++f) {
      const double* s = scores + combo * n_gt + p.gt_off[f];
      v.insert(v.end(), s, s + tp_count[(long long)combo * nf + f]);
      total_gt += gt_count[(long long)combo * nf + f];
    }
    std::vector<double> t = egn_kitti::recall_thresholds(v, total_gt);
    if (t.size() > (size_t)SAMPLES) t.resize(SAMPLES);
    n_thr[combo] = (int)t.size();
    for (size_t k = 0; k < t.size(); ++k) thr[combo * SAMPLES + k] = t[k];
    r.n_thresholds[combo] = n_thr[combo];
    r.n_gt[combo] = total_gt;
  }
  EGN_CHECK_HIP(hipMemcpyAsync(dev + o_thr, thr_stage.data(), thr_stage.size(), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(kitti_precision_kernel, dim3((unsigned)((tasks + KWAVES - 1) / KWAVES)), dim3(KT), 0, stream, a);
  hipLaunchKernelGGL(kitti_fold_kernel, dim3((9 * SAMPLES + KT - 1) / KT), dim3(KT), 0, stream, a);
  egn_count_launches(2);
  EGN_CHECK_HIP(hipGetLastError());
  std::vector<char> out(out_bytes);
  EGN_CHECK_HIP(hipMemcpyAsync(out.data(), dev + o_out, out_bytes, hipMemcpyDeviceToHost, stream));
  EGN_CHECK_HIP(hipStreamSynchronize(stream));

  memcpy(r.counts, out.data(), sizeof r.counts);
  const double* sim_sum = (const double*)(out.data() + (o_sim_sum - o_out));
  for (int combo = 0; combo < COMBOS; ++combo)
    if (active >> combo & 1u)
      egn_kitti::curves(r.counts + combo * SAMPLES * 3, sim_sum + (combo < 9 ? combo : 0) * SAMPLES, n_thr[combo],
                        combo < 9 && with_aos, r.precision + combo * SAMPLES,
                        combo < 9 ? r.aos + combo * SAMPLES : nullptr);
  return 0;
}

}  // namespace

extern "C" int egn_kitti_eval_dirs_dev(const char* gt_dir, const char* result_dir, int metrics, int* n_frames,
                                       int* evaluated, int* aos_valid, double* precision, double* aos, int* counts,
                                       int* n_thresholds, void* stream) {
  if (!gt_dir || !result_dir || !evaluated || !aos_valid || !precision || !aos || (metrics & ~7)) return EGN_E_BADARG;
  egn_kitti::Packed p;
  if (const int rc = egn_kitti::load_dirs(gt_dir, result_dir, p)) return rc;
  egn_kitti::Result r;
  if (const int rc = evaluate_device(p, metrics, (hipStream_t)stream, r)) return rc;
  egn_kitti::copy_out(r, n_frames, evaluated, aos_valid, precision, aos, counts, n_thresholds);
  return 0;
}

extern "C" int egn_kitti_eval_packed_dev(int n_frames, const int* gt_off, const int* det_off, const double* gt_box,
                                         const int* gt_type, const double* gt_trunc, const int* gt_occ,
                                         const double* det_box, const int* det_type, const double* det_score,
                                         int metrics, int* evaluated, int* aos_valid, double* precision, double* aos,
                                         int* counts, int* n_thresholds, void* stream) {
  if (!evaluated || !aos_valid || !precision || !aos || (metrics & ~7)) return EGN_E_BADARG;
  egn_kitti::Packed p;
  if (egn_kitti::from_arrays(n_frames, gt_off, det_off, gt_box, gt_type, gt_trunc, gt_occ, det_box, det_type,
                             det_score, p))
    return EGN_E_BADARG;
  egn_kitti::Result r;
  if (const int rc = evaluate_device(p, metrics, (hipStream_t)stream, r)) return rc;
  egn_kitti::copy_out(r, nullptr, evaluated, aos_valid, precision, aos, counts, n_thresholds);
  return 0;
}

extern "C" int egn_kitti_overlap_dev_f64(const double* det_box, const double* gt_box, long n, int criterion,
                                         double* out, void* stream) {
  if (n < 0 || n > 0x7fffffffL || criterion < -1 || criterion > 1 || (n > 0 && (!det_box || !gt_box || !out)))
    return EGN_E_BADARG;
  if (n == 0) return 0;
  hipLaunchKernelGGL(kitti_overlap_pairs_kernel, dim3((unsigned)((n + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, det_box, gt_box, n, criterion, out);
  egn_count_launches(1);
  return (int)hipGetLastError();
}
