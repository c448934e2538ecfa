// kitti_eval_core.h -- what the host evaluator (kitti_eval.cpp) and the device evaluator (kitti_eval.hip) share: the
// packed frame set, cleanData (:381-454) and computeStatistics (:456-615) of the reference's
// tools/kitti-eval/evaluate_object_3d_offline.cpp as one host/device function over a per-frame overlap table, and the
// declarations of the host-only parts (parsing, getThresholds, the curves of eval_class).
//
// Index conventions: metric 0 IMAGE, 1 GROUND, 2 BOX3D; class 0 car, 1 pedestrian, 2 cyclist; level 0 easy,
// 1 moderate, 2 hard; a "combination" is (metric * 3 + class) * 3 + level, 27 of them.
#pragma once
#include "kitti_overlap_math.h"

#define EGN_KITTI_COMBOS 27
#define EGN_KITTI_SAMPLES 41
// type codes of a label / result row (compared case-insensitively when packed)
#define EGN_KT_CAR 0
#define EGN_KT_PEDESTRIAN 1
#define EGN_KT_CYCLIST 2
#define EGN_KT_VAN 3
#define EGN_KT_PERSON_SITTING 4
#define EGN_KT_DONTCARE 5
#define EGN_KT_OTHER 6

// All frames as flat arrays.  Frame f owns ground truths gt_off[f] .. gt_off[f + 1], detections det_off[f] ..
// det_off[f + 1], overlap-table entries pair_off[f] .. pair_off[f + 1] (ground-truth major: i * nd + j) and
// word_off[f] .. word_off[f + 1] 32-bit words of an assigned-detection set.
struct EgnKittiView {
  int nf;
  const int* gt_off;
  const int* det_off;
  const long long* pair_off;
  const int* word_off;
  const double* gt_box;      // [n_gt][EGN_KITTI_BOX]
  const double* gt_trunc;
  const int* gt_type;
  const int* gt_occ;
  const double* det_box;     // [n_det][EGN_KITTI_BOX]
  const double* det_score;
  const int* det_type;
  const double* ov;          // [3 metrics][pairs]: union overlap; over the detection where the row is a DontCare area
  const double* sim;         // [pairs] (1 + cos(alpha_gt - alpha_det)) / 2, or NULL without AOS
  long long pairs;
};

struct EgnKittiCounts {
  int tp, fp, fn, n_gt;
  double similarity;
};

EGN_HD inline int egn_kitti_min_height(int level) { return level == 0 ? 40 : 25; }
EGN_HD inline double egn_kitti_max_truncation(int level) { return level == 0 ? 0.15 : (level == 1 ? 0.3 : 0.5); }
// MIN_OVERLAP as the reference overwrote it (:55): the same row for all three metrics
EGN_HD inline double egn_kitti_min_overlap(int cls) { return cls == 0 ? 0.7 : 0.5; }

// cleanData.  Ground truth: 0 counted, 1 ignored (neighbour class / too hard), -1 other class.  The difficulty
// filters use the 2D box height in every metric (:387, :444).
EGN_HD inline int egn_kitti_gt_flag(int cls, int level, int type, double trunc, int occ, const double* box) {
  int valid = -1;
  if (type == cls) valid = 1;
  else if (cls == EGN_KT_PEDESTRIAN && type == EGN_KT_PERSON_SITTING) valid = 0;
  else if (cls == EGN_KT_CAR && type == EGN_KT_VAN) valid = 0;
  const bool hard = occ > level || trunc > egn_kitti_max_truncation(level) ||
                    (box[EGN_KB_Y2] - box[EGN_KB_Y1]) < egn_kitti_min_height(level);
  if (valid == 1 && !hard) return 0;
  if (valid == 0 || (hard && valid == 1)) return 1;
  return -1;
}

// Detection: 0 evaluated, 1 too small, -1 other class.  The height is truncated to an integer, as the reference does.
EGN_HD inline int egn_kitti_det_flag(int cls, int level, int type, const double* box) {
  const int height = (int)fabs(box[EGN_KB_Y1] - box[EGN_KB_Y2]);
  if (height < egn_kitti_min_height(level)) return 1;
  return type == cls ? 0 : -1;
}

// computeStatistics for frame f.  FP = false is the recall pass (the most confident candidate wins; tp_scores
// receives the score of every true positive, at most min(n_gt, n_det) of them); FP = true the precision pass at
// score threshold thresh (the best-overlapping candidate wins, false positives and DontCare areas are counted).
// taken: the assigned-detection set, word k at taken[k * stride], word_off[f + 1] - word_off[f] words; cleared here.
template <bool FP>
EGN_HD inline void egn_kitti_match(const EgnKittiView& v, int f, int cls, int level, int metric, bool with_aos,
                                   double thresh, unsigned* taken, long stride, double* tp_scores,
                                   EgnKittiCounts& out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double kNone = -10000000;
  const int g0 = v.gt_off[f], ng = v.gt_off[f + 1] - g0;
  const int d0 = v.det_off[f], nd = v.det_off[f + 1] - d0;
  const int nw = v.word_off[f + 1] - v.word_off[f];
  const double* ov = v.ov + (long long)metric * v.pairs + v.pair_off[f];
  const double* sim = v.sim ? v.sim + v.pair_off[f] : nullptr;
  const double min_ov = egn_kitti_min_overlap(cls);
  for (int k = 0; k < nw; ++k) taken[k * stride] = 0u;
  out.tp = out.fp = out.fn = out.n_gt = 0;
  double s = 0.0;
  unsigned cur = 0u;
  for (int i = 0; i < ng; ++i) {
    const int gflag = egn_kitti_gt_flag(cls, level, v.gt_type[g0 + i], v.gt_trunc[g0 + i], v.gt_occ[g0 + i],
                                        v.gt_box + (long long)(g0 + i) * EGN_KITTI_BOX);
    if (gflag == -1) continue;
    if (gflag == 0) ++out.n_gt;
    int pick = -1, pick_flag = 0;
    double valid = kNone, best = 0;
    bool picked_small = false;
    for (int j = 0; j < nd; ++j) {
      if ((j & 31) == 0) cur = taken[(j >> 5) * stride];
      const int dflag = egn_kitti_det_flag(cls, level, v.det_type[d0 + j], v.det_box + (long long)(d0 + j) * EGN_KITTI_BOX);
      if (dflag == -1 || ((cur >> (j & 31)) & 1u)) continue;
      const double score = v.det_score[d0 + j];
      if (FP && score < thresh) continue;
      const double o = ov[(long long)i * nd + j];
      if (!(o > min_ov)) continue;
      if (!FP) {                                         // recall pass: the most confident candidate
        if (score > valid) {
          pick = j;
          pick_flag = dflag;
          valid = score;
        }
      } else if ((o > best || picked_small) && dflag == 0) {   // pr pass: the best-overlapping one
        best = o;
        pick = j;
        pick_flag = dflag;
        valid = 1;
        picked_small = false;
      } else if (valid == kNone && dflag == 1) {
        pick = j;
        pick_flag = dflag;
        valid = 1;
        picked_small = true;
      }
    }
    if (valid == kNone) {
      if (gflag == 0) ++out.fn;
      continue;
    }
    taken[(pick >> 5) * stride] |= 1u << (pick & 31);   // matched; with one side ignored neither TP nor FP
    if (gflag == 1 || pick_flag == 1) continue;
    if (!FP) tp_scores[out.tp] = v.det_score[d0 + pick];
    if (FP && with_aos) s = s + sim[(long long)i * nd + pick];
    ++out.tp;
  }
  out.similarity = 0.0;
  if (!FP) return;
  for (int j = 0; j < nd; ++j) {
    if ((j & 31) == 0) cur = taken[(j >> 5) * stride];
    if (((cur >> (j & 31)) & 1u) || v.det_score[d0 + j] < thresh) continue;
    if (egn_kitti_det_flag(cls, level, v.det_type[d0 + j], v.det_box + (long long)(d0 + j) * EGN_KITTI_BOX) == 0) ++out.fp;
  }
  int stuff = 0;                                         // DontCare areas absorb what is left, by the metric's own
  for (int i = 0; i < ng; ++i) {                         // overlap over the detection (:582)
    if (v.gt_type[g0 + i] != EGN_KT_DONTCARE) continue;
    for (int j = 0; j < nd; ++j) {
      if ((j & 31) == 0) cur = taken[(j >> 5) * stride];
      if (((cur >> (j & 31)) & 1u) || v.det_score[d0 + j] < thresh) continue;
      if (egn_kitti_det_flag(cls, level, v.det_type[d0 + j], v.det_box + (long long)(d0 + j) * EGN_KITTI_BOX) != 0) continue;
      if (ov[(long long)i * nd + j] > min_ov) {
        cur |= 1u << (j & 31);
        taken[(j >> 5) * stride] = cur;
        ++stuff;
      }
    }
  }
  out.fp -= stuff;
  if (with_aos) out.similarity = (out.tp > 0 || out.fp > 0) ? s : -1.0;   // false positives contribute 0
}

#include <vector>

namespace egn_kitti {

// The frame set with its own storage.
struct Packed {
  std::vector<int> gt_off{0}, det_off{0}, word_off{0};
  std::vector<long long> pair_off{0};
  std::vector<double> gt_box, gt_trunc, det_box, det_score;
  std::vector<int> gt_type, gt_occ, det_type;
  int nf() const { return (int)gt_off.size() - 1; }
  void end_frame();                       // after the rows of a frame were appended
  EgnKittiView view(const double* ov, const double* sim) const;
};

struct Result {
  int n_frames = 0, aos_valid = 0;
  int evaluated[9] = {0};                                        // [metric][class]
  double precision[EGN_KITTI_COMBOS * EGN_KITTI_SAMPLES] = {0};  // [metric][class][level][41]
  double aos[9 * EGN_KITTI_SAMPLES] = {0};                       // [class][level][41], IMAGE only
  int counts[EGN_KITTI_COMBOS * EGN_KITTI_SAMPLES * 3] = {0};    // tp, fp, fn per recall step
  int n_thresholds[EGN_KITTI_COMBOS] = {0};
  int n_gt[EGN_KITTI_COMBOS] = {0};
};

int type_code(const char* name);
// 0, -2 (a result file has no ground-truth file), -3 (result_dir/data cannot be read or is empty)
int load_dirs(const char* gt_dir, const char* result_dir, Packed& p);
// 0 or -1: offsets that do not start at 0 or decrease, a type code outside the table, tables past 2^31 - 1
int from_arrays(int nf, const int* gt_off, const int* det_off, const double* gt_box, const int* gt_type,
                const double* gt_trunc, const int* gt_occ, const double* det_box, const int* det_type,
                const double* det_score, Packed& p);
// which (metric, class) are scored (:156-167) under the caller's metric mask (bit m = metric m), and AOS validity
void scored(const Packed& p, int metrics, Result& r);
// (1 + cos(alpha_gt - alpha_det)) / 2 for every pair of one class, 0 elsewhere: evaluated once, on the host for both
// paths, so that the device sums the same doubles as the host (the two cos() differ in the last place)
std::vector<double> similarity_table(const Packed& p);
std::vector<double> recall_thresholds(std::vector<double> v, double n_gt);            // getThresholds
void curves(const int* counts, const double* similarity, int n_thr, bool with_aos, double* precision, double* aos);
void evaluate_host(const Packed& p, int metrics, Result& r);
void copy_out(const Result& r, int* n_frames, int* evaluated, int* aos_valid, double* precision, double* aos,
              int* counts, int* n_thresholds);

}  // namespace egn_kitti
