// kitti_eval.cpp -- the KITTI object evaluator on the host: 2D AP and Average Orientation Similarity (IMAGE),
// bird's-eye-view AP (GROUND) and 3D AP (BOX3D), all three blocks of the reference's offline evaluator, without Boost
// (SURVEY section 8f rank 4).  Host code: it runs without a GPU and is also what tools/kitti_eval_cli.cpp links; the
// device path (kitti_eval.hip) shares the parsing, the thresholds and the curves defined here.
//
// Reference: tools/kitti-eval/evaluate_object_3d_offline.cpp
//   loadDetections :131-176, loadGroundtruth :178-202, imageBoxOverlap :227-265, toPolygon / groundBoxOverlap /
//   box3DOverlap :268-344 (kitti_overlap_math.h: the one Boost operation, the intersection of two rotated rectangles,
//   is a four-side clip), getThresholds :346-379, cleanData :381-454, computeStatistics :456-615 (kitti_eval_core.h),
//   eval_class :622-706, 11-point summary in saveAndPlotPlots :720-724, eval :795-915.
// The reference file cannot be compiled here (Boost headers absent): PARITY UNPINNED against the reference binary.
// What pins this file instead: an independent Python restatement (oracle/kitti_eval_oracle.py for IMAGE,
// tests/kitti_eval3d_ref.py for GROUND / BOX3D, whose overlaps come from scipy's half-plane intersection), closed-form
// overlaps and hand-computed cases.
//
// Where the reference recomputes an overlap inside the matching loops (recall pass + up to 41 threshold passes, times
// 3 levels, per metric), the overlaps of all (detection, ground truth) pairs of a frame are computed once here.
//
// Semantics kept on purpose: the class-overlap table as overwritten in the reference (0.7 / 0.5 / 0.5 for car /
// pedestrian / cyclist in every metric, :55), difficulty by the 2D box height in every metric, detection heights
// truncated to int (:444), "Van" / "Person_sitting" neighbours ignored, DontCare areas absorb unassigned detections by
// the metric's own overlap over the detection (:582), AOS only for IMAGE (:877), a class scored in GROUND / BOX3D only
// when one of its detections has t1 / t2 != -1000 (:164-167), recall sampled at 41 points with the left/right-closest
// rule, precision and AOS made monotone from the right.
#include <dirent.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/egonet_hip.h"
#include "kitti_eval_core.h"

namespace egn_kitti {

namespace {

constexpr int kSamples = EGN_KITTI_SAMPLES;

bool read_lines(const std::string& path, std::vector<std::vector<std::string>>& rows) {
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return false;
  char buf[1024];
  while (fgets(buf, sizeof buf, f)) {
    std::vector<std::string> tok;
    for (char* p = strtok(buf, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) tok.push_back(p);
    if (!tok.empty()) rows.push_back(tok);
  }
  fclose(f);
  return true;
}

// fields 3 (alpha), 4-7 (2D box), 8-14 (h w l t1 t2 t3 ry) of a row -> EGN_KITTI_BOX doubles
void push_box(const std::vector<std::string>& r, std::vector<double>& out) {
  for (int k = 4; k < 8; ++k) out.push_back(atof(r[k].c_str()));
  out.push_back(atof(r[3].c_str()));
  for (int k = 8; k < 15; ++k) out.push_back(atof(r[k].c_str()));
}

}  // namespace

int type_code(const char* name) {
  static const char* const kNames[] = {"car", "pedestrian", "cyclist", "van", "person_sitting", "dontcare"};
  for (int k = 0; k < 6; ++k)
    if (strcasecmp(name, kNames[k]) == 0) return k;
  return EGN_KT_OTHER;
}

void Packed::end_frame() {
  const long long ng = (long long)gt_type.size() - gt_off.back(), nd = (long long)det_type.size() - det_off.back();
  gt_off.push_back((int)gt_type.size());
  det_off.push_back((int)det_type.size());
  pair_off.push_back(pair_off.back() + ng * nd);
  word_off.push_back(word_off.back() + (int)((nd + 31) / 32));
}

EgnKittiView Packed::view(const double* ov, const double* sim) const {
  EgnKittiView v;
  v.nf = nf();
  v.gt_off = gt_off.data();
  v.det_off = det_off.data();
  v.pair_off = pair_off.data();
  v.word_off = word_off.data();
  v.gt_box = gt_box.data();
  v.gt_trunc = gt_trunc.data();
  v.gt_type = gt_type.data();
  v.gt_occ = gt_occ.data();
  v.det_box = det_box.data();
  v.det_score = det_score.data();
  v.det_type = det_type.data();
  v.ov = ov;
  v.sim = sim;
  v.pairs = pair_off.back();
  return v;
}

int load_dirs(const char* gt_dir, const char* result_dir, Packed& p) {
  const std::string data_dir = std::string(result_dir) + "/data/";
  std::vector<int> ids;
  if (DIR* d = opendir(data_dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string name = e->d_name;
      if (name.size() < 10) continue;
      ids.push_back(atoi(name.substr(name.size() - 10).c_str()));
    }
    closedir(d);
  }
  if (ids.empty()) return -3;
  std::sort(ids.begin(), ids.end());
  for (size_t f = 0; f < ids.size(); ++f) {
    char name[32];
    snprintf(name, sizeof name, "%06d.txt", ids[f]);
    std::vector<std::vector<std::string>> rows;
    if (!read_lines(std::string(gt_dir) + "/" + name, rows)) return -2;
    for (const auto& r : rows) {
      if (r.size() < 15) continue;
      push_box(r, p.gt_box);
      p.gt_type.push_back(type_code(r[0].c_str()));
      p.gt_trunc.push_back(atof(r[1].c_str()));
      p.gt_occ.push_back(atoi(r[2].c_str()));
    }
    rows.clear();
    if (!read_lines(data_dir + name, rows)) return -3;
    for (const auto& r : rows) {
      if (r.size() < 16) continue;
      push_box(r, p.det_box);
      p.det_type.push_back(type_code(r[0].c_str()));
      p.det_score.push_back(atof(r[15].c_str()));
    }
    if (p.gt_type.size() > 0x7ffffff || p.det_type.size() > 0x7ffffff) return -1;
    p.end_frame();
  }
  return 0;
}

int from_arrays(int nf, const int* gt_off, const int* det_off, const double* gt_box, const int* gt_type,
                const double* gt_trunc, const int* gt_occ, const double* det_box, const int* det_type,
                const double* det_score, Packed& p) {
  if (nf < 0 || !gt_off || !det_off || gt_off[0] != 0 || det_off[0] != 0) return -1;
  for (int f = 0; f < nf; ++f)
    if (gt_off[f + 1] < gt_off[f] || det_off[f + 1] < det_off[f]) return -1;
  const int ng = gt_off[nf], nd = det_off[nf];
  if (ng > 0x7ffffff || nd > 0x7ffffff) return -1;
  if (ng > 0 && (!gt_box || !gt_type || !gt_trunc || !gt_occ)) return -1;
  if (nd > 0 && (!det_box || !det_type || !det_score)) return -1;
  for (int i = 0; i < ng; ++i)
    if (gt_type[i] < 0 || gt_type[i] > EGN_KT_OTHER) return -1;
  for (int j = 0; j < nd; ++j)
    if (det_type[j] < 0 || det_type[j] > EGN_KT_OTHER) return -1;
  p.gt_box.assign(gt_box, gt_box + (size_t)ng * EGN_KITTI_BOX);
  p.gt_type.assign(gt_type, gt_type + ng);
  p.gt_trunc.assign(gt_trunc, gt_trunc + ng);
  p.gt_occ.assign(gt_occ, gt_occ + ng);
  p.det_box.assign(det_box, det_box + (size_t)nd * EGN_KITTI_BOX);
  p.det_type.assign(det_type, det_type + nd);
  p.det_score.assign(det_score, det_score + nd);
  for (int f = 0; f < nf; ++f) {
    const long long g = gt_off[f + 1] - gt_off[f], d = det_off[f + 1] - det_off[f];
    p.gt_off.push_back(gt_off[f + 1]);
    p.det_off.push_back(det_off[f + 1]);
    p.pair_off.push_back(p.pair_off.back() + g * d);
    p.word_off.push_back(p.word_off.back() + (int)((d + 31) / 32));
  }
  if (p.pair_off.back() > (1LL << 36)) return -1;
  return 0;
}

void scored(const Packed& p, int metrics, Result& r) {
  r.n_frames = p.nf();
  r.aos_valid = 1;
  for (int k = 0; k < 9; ++k) r.evaluated[k] = 0;
  for (size_t j = 0; j < p.det_type.size(); ++j) {
    const double* b = p.det_box.data() + j * EGN_KITTI_BOX;
    if (b[EGN_KB_ALPHA] == -10) r.aos_valid = 0;
    const int c = p.det_type[j];
    if (c > EGN_KT_CYCLIST) continue;
    if (b[EGN_KB_X1] >= 0) r.evaluated[c] = 1;
    if (b[EGN_KB_T1] != -1000) r.evaluated[3 + c] = 1;
    if (b[EGN_KB_T2] != -1000) r.evaluated[6 + c] = 1;
  }
  for (int m = 0; m < 3; ++m)
    if (!(metrics >> m & 1))
      for (int c = 0; c < 3; ++c) r.evaluated[m * 3 + c] = 0;
}

std::vector<double> similarity_table(const Packed& p) {
  std::vector<double> sim((size_t)p.pair_off.back(), 0.0);
  for (int f = 0; f < p.nf(); ++f) {
    const int g0 = p.gt_off[f], ng = p.gt_off[f + 1] - g0, d0 = p.det_off[f], nd = p.det_off[f + 1] - d0;
    double* s = sim.data() + p.pair_off[f];
    for (int i = 0; i < ng; ++i) {
      if (p.gt_type[g0 + i] > EGN_KT_CYCLIST) continue;          // only a pair of one class can be a true positive
      const double ag = p.gt_box[(size_t)(g0 + i) * EGN_KITTI_BOX + EGN_KB_ALPHA];
      for (int j = 0; j < nd; ++j)
        if (p.det_type[d0 + j] == p.gt_type[g0 + i])
          s[(size_t)i * nd + j] = (1.0 + cos(ag - p.det_box[(size_t)(d0 + j) * EGN_KITTI_BOX + EGN_KB_ALPHA])) / 2.0;
    }
  }
  return sim;
}

std::vector<double> recall_thresholds(std::vector<double> v, double n_gt) {
  std::sort(v.begin(), v.end(), [](double a, double b) { return a > b; });
  std::vector<double> t;
  double current = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    const double left = (double)(i + 1) / n_gt;
    const double right = i + 1 < v.size() ? (double)(i + 2) / n_gt : left;
    if ((right - current) < (current - left) && i + 1 < v.size()) continue;
    t.push_back(v[i]);
    current += 1.0 / (kSamples - 1.0);
  }
  return t;
}

void curves(const int* counts, const double* similarity, int n_thr, bool with_aos, double* precision, double* aos) {
  for (int i = 0; i < kSamples; ++i) {
    precision[i] = 0;
    if (aos) aos[i] = 0;
  }
  for (int i = 0; i < n_thr && i < kSamples; ++i) {
    const int tp = counts[3 * i], fp = counts[3 * i + 1];
    precision[i] = tp / (double)(tp + fp);
    if (with_aos) aos[i] = similarity[i] / (double)(tp + fp);
  }
  for (int i = 0; i < n_thr && i < kSamples; ++i) {   // monotone from the right, over all 41 samples
    precision[i] = *std::max_element(precision + i, precision + kSamples);
    if (with_aos) aos[i] = *std::max_element(aos + i, aos + kSamples);
  }
}

namespace {

// the three overlap tables of every frame, once
std::vector<double> overlap_tables(const Packed& p) {
  const size_t pairs = (size_t)p.pair_off.back();
  std::vector<double> ov(3 * pairs);
  for (int f = 0; f < p.nf(); ++f) {
    const int g0 = p.gt_off[f], ng = p.gt_off[f + 1] - g0, d0 = p.det_off[f], nd = p.det_off[f + 1] - d0;
    for (int i = 0; i < ng; ++i) {
      const double* g = p.gt_box.data() + (size_t)(g0 + i) * EGN_KITTI_BOX;
      const int criterion = p.gt_type[g0 + i] == EGN_KT_DONTCARE ? 0 : -1;
      for (int j = 0; j < nd; ++j) {
        double o[4];
        egn_kitti_overlaps(p.det_box.data() + (size_t)(d0 + j) * EGN_KITTI_BOX, g, criterion, o);
        const size_t at = (size_t)p.pair_off[f] + (size_t)i * nd + j;
        for (int m = 0; m < 3; ++m) ov[m * pairs + at] = o[m];
      }
    }
  }
  return ov;
}

// eval_class for one (metric, class, level)
void evaluate(const EgnKittiView& v, int metric, int cls, int level, bool with_aos, Result& r) {
  const int combo = (metric * 3 + cls) * 3 + level;
  int max_words = 1, max_gt = 1;
  for (int f = 0; f < v.nf; ++f) {
    max_words = std::max(max_words, v.word_off[f + 1] - v.word_off[f]);
    max_gt = std::max(max_gt, v.gt_off[f + 1] - v.gt_off[f]);
  }
  std::vector<unsigned> taken(max_words);
  std::vector<double> frame_scores(max_gt), scores;
  EgnKittiCounts c;
  int n_gt = 0;
  for (int f = 0; f < v.nf; ++f) {
    egn_kitti_match<false>(v, f, cls, level, metric, false, 0.0, taken.data(), 1, frame_scores.data(), c);
    n_gt += c.n_gt;
    scores.insert(scores.end(), frame_scores.begin(), frame_scores.begin() + c.tp);
  }
  std::vector<double> thr = recall_thresholds(scores, n_gt);
  if (thr.size() > (size_t)kSamples) thr.resize(kSamples);
  const int nt = (int)thr.size();
  int* counts = r.counts + combo * kSamples * 3;
  double similarity[kSamples] = {0};
  for (int f = 0; f < v.nf; ++f)
    for (int t = 0; t < nt; ++t) {
      egn_kitti_match<true>(v, f, cls, level, metric, with_aos, thr[t], taken.data(), 1, nullptr, c);
      counts[3 * t] += c.tp;
      counts[3 * t + 1] += c.fp;
      counts[3 * t + 2] += c.fn;
      if (c.similarity != -1) similarity[t] += c.similarity;
    }
  r.n_thresholds[combo] = nt;
  r.n_gt[combo] = n_gt;
  curves(counts, similarity, nt, with_aos, r.precision + combo * kSamples,
         metric == 0 ? r.aos + (cls * 3 + level) * kSamples : nullptr);
}

}  // namespace

void evaluate_host(const Packed& p, int metrics, Result& r) {
  scored(p, metrics, r);
  const std::vector<double> ov = overlap_tables(p);
  const bool with_aos = r.aos_valid && (r.evaluated[0] || r.evaluated[1] || r.evaluated[2]);
  std::vector<double> sim;
  if (with_aos) sim = similarity_table(p);
  const EgnKittiView v = p.view(ov.data(), with_aos ? sim.data() : nullptr);
  for (int m = 0; m < 3; ++m)
    for (int c = 0; c < 3; ++c)
      for (int l = 0; l < 3; ++l)
        if (r.evaluated[m * 3 + c]) evaluate(v, m, c, l, m == 0 && with_aos, r);
}

void copy_out(const Result& r, int* n_frames, int* evaluated, int* aos_valid, double* precision, double* aos,
              int* counts, int* n_thresholds) {
  if (n_frames) *n_frames = r.n_frames;
  *aos_valid = r.aos_valid;
  memcpy(evaluated, r.evaluated, sizeof r.evaluated);
  memcpy(precision, r.precision, sizeof r.precision);
  memcpy(aos, r.aos, sizeof r.aos);
  if (counts) memcpy(counts, r.counts, sizeof r.counts);
  if (n_thresholds) memcpy(n_thresholds, r.n_thresholds, sizeof r.n_thresholds);
}

}  // namespace egn_kitti

// precision / aos: [3 classes][3 difficulty levels][41 recall samples] doubles.
// evaluated[c] = 1 when class c has at least one detection (with x1 >= 0);
// *aos_valid = 0 when any detection carries alpha == -10 (AOS rows stay 0).
// Returns 0, or -1 (bad argument), -2 (a result file has no ground-truth file),
// -3 (result_dir/data cannot be read or is empty).
extern "C" int egn_kitti_eval_image(const char* gt_dir, const char* result_dir, int* n_frames, int* evaluated,
                                    int* aos_valid, double* precision, double* aos) {
  if (!gt_dir || !result_dir || !evaluated || !aos_valid || !precision || !aos) return -1;
  egn_kitti::Packed p;
  if (const int rc = egn_kitti::load_dirs(gt_dir, result_dir, p)) return rc;
  egn_kitti::Result r;
  egn_kitti::evaluate_host(p, 1, r);
  if (n_frames) *n_frames = r.n_frames;
  *aos_valid = r.aos_valid;
  for (int c = 0; c < 3; ++c) evaluated[c] = r.evaluated[c];
  memcpy(precision, r.precision, sizeof(double) * 9 * EGN_KITTI_SAMPLES);
  memcpy(aos, r.aos, sizeof(double) * 9 * EGN_KITTI_SAMPLES);
  return 0;
}

extern "C" int egn_kitti_eval_dirs_host(const char* gt_dir, const char* result_dir, int metrics, int* n_frames,
                                        int* evaluated, int* aos_valid, double* precision, double* aos, int* counts,
                                        int* n_thresholds) {
  if (!gt_dir || !result_dir || !evaluated || !aos_valid || !precision || !aos || (metrics & ~7)) return -1;
  egn_kitti::Packed p;
  if (const int rc = egn_kitti::load_dirs(gt_dir, result_dir, p)) return rc;
  egn_kitti::Result r;
  egn_kitti::evaluate_host(p, metrics, r);
  egn_kitti::copy_out(r, n_frames, evaluated, aos_valid, precision, aos, counts, n_thresholds);
  return 0;
}

extern "C" int egn_kitti_eval_packed_host(int n_frames, const int* gt_off, const int* det_off, const double* gt_box,
                                          const int* gt_type, const double* gt_trunc, const int* gt_occ,
                                          const double* det_box, const int* det_type, const double* det_score,
                                          int metrics, int* evaluated, int* aos_valid, double* precision, double* aos,
                                          int* counts, int* n_thresholds) {
  if (!evaluated || !aos_valid || !precision || !aos || (metrics & ~7)) return -1;
  egn_kitti::Packed p;
  if (egn_kitti::from_arrays(n_frames, gt_off, det_off, gt_box, gt_type, gt_trunc, gt_occ, det_box, det_type,
                             det_score, p))
    return -1;
  egn_kitti::Result r;
  egn_kitti::evaluate_host(p, metrics, r);
  egn_kitti::copy_out(r, nullptr, evaluated, aos_valid, precision, aos, counts, n_thresholds);
  return 0;
}

extern "C" int egn_kitti_overlap_host_f64(const double* det_box, const double* gt_box, long n, int criterion,
                                          double* out) {
  if (n < 0 || criterion < -1 || criterion > 1 || (n > 0 && (!det_box || !gt_box || !out))) return -1;
  for (long k = 0; k < n; ++k)
    egn_kitti_overlaps(det_box + k * EGN_KITTI_BOX, gt_box + k * EGN_KITTI_BOX, criterion, out + 4 * k);
  return 0;
}
