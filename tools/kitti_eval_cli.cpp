// kitti_eval_cli -- the KITTI object evaluator as a stand-alone host program, with the reference binary's command
// line (tools/kitti-eval/evaluate_object_3d_offline.cpp: main :917-947):
//
//     kitti_eval_cli gt_dir result_dir
//
// reads gt_dir/%06d.txt and result_dir/data/%06d.txt, prints one "<class>_<curve> AP: easy moderate hard" line per
// scored class and metric (car: detection, orientation, detection_ground, detection_3d -- the nine AP numbers and
// AOS) and writes result_dir/stats_<class>_detection[_ground|_3d].txt and stats_<class>_orientation.txt in the
// format of saveStats (:204-219): one line of 41 "%f " values per difficulty level.  No plots.
//
// Links csrc/kitti_eval.cpp only (python -m egonet_amd.build puts it in tools/_build/); no GPU, no HIP runtime.  It is
// also the program to run under -fsanitize=address,undefined.
#include <stdio.h>

#include <string>

#include "../include/egonet_hip.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "Usage: %s gt_dir result_dir\n", argv[0]);
    return 1;
  }
  static const char* const kClass[3] = {"car", "pedestrian", "cyclist"};
  static const char* const kSuffix[3] = {"detection", "detection_ground", "detection_3d"};
  static double precision[3 * 3 * 3 * 41], aos[3 * 3 * 41];
  int evaluated[9], aos_valid = 0, n_frames = 0;
  const int rc = egn_kitti_eval_dirs_host(argv[1], argv[2], 7, &n_frames, evaluated, &aos_valid, precision, aos,
                                          nullptr, nullptr);
  if (rc != 0) {
    fprintf(stderr, "%s\n", rc == -2   ? "a result file has no ground-truth file"
                            : rc == -3 ? "no result files under result_dir/data"
                                       : "bad argument");
    return 2;
  }
  printf("number of files for evaluation: %d\n", n_frames);
  const std::string dir = argv[2];
  auto report = [&](const std::string& name, const double* curve) {     // curve [3 levels][41]
    if (FILE* f = fopen((dir + "/stats_" + name + ".txt").c_str(), "w")) {
      for (int l = 0; l < 3; ++l) {
        for (int i = 0; i < 41; ++i) fprintf(f, "%f ", curve[l * 41 + i]);
        fprintf(f, "\n");
      }
      fclose(f);
    } else {
      fprintf(stderr, "cannot write %s/stats_%s.txt\n", dir.c_str(), name.c_str());
    }
    float sum[3] = {0, 0, 0};                                          // the reference sums in float (:719-723)
    for (int l = 0; l < 3; ++l)
      for (int i = 0; i < 41; i += 4) sum[l] += curve[l * 41 + i];
    printf("%s AP: %f %f %f\n", name.c_str(), sum[0] / 11 * 100, sum[1] / 11 * 100, sum[2] / 11 * 100);
  };
  for (int m = 0; m < 3; ++m)
    for (int c = 0; c < 3; ++c) {
      if (!evaluated[m * 3 + c]) continue;
      report(std::string(kClass[c]) + "_" + kSuffix[m], precision + (m * 3 + c) * 3 * 41);
      if (m == 0 && aos_valid) report(std::string(kClass[c]) + "_orientation", aos + c * 3 * 41);
    }
  return 0;
}
