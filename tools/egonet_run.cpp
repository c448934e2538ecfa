// egonet_run -- run an inference plan without Python: the C ABI of include/egonet_hip.h and the HIP runtime, nothing else.
//
//   egonet_run <plan.egnplan> <case file> <output directory> [repeats]
//
// The case file (little-endian) is what tools/export_plan.py --case writes:
//   "EGNCASE\0"  u32 n, C, H, W, has_K, alpha_mode  f64 fx, cx  f32 crops[n*C*H*W]  f64 centers[n*2]  f64 scales[n*2]
// The outputs of egn_plan_infer are written as raw arrays: local.f32 [n,J,2], kpts_2d.f64 [n,2J], kpts_3d.f64 [n,D] and,
// for the 96-output lifter, euler.f64 [n,3] and alpha.f64 [n].  Exit code 0: done; 1: usage / file trouble; 2: the
// library refused (its message is printed).  Built by egonet_amd/build.py (build_run) into tools/_build/.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "egonet_hip.h"

static bool read_all(const char* path, std::vector<uint8_t>* out) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  fseek(fp, 0, SEEK_END);
  const long size = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  if (size < 0) { fclose(fp); return false; }
  out->resize((size_t)size);
  const bool ok = fread(out->data(), 1, (size_t)size, fp) == (size_t)size;
  fclose(fp);
  return ok;
}

static bool write_all(const std::string& path, const void* p, size_t n) {
  FILE* fp = fopen(path.c_str(), "wb");
  if (!fp) return false;
  const bool ok = fwrite(p, 1, n, fp) == n;
  return fclose(fp) == 0 && ok;
}

#define HIP_OK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      fprintf(stderr, "egonet_run: %s: %s\n", #expr, hipGetErrorString(e_));            \
      return 2;                                                                         \
    }                                                                                   \
  } while (0)
#define EGN_OK(expr)                                                                    \
  do {                                                                                  \
    int c_ = (expr);                                                                    \
    if (c_ != 0) {                                                                      \
      fprintf(stderr, "egonet_run: %s: %s (code %d)\n", #expr, egn_strerror(c_), c_);   \
      return 2;                                                                         \
    }                                                                                   \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: egonet_run <plan.egnplan> <case file> <output directory> [repeats]\n");
    return 1;
  }
  const int repeats = argc > 4 ? atoi(argv[4]) : 1;
  std::vector<uint8_t> cs;
  if (!read_all(argv[2], &cs) || cs.size() < 48 || memcmp(cs.data(), "EGNCASE\0", 8)) {
    fprintf(stderr, "egonet_run: %s is not a case file\n", argv[2]);
    return 1;
  }
  uint32_t hd[6];
  double fxcx[2];
  memcpy(hd, cs.data() + 8, 24);
  memcpy(fxcx, cs.data() + 32, 16);
  const uint64_t n = hd[0], C = hd[1], H = hd[2], W = hd[3];
  if (n < 1 || n > 65535 || C < 1 || C > 4096 || H < 1 || H > 65536 || W < 1 || W > 65536 ||
      cs.size() != 48 + n * C * H * W * 4 + n * 4 * 8) {
    fprintf(stderr, "egonet_run: %s: sizes do not match the file length\n", argv[2]);
    return 1;
  }
  egn_plan* plan = nullptr;
  EGN_OK(egn_plan_open(argv[1], &plan));
  egn_plan_info info;
  EGN_OK(egn_plan_get_info(plan, &info));
  if ((uint64_t)info.C != C || (uint64_t)info.H != H || (uint64_t)info.W != W) {
    fprintf(stderr, "egonet_run: the plan takes [%d,%d,%d] crops, the case has [%d,%d,%d]\n", info.C, info.H, info.W, (int)C,
            (int)H, (int)W);
    return 1;
  }
  EGN_OK(egn_plan_load(plan, 0));
  const size_t crop_bytes = n * C * H * W * 4, J = (size_t)info.J, D = (size_t)info.lifter_out;
  const bool pose = D == 96;
  float *crops = nullptr, *local = nullptr;
  double *centers = nullptr, *scales = nullptr, *k2d = nullptr, *k3d = nullptr, *euler = nullptr, *alpha = nullptr;
  HIP_OK(hipMalloc(&crops, crop_bytes));
  HIP_OK(hipMalloc(&centers, n * 16));
  HIP_OK(hipMalloc(&scales, n * 16));
  HIP_OK(hipMalloc(&local, n * J * 8));
  HIP_OK(hipMalloc(&k2d, n * J * 16));
  HIP_OK(hipMalloc(&k3d, n * D * 8));
  HIP_OK(hipMalloc(&euler, n * 24));
  HIP_OK(hipMalloc(&alpha, n * 8));
  HIP_OK(hipMemcpy(crops, cs.data() + 48, crop_bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(centers, cs.data() + 48 + crop_bytes, n * 16, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(scales, cs.data() + 48 + crop_bytes + n * 16, n * 16, hipMemcpyHostToDevice));
  hipStream_t stream;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  const egn_plan_outputs outs = {local, k2d, k3d, euler, alpha};
  for (int k = 0; k < (repeats > 0 ? repeats : 1); ++k)
    EGN_OK(egn_plan_infer(plan, crops, (int)n, centers, scales, (int)hd[4], fxcx[0], fxcx[1], (int)hd[5], &outs, stream));
  HIP_OK(hipStreamSynchronize(stream));
  const std::string dir = std::string(argv[3]) + "/";
  struct Out { const char* name; const void* dev; size_t bytes; };
  const Out list[] = {{"local.f32", local, n * J * 8}, {"kpts_2d.f64", k2d, n * J * 16}, {"kpts_3d.f64", k3d, n * D * 8},
                      {"euler.f64", euler, pose ? n * 24 : 0}, {"alpha.f64", alpha, pose ? n * 8 : 0}};
  for (const Out& o : list) {
    if (!o.bytes) continue;
    std::vector<uint8_t> host(o.bytes);
    HIP_OK(hipMemcpy(host.data(), o.dev, o.bytes, hipMemcpyDeviceToHost));
    if (!write_all(dir + o.name, host.data(), o.bytes)) {
      fprintf(stderr, "egonet_run: cannot write %s%s\n", dir.c_str(), o.name);
      return 1;
    }
  }
  printf("egonet_run: %d crops, %ld program launches\n", (int)n, egn_launch_count());
  egn_plan_close(plan);
  (void)hipStreamDestroy(stream);
  for (void* p : {(void*)crops, (void*)centers, (void*)scales, (void*)local, (void*)k2d, (void*)k3d, (void*)euler, (void*)alpha})
    (void)hipFree(p);
  return 0;
}
