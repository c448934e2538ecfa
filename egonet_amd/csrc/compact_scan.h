// compact_scan.h -- the one-block exclusive scan of per-block kept counts that the stream compactions of
// lifter_pairs.hip and pose_annot.hip run between their flag pass and their write pass.  The kernel has internal
// linkage: each including file launches its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// one block: counts -> exclusive offsets, total -> *total.  Thread t owns a contiguous chunk; the chunk sums are
// scanned by thread 0, so the result does not depend on scheduling.
__global__ __launch_bounds__(1024) void pairs_scan_kernel(int* counts, int n, long long* total) {
  __shared__ long long s_sum[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int b = min(t * per, n), e = min(b + per, n);
  long long sum = 0;
  for (int i = b; i < e; ++i) sum += counts[i];
  s_sum[t] = sum;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < 1024; ++i) {
      const long long v = s_sum[i];
      s_sum[i] = run;
      run += v;
    }
    *total = run;
  }
  __syncthreads();
  long long run = s_sum[t];
  for (int i = b; i < e; ++i) {
    const int v = counts[i];
    counts[i] = (int)run;
    run += v;
  }
}

}  // namespace
