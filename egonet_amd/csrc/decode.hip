// decode.hip -- key-point decode from NCHW heat-maps, one 64-lane wavefront per
// (n,k) map.  HBM-bound: every map element is read ONCE.  The per-map body (hard arg-max, soft-arg-max, the
// numpy-style soft-arg-max) is egn_decode_map in decode_map.h, which kpt_metrics.hip runs too.
#include "egn_internal.h"
#include "decode_map.h"

__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ hm, int nmaps, int H, int W,
                                                     int mode, float* __restrict__ out_xy,
                                                     float* __restrict__ out_max, int32_t* __restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int map = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (map >= nmaps) return;
  float ox, oy, best;
  int bidx;
  egn_decode_map(hm + (size_t)map * (H * W), H, W, mode, lane, ox, oy, best, bidx);
  if (lane == 0) {
    out_xy[2 * (size_t)map] = ox;
    out_xy[2 * (size_t)map + 1] = oy;
    out_max[map] = best;
    if (out_idx) out_idx[map] = bidx;
  }
}

extern "C" int egn_decode_heatmaps_f32(const float* hm, int N, int K, int H, int W, int mode,
                                       float* out_xy, float* out_max, int32_t* out_idx, void* stream) {
  if (N < 0 || K <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2) return EGN_E_BADARG;
  const int nmaps = N * K;
  if (nmaps == 0) return 0;
  const int waves_per_block = 4;
  const int grid = (nmaps + waves_per_block - 1) / waves_per_block;
  hipLaunchKernelGGL(decode_kernel, dim3(grid), dim3(64 * waves_per_block), 0, (hipStream_t)stream,
                     hm, nmaps, H, W, mode, out_xy, out_max, out_idx);
  return (int)hipGetLastError();
}
