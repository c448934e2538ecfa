// pnp_refine.hip -- batched reprojection refinement of lifted cuboids (pnp_math.h) on the device, and its host twin.
//
// One wave64 per instance, four instances per 256-thread block.  Lane i owns correspondence i (J <= 64; lanes >= J
// add zeros).  The 21 + 6 sums of J^T J and J^T r and the cost are totalled by an xor butterfly in a fixed order;
// a + b and b + a are the same double, so after each stage both partners hold the same bits and at the end every
// lane holds the same totals.  Every lane then solves the 6x6 system redundantly: the control flow of a wave is
// uniform, there is no LDS, no atomic and no block barrier, and equal inputs give equal bits from run to run.
#include "egn_internal.h"
#include "pnp_math.h"

constexpr int PNP_WAVES = 4;

struct pnp_wave {
  int lane;
  __host__ __device__ int first() const { return lane; }
  __host__ __device__ int stride() const { return 64; }
  __host__ __device__ bool leader() const { return lane == 0; }
  template <int N>
  __host__ __device__ void sum(double (&v)[N]) const {
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
      for (int t = 0; t < N; ++t) v[t] += __shfl_xor(v[t], m, 64);
#endif
  }
};

static __host__ __device__ inline egn_pnp_in pnp_instance(const double* shape, const double* kpts2d,
                                                          const double* intr, const double* weights,
                                                          const double* root0, int J, double max_shift, size_t i) {
  egn_pnp_in in;
  in.S = shape + i * 3 * (size_t)(J - 1);
  in.k = kpts2d + i * 2 * (size_t)J;
  in.w = weights ? weights + i * (size_t)J : nullptr;
  in.T0 = root0 ? root0 + i * 3 : nullptr;
  in.fx = intr[4 * i];
  in.fy = intr[4 * i + 1];
  in.cx = intr[4 * i + 2];
  in.cy = intr[4 * i + 3];
  in.max_shift = max_shift;
  in.J = J;
  return in;
}

__global__ __launch_bounds__(64 * PNP_WAVES) void pnp_refine_kernel(
    const double* __restrict__ shape, const double* __restrict__ kpts2d, const double* __restrict__ intr,
    const double* __restrict__ weights, const double* __restrict__ root0, int n, int J, double max_shift,
    double* __restrict__ refined, double* __restrict__ rt, double* __restrict__ cost, int* __restrict__ iters,
    int* __restrict__ status, double* __restrict__ dims) {
  const int inst = blockIdx.x * PNP_WAVES + (threadIdx.x >> 6);   // uniform over the wave
  if (inst >= n) return;
  const size_t i = (size_t)inst;
  pnp_wave par;
  par.lane = threadIdx.x & 63;
  const egn_pnp_in in = pnp_instance(shape, kpts2d, intr, weights, root0, J, max_shift, i);
  egn_pnp_refine_one(par, in, refined + i * 3 * (size_t)J, rt + i * 12, cost + i * 2, iters + i, status + i,
                     dims + i * 3);
}

static int pnp_check(const double* shape, const double* kpts2d, const double* intr, int n, int J, double max_shift,
                     const double* refined, const double* rt, const double* cost, const int* iters,
                     const int* status, const double* dims) {
  if (n < 0 || J < 2 || J > 64 || !(max_shift >= 0.0)) return EGN_E_BADARG;
  if (n > 0 && (!shape || !kpts2d || !intr || !refined || !rt || !cost || !iters || !status || !dims))
    return EGN_E_BADARG;
  return 0;
}

extern "C" int egn_pnp_refine_f64(const double* shape, const double* kpts2d, const double* intr,
                                  const double* weights, const double* root0, int n, int J, double max_shift,
                                  double* refined, double* rt, double* cost, int* iters, int* status, double* dims,
                                  void* stream) {
  const int bad = pnp_check(shape, kpts2d, intr, n, J, max_shift, refined, rt, cost, iters, status, dims);
  if (bad) return bad;
  if (n == 0) return 0;
  const int blocks = (int)(((long)n + PNP_WAVES - 1) / PNP_WAVES);
  hipLaunchKernelGGL(pnp_refine_kernel, dim3(blocks), dim3(64 * PNP_WAVES), 0, (hipStream_t)stream, shape, kpts2d,
                     intr, weights, root0, n, J, max_shift, refined, rt, cost, iters, status, dims);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

// Host twin: the same pnp_math.h as a plain loop over HOST pointers (EgoNet.refine_pnp on numpy inputs or a CPU
// model).  Not a fallback of the device path: CUDA tensors never come here.
extern "C" int egn_pnp_refine_host_f64(const double* shape, const double* kpts2d, const double* intr,
                                       const double* weights, const double* root0, int n, int J, double max_shift,
                                       double* refined, double* rt, double* cost, int* iters, int* status,
                                       double* dims) {
  const int bad = pnp_check(shape, kpts2d, intr, n, J, max_shift, refined, rt, cost, iters, status, dims);
  if (bad) return bad;
  const egn_pnp_serial par;
  for (int idx = 0; idx < n; ++idx) {
    const size_t i = (size_t)idx;
    const egn_pnp_in in = pnp_instance(shape, kpts2d, intr, weights, root0, J, max_shift, i);
    egn_pnp_refine_one(par, in, refined + i * 3 * (size_t)J, rt + i * 12, cost + i * 2, iters + i, status + i,
                       dims + i * 3);
  }
  return 0;
}
