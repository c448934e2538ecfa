// softargmax.hip -- the differentiable soft-arg-max of the heat-map head's integral terms (JointsCompositeLoss on a
// model that returns heat-maps only, libs/loss/function.py:187-201 with soft_arg_max, libs/common/img_proc.py:678-707):
// forward (coordinates of every map) and backward (d coords -> d maps through the softmax Jacobian) on the padded NHWC
// maps of the training tape.  The arithmetic and its order are defined in softargmax_math.h; the host twins below run
// the same text and give the same bits.
//
// Layout of the work.  The maps of one image interleave by channel, so a thread owns ONE channel and a slice of the
// pixels: thread t of a block = (slice j, channel) with the channel fastest and S = slices(cs) slices.  Neighbouring
// lanes read neighbouring floats of a pixel and the next lanes the next pixel: loads are coalesced (the backward's
// S * cs threads read S whole pixels = S * cs consecutive floats), no map is transposed, and nothing but plain vector
// loads / stores touches memory (no atomics).
//   forward : a block per (image, group of 12 channels): S slices x 12 threads, two passes over its maps (max, then the
//             three sums; the second pass hits L2), per-slice partials folded in LDS by the fixed tree of the header.
//             The exp makes the pass compute-bound on one CU per image; the channel groups spread an image over CUs at
//             the price of 48-byte pieces of each pixel per block (the other groups' blocks read the rest from L2).
//   backward: no reduction -- a block per (image, 128 pixels), 256 threads in the same (slice, channel) arrangement,
//             each computes its channel's six constants once and walks its pixels.
#include "egn_internal.h"
#include "softargmax_math.h"

constexpr int SAM_BWD_THREADS = 256;
constexpr int SAM_BWD_PIXELS = 128;     // pixels of a backward block
constexpr int SAM_BATCH = 8;            // loads a forward thread issues before it uses the first
constexpr int SAM_FWD_GROUP = 12;       // channels of a forward block (48 contiguous bytes of every pixel)

// pixel (x, y) of a thread walking p, p + S, p + 2S, ...: no division in the loops
struct sam_walk {
  int x, y, dx, dy, w;
  __device__ sam_walk(long p, int S, int w_) : x((int)(p % w_)), y((int)(p / w_)), dx(S % w_), dy(S / w_), w(w_) {}
  __device__ void next() {
    x += dx;
    y += dy;
    if (x >= w) {
      x -= w;
      ++y;
    }
  }
};

__global__ __launch_bounds__(EGN_SAM_THREADS) void softargmax_fwd_kernel(const float* __restrict__ z, int h, int w, int K,
                                                                         int cs, int cwg, float div_x, float div_y,
                                                                         float* __restrict__ coords,
                                                                         float* __restrict__ save) {
  __shared__ float s_a[EGN_SAM_THREADS], s_b[EGN_SAM_THREADS], s_c[EGN_SAM_THREADS];
  const int n = blockIdx.x, t = threadIdx.x;
  const int cw = egn_sam_chan_width(cs), S = egn_sam_slices(cs), top = egn_sam_tree_top(S);
  const int j = t / cwg, cl = t - j * cwg;        // blockDim.x = S * cwg: j < S
  const int cg = blockIdx.y * cwg + cl;           // this thread's channel within a chunk of cw
  const long hw = (long)h * w;
  const float* zn = z + (size_t)n * hw * cs;
  for (int cb = 0; cb < K; cb += cw) {
    const int c = cb + cg;
    const bool live = cg < cw && c < K;
    float m = -INFINITY;
    if (live) {
      // SAM_BATCH loads in flight per thread before the first use
      for (long p = j; p < hw; p += (long)S * SAM_BATCH) {
        float v[SAM_BATCH];
#pragma unroll
        for (int u = 0; u < SAM_BATCH; ++u) {
          const long q = p + (long)u * S;
          v[u] = q < hw ? zn[(size_t)q * cs + c] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < SAM_BATCH; ++u) m = egn_sam_max(m, v[u]);
      }
    }
    s_a[t] = m;
    __syncthreads();
    for (int off = top; off >= 1; off >>= 1) {
      if (live && j < off && j + off < S) s_a[t] = egn_sam_max(s_a[t], s_a[t + off * cwg]);
      __syncthreads();
    }
    m = s_a[cl];
    __syncthreads();
    egn_sam_sums a = {0.f, 0.f, 0.f};
    if (live) {
      sam_walk at(j, S, w);
      for (long p = j; p < hw; p += (long)S * SAM_BATCH) {
        float v[SAM_BATCH];
#pragma unroll
        for (int u = 0; u < SAM_BATCH; ++u) {
          const long q = p + (long)u * S;
          v[u] = q < hw ? zn[(size_t)q * cs + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < SAM_BATCH; ++u) {       // in increasing pixel order, as the header says
          if (p + (long)u * S < hw) {
            egn_sam_accum(a, v[u], m, at.x, at.y);
            at.next();
          }
        }
      }
    }
    s_a[t] = a.se;
    s_b[t] = a.sx;
    s_c[t] = a.sy;
    __syncthreads();
    for (int off = top; off >= 1; off >>= 1) {
      if (live && j < off && j + off < S) {
        const int o = t + off * cwg;
        egn_sam_sums mine = {s_a[t], s_b[t], s_c[t]}, other = {s_a[o], s_b[o], s_c[o]};
        egn_sam_fold(mine, other);
        s_a[t] = mine.se;
        s_b[t] = mine.sx;
        s_c[t] = mine.sy;
      }
      __syncthreads();
    }
    if (live && j == 0) {
      const egn_sam_sums tot = {s_a[t], s_b[t], s_c[t]};
      float cd[2], sv[4];
      egn_sam_finish(tot, m, div_x, div_y, cd, sv);
      const size_t e = (size_t)n * K + c;
      *reinterpret_cast<float2*>(coords + e * 2) = make_float2(cd[0], cd[1]);
      *reinterpret_cast<float4*>(save + e * 4) = make_float4(sv[0], sv[1], sv[2], sv[3]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SAM_BWD_THREADS) void softargmax_bwd_kernel(const float* __restrict__ z,
                                                                         const float* __restrict__ save,
                                                                         const float* __restrict__ dcoords, int h, int w,
                                                                         int K, int cs, float div_x, float div_y,
                                                                         int accumulate, float* __restrict__ dz) {
  const int n = blockIdx.y, t = threadIdx.x;
  const int cw = cs < SAM_BWD_THREADS ? cs : SAM_BWD_THREADS, S = SAM_BWD_THREADS / cw;
  const int j = t / cw, cl = t - j * cw;
  if (j >= S) return;
  const long hw = (long)h * w;
  const long p0 = (long)blockIdx.x * SAM_BWD_PIXELS;
  const long p1 = p0 + SAM_BWD_PIXELS < hw ? p0 + SAM_BWD_PIXELS : hw;
  const size_t base = (size_t)n * hw * cs;
  for (int c = cl; c < K; c += cw) {
    const size_t e = (size_t)n * K + c;
    const float4 sv = *reinterpret_cast<const float4*>(save + e * 4);
    const float2 g = *reinterpret_cast<const float2*>(dcoords + e * 2);
    const float svv[4] = {sv.x, sv.y, sv.z, sv.w}, gv[2] = {g.x, g.y};
    const egn_sam_back b = egn_sam_back_of(svv, gv, div_x, div_y);
    sam_walk at(p0 + j, S, w);
#pragma unroll 4
    for (long p = p0 + j; p < p1; p += S) {
      const size_t i = base + (size_t)p * cs + c;
      const float d = egn_sam_dz(b, z[i], at.x, at.y);
      dz[i] = accumulate ? dz[i] + d : d;
      at.next();
    }
  }
}

static bool sam_misaligned(const void* p, uintptr_t a) { return !p || ((uintptr_t)p & (a - 1)) != 0; }

static bool sam_bad_shape(int N, int h, int w, int K, int cs, float div_x, float div_y) {
  return N < 1 || h < 1 || w < 1 || K < 1 || K > cs || cs % 4 != 0 || !(div_x > 0.f) || !(div_y > 0.f);
}

extern "C" int egn_softargmax_fwd_f32(const float* z, int N, int h, int w, int K, int cs, float div_x, float div_y,
                                      float* coords, float* save, void* stream) {
  if (sam_bad_shape(N, h, w, K, cs, div_x, div_y) || sam_misaligned(z, 16) || sam_misaligned(coords, 8) ||
      sam_misaligned(save, 16))
    return EGN_E_BADARG;
  // a block = S slices x cwg channels of one image; the groups of an image run on different CUs (the order of every
  // sum is the header's whatever cwg is)
  const int cw = egn_sam_chan_width(cs), cwg = cw < SAM_FWD_GROUP ? cw : SAM_FWD_GROUP;
  hipLaunchKernelGGL(softargmax_fwd_kernel, dim3(N, (cw + cwg - 1) / cwg), dim3(egn_sam_slices(cs) * cwg), 0,
                     (hipStream_t)stream, z, h, w, K, cs, cwg, div_x, div_y, coords, save);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_softargmax_bwd_f32(const float* z, const float* save, const float* dcoords, int N, int n_rows, int h,
                                      int w, int K, int cs, float div_x, float div_y, int accumulate, float* dz,
                                      void* stream) {
  if (sam_bad_shape(N, h, w, K, cs, div_x, div_y) || n_rows < 0 || n_rows > N || sam_misaligned(z, 16) ||
      sam_misaligned(save, 16) || sam_misaligned(dcoords, 8) || sam_misaligned(dz, 16))
    return EGN_E_BADARG;
  if (n_rows == 0) return 0;
  const long chunks = ((long)h * w + SAM_BWD_PIXELS - 1) / SAM_BWD_PIXELS;
  if (chunks > 0x7fffffffL || n_rows > 65535) return EGN_E_BADARG;
  hipLaunchKernelGGL(softargmax_bwd_kernel, dim3((unsigned)chunks, n_rows), dim3(SAM_BWD_THREADS), 0, (hipStream_t)stream,
                     z, save, dcoords, h, w, K, cs, div_x, div_y, accumulate, dz);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// host twins: plain loops over the same header, the same order -- the same bits
// ---------------------------------------------------------------------------------------------------------------
extern "C" int egn_softargmax_fwd_host_f32(const float* z, int N, int h, int w, int K, int cs, float div_x, float div_y,
                                           float* coords, float* save) {
  if (sam_bad_shape(N, h, w, K, cs, div_x, div_y) || sam_misaligned(z, 16) || sam_misaligned(coords, 8) ||
      sam_misaligned(save, 16))
    return EGN_E_BADARG;
  const int S = egn_sam_slices(cs), top = egn_sam_tree_top(S);
  const long hw = (long)h * w;
  float pm[EGN_SAM_MAX_SLICES];
  egn_sam_sums ps[EGN_SAM_MAX_SLICES];
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < K; ++c) {
      const float* zc = z + (size_t)n * hw * cs + c;
      for (int j = 0; j < S; ++j) {
        pm[j] = -INFINITY;
        for (long p = j; p < hw; p += S) pm[j] = egn_sam_max(pm[j], zc[(size_t)p * cs]);
      }
      for (int off = top; off >= 1; off >>= 1)
        for (int j = 0; j < off && j + off < S; ++j) pm[j] = egn_sam_max(pm[j], pm[j + off]);
      const float m = pm[0];
      for (int j = 0; j < S; ++j) {
        ps[j] = egn_sam_sums{0.f, 0.f, 0.f};
        for (long p = j; p < hw; p += S) egn_sam_accum(ps[j], zc[(size_t)p * cs], m, (int)(p % w), (int)(p / w));
      }
      for (int off = top; off >= 1; off >>= 1)
        for (int j = 0; j < off && j + off < S; ++j) egn_sam_fold(ps[j], ps[j + off]);
      const size_t e = (size_t)n * K + c;
      egn_sam_finish(ps[0], m, div_x, div_y, coords + e * 2, save + e * 4);
    }
  return 0;
}

extern "C" int egn_softargmax_bwd_host_f32(const float* z, const float* save, const float* dcoords, int N, int n_rows,
                                           int h, int w, int K, int cs, float div_x, float div_y, int accumulate,
                                           float* dz) {
  if (sam_bad_shape(N, h, w, K, cs, div_x, div_y) || n_rows < 0 || n_rows > N || sam_misaligned(z, 16) ||
      sam_misaligned(save, 16) || sam_misaligned(dcoords, 8) || sam_misaligned(dz, 16))
    return EGN_E_BADARG;
  const long hw = (long)h * w;
  for (int n = 0; n < n_rows; ++n)
    for (int c = 0; c < K; ++c) {
      const size_t e = (size_t)n * K + c;
      const egn_sam_back b = egn_sam_back_of(save + e * 4, dcoords + e * 2, div_x, div_y);
      for (long p = 0; p < hw; ++p) {
        const size_t i = ((size_t)n * hw + p) * cs + c;
        const float d = egn_sam_dz(b, z[i], (int)(p % w), (int)(p / w));
        dz[i] = accumulate ? dz[i] + d : d;
      }
    }
  return 0;
}
