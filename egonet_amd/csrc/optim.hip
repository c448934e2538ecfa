// The optimizer step for parameter groups: torch.optim.Adam / AdamW / SGD over the flat parameter buffer of a native
// training step (train_common.FlatParams) with per-group hyper-parameters, AMSGrad, Nesterov, dampening, and
// torch.nn.utils.clip_grad_norm_ folded into the update.  include/egonet_hip.h states the arithmetic.
//
// ONE update launch whatever the number of groups.  The host cuts the buffer into work items (begin, length <=
// OPT_ITEM floats, group) that never cross the boundary between two groups' segments; a wave takes one item at a
// time, a lane up to OPT_ITEM / 256 float4 of it, 64 float4 apart.  Everything that changes between steps is read
// from device memory (the group table with the learning rates, the step counter, the clip coefficient), so a captured
// step replays correctly -- the rule adam_dev_kernel (train_ops.hip) follows.
#include <math.h>

#include "egn_internal.h"

namespace {

constexpr int OPT_ITEM = 1024;                  // floats per work item: 4 float4 per lane of a wave
constexpr int OPT_THREADS = 256;
constexpr int OPT_WAVES = OPT_THREADS / 64;
constexpr int OPT_BLOCKS_PER_CU = 8;
constexpr int NORM_BLOCKS = 1024;               // the fixed grid of the norm's first launch
constexpr int NORM_THREADS = 256;

__global__ void optim_tick_kernel(int* __restrict__ state) { state[0] += 1; }

// what a block derives once from a group's row and the step counter
struct GroupDerived {
  float step_size;   // Adam: lr / (1 - b1^t); SGD: lr
  float bc2_sqrt;    // sqrt(1 - b2^t)
  float decay;       // AdamW: 1 - lr wd
  float wd;          // coupled weight decay (0 for AdamW)
};

__device__ inline float4 ld4(const float* a, long q) { return reinterpret_cast<const float4*>(a)[q]; }
__device__ inline void st4(float* a, long q, const float4& x) { reinterpret_cast<float4*>(a)[q] = x; }

template <int FAMILY>
__global__ __launch_bounds__(OPT_THREADS) void optim_grouped_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    float* __restrict__ vmax, const egn_optim_group* __restrict__ groups, int ngroups,
    const egn_optim_item* __restrict__ items, long nitems, const float* __restrict__ clip,
    const int* __restrict__ state) {
  __shared__ GroupDerived s_d[EGN_OPTIM_MAX_GROUPS];
  __shared__ egn_optim_group s_g[EGN_OPTIM_MAX_GROUPS];
  const int t_step = state[0];
  if ((int)threadIdx.x < ngroups) {
    const egn_optim_group gr = groups[threadIdx.x];
    GroupDerived d;
    if (FAMILY == EGN_OPTIM_SGD) {
      d.step_size = gr.lr;
      d.bc2_sqrt = 1.f;
      d.decay = 1.f;
      d.wd = gr.weight_decay;
    } else {
      const double t = (double)t_step;
      d.step_size = (float)((double)gr.lr / (1.0 - pow((double)gr.beta1, t)));
      d.bc2_sqrt = (float)sqrt(1.0 - pow((double)gr.beta2, t));
      d.decay = (float)(1.0 - (double)gr.lr * (double)gr.weight_decay);
      d.wd = FAMILY == EGN_OPTIM_ADAMW ? 0.f : gr.weight_decay;
    }
    s_d[threadIdx.x] = d;
    s_g[threadIdx.x] = gr;
  }
  __syncthreads();
  const float coef = clip ? clip[1] : 1.f;
  const bool first = t_step <= 1;
  const int lane = threadIdx.x & 63;
  const long wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (long it = (long)blockIdx.x * OPT_WAVES + wave; it < nitems; it += (long)gridDim.x * OPT_WAVES) {
    const egn_optim_item item = items[it];
    const egn_optim_group gr = s_g[item.group];
    const GroupDerived d = s_d[item.group];
    const long q0 = item.begin >> 2;
    const int nq = item.length >> 2;
#pragma unroll
    for (int k = 0; k < OPT_ITEM / 256; ++k) {
      const int j = lane + 64 * k;
      if (j >= nq) break;
      const long q = q0 + j;
      const float4 p4 = ld4(p, q), g4 = ld4(g, q);
      float pe[4] = {p4.x, p4.y, p4.z, p4.w};
      float ge[4] = {g4.x, g4.y, g4.z, g4.w};
      if (FAMILY == EGN_OPTIM_SGD) {
        const float mu = gr.momentum;
        if (mu != 0.f) {
          const float4 b4 = ld4(m, q);
          float be[4] = {b4.x, b4.y, b4.z, b4.w};
          const float keep = 1.f - gr.dampening;
          const bool nesterov = (gr.flags & EGN_OPTIM_NESTEROV) != 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float gi = ge[c] * coef + d.wd * pe[c];
            const float bi = first ? gi : mu * be[c] + keep * gi;
            be[c] = bi;
            pe[c] = pe[c] - d.step_size * (nesterov ? gi + mu * bi : bi);
          }
          st4(m, q, make_float4(be[0], be[1], be[2], be[3]));
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) pe[c] = pe[c] - d.step_size * (ge[c] * coef + d.wd * pe[c]);
        }
      } else {
        const float4 m4 = ld4(m, q), v4 = ld4(v, q);
        float me[4] = {m4.x, m4.y, m4.z, m4.w};
        float ve[4] = {v4.x, v4.y, v4.z, v4.w};
        const bool ams = (gr.flags & EGN_OPTIM_AMSGRAD) != 0;
        float xe[4] = {0.f, 0.f, 0.f, 0.f};
        if (ams) {
          const float4 x4 = ld4(vmax, q);
          xe[0] = x4.x, xe[1] = x4.y, xe[2] = x4.z, xe[3] = x4.w;
        }
        const float b1 = gr.beta1, b2 = gr.beta2;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float pc = pe[c];
          if (FAMILY == EGN_OPTIM_ADAMW) pc = pc * d.decay;
          const float gi = ge[c] * coef + d.wd * pc;
          const float mi = b1 * me[c] + (1.f - b1) * gi;
          const float vi = b2 * ve[c] + (1.f - b2) * gi * gi;
          me[c] = mi;
          ve[c] = vi;
          float vd = vi;
          if (ams) {
            // torch.maximum: a NaN on either side stays a NaN
            vd = (vi != vi || xe[c] != xe[c]) ? vi + xe[c] : (xe[c] > vi ? xe[c] : vi);
            xe[c] = vd;
          }
          pe[c] = pc - d.step_size * (mi / (sqrtf(vd) / d.bc2_sqrt + gr.eps));
        }
        st4(m, q, make_float4(me[0], me[1], me[2], me[3]));
        st4(v, q, make_float4(ve[0], ve[1], ve[2], ve[3]));
        if (ams) st4(vmax, q, make_float4(xe[0], xe[1], xe[2], xe[3]));
      }
      st4(p, q, make_float4(pe[0], pe[1], pe[2], pe[3]));
    }
  }
}

// sum of squares in double: thread partials over a grid-stride loop of float4, then a fixed tree per block
__device__ inline double block_sum_fixed(double acc, double* s) {
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = NORM_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(NORM_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, long nq,
                                                                  double* __restrict__ partial) {
  __shared__ double s[NORM_THREADS];
  double acc = 0.0;
  for (long q = (long)blockIdx.x * NORM_THREADS + threadIdx.x; q < nq; q += (long)NORM_BLOCKS * NORM_THREADS) {
    const float4 x = ld4(g, q);
    acc += (double)x.x * x.x;
    acc += (double)x.y * x.y;
    acc += (double)x.z * x.z;
    acc += (double)x.w * x.w;
  }
  const double tot = block_sum_fixed(acc, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(NORM_THREADS) void grad_norm_finish_kernel(const double* __restrict__ partial,
                                                                        float max_norm, float* __restrict__ clip) {
  __shared__ double s[NORM_THREADS];
  double acc = 0.0;
  for (int k = threadIdx.x; k < NORM_BLOCKS; k += NORM_THREADS) acc += partial[k];
  const double tot = block_sum_fixed(acc, s);
  if (threadIdx.x == 0) {
    const double norm = sqrt(tot);
    const double c = (double)max_norm / (norm + 1e-6);
    const float2 out = make_float2((float)norm, (float)(c > 1.0 ? 1.0 : c));   // a NaN c stays NaN (torch.clamp)
    *reinterpret_cast<float2*>(clip) = out;
  }
}

bool misaligned(const void* p, uintptr_t a) { return !p || ((uintptr_t)p & (a - 1)) != 0; }
bool nonneg_finite(float x) { return x >= 0.f && isfinite(x); }

bool bad_group(int family, const egn_optim_group& gr) {
  if (!nonneg_finite(gr.lr) || !nonneg_finite(gr.weight_decay)) return true;
  if (family == EGN_OPTIM_SGD) {
    if (gr.flags & ~EGN_OPTIM_NESTEROV) return true;
    if (!nonneg_finite(gr.momentum) || !(gr.dampening >= 0.f && gr.dampening <= 1.f)) return true;
    if ((gr.flags & EGN_OPTIM_NESTEROV) && (gr.momentum == 0.f || gr.dampening != 0.f)) return true;
    return false;
  }
  if (gr.flags & ~EGN_OPTIM_AMSGRAD) return true;
  if (!(gr.beta1 >= 0.f && gr.beta1 < 1.f) || !(gr.beta2 >= 0.f && gr.beta2 < 1.f)) return true;
  return !(gr.eps > 0.f) || !isfinite(gr.eps);
}

}  // namespace

extern "C" int egn_optim_item_floats(void) { return OPT_ITEM; }

extern "C" int egn_optim_grouped_step_f32(int family, float* p, const float* g, float* m, float* v, float* vmax,
                                          long n, const egn_optim_group* groups_host,
                                          const egn_optim_group* groups_dev, int ngroups,
                                          const egn_optim_item* items_host, const egn_optim_item* items_dev,
                                          long nitems, const float* clip, int* step_dev, void* stream) {
  if (family < EGN_OPTIM_ADAM || family > EGN_OPTIM_SGD) return EGN_E_BADARG;
  if (n < 1 || n % 4 || ngroups < 1 || ngroups > EGN_OPTIM_MAX_GROUPS || nitems < 1) return EGN_E_BADARG;
  if (misaligned(p, 16) || misaligned(g, 16) || !groups_host || misaligned(groups_dev, 4) || !items_host ||
      misaligned(items_dev, 8) || misaligned(step_dev, 4) || (clip && misaligned(clip, 8)))
    return EGN_E_BADARG;
  bool any_ams = false, any_momentum = false;
  for (int k = 0; k < ngroups; ++k) {
    if (bad_group(family, groups_host[k])) return EGN_E_BADARG;
    any_ams |= (groups_host[k].flags & EGN_OPTIM_AMSGRAD) != 0;
    any_momentum |= groups_host[k].momentum != 0.f;
  }
  if (family == EGN_OPTIM_SGD) {
    if (any_momentum && misaligned(m, 16)) return EGN_E_BADARG;
  } else {
    if (misaligned(m, 16) || misaligned(v, 16) || (any_ams && misaligned(vmax, 16))) return EGN_E_BADARG;
  }
  long long at = 0;
  for (long k = 0; k < nitems; ++k) {
    const egn_optim_item& it = items_host[k];
    if (it.begin != at || it.length < 4 || it.length > OPT_ITEM || it.length % 4 || it.group < 0 ||
        it.group >= ngroups || it.begin + it.length > n)
      return EGN_E_BADARG;
    at += it.length;
  }
  if (at != n) return EGN_E_BADARG;

  const hipStream_t st = (hipStream_t)stream;
  const long want = (nitems + OPT_WAVES - 1) / OPT_WAVES;
  const long cap = (long)OPT_BLOCKS_PER_CU * egn_device_cus();
  const dim3 grid((unsigned)(want < cap ? want : cap)), block(OPT_THREADS);
  hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(1), 0, st, step_dev);
  if (family == EGN_OPTIM_ADAM)
    hipLaunchKernelGGL(optim_grouped_kernel<EGN_OPTIM_ADAM>, grid, block, 0, st, p, g, m, v, vmax, groups_dev, ngroups,
                       items_dev, nitems, clip, step_dev);
  else if (family == EGN_OPTIM_ADAMW)
    hipLaunchKernelGGL(optim_grouped_kernel<EGN_OPTIM_ADAMW>, grid, block, 0, st, p, g, m, v, vmax, groups_dev, ngroups,
                       items_dev, nitems, clip, step_dev);
  else
    hipLaunchKernelGGL(optim_grouped_kernel<EGN_OPTIM_SGD>, grid, block, 0, st, p, g, m, v, vmax, groups_dev, ngroups,
                       items_dev, nitems, clip, step_dev);
  egn_count_launches(2);
  return (int)hipGetLastError();
}

extern "C" long egn_grad_norm_ws_bytes(void) { return (long)NORM_BLOCKS * (long)sizeof(double); }

extern "C" int egn_grad_norm_clip_f32(const float* g, long n, float max_norm, double* ws, float* clip, void* stream) {
  if (misaligned(g, 16) || misaligned(ws, 8) || misaligned(clip, 8) || n < 1 || n % 4 || !(max_norm >= 0.f))
    return EGN_E_BADARG;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(NORM_BLOCKS), dim3(NORM_THREADS), 0, st, g, n / 4, ws);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(NORM_THREADS), 0, st, ws, max_norm, clip);
  egn_count_launches(2);
  return (int)hipGetLastError();
}
