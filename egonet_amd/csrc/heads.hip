// heads.hip -- the training-side layers of the two HRNet heads the trunk tape did not cover
// (reference: libs/model/heatmapModel/hrnet.py:373-422, 596-611; libs/loss/function.py:22-46):
//
//   * the heat-map criterion on PIXEL-SHUFFLED maps, read straight from the pre-shuffle NHWC
//     activations (the shuffled prediction is never materialised for the loss), gradient written
//     back in the pre-shuffle layout;
//   * PixelUnshuffle NCHW -> padded NHWC: the backward of egn_pixel_shuffle_nhwc_to_nchw_f32 when
//     torch hands the maps' gradient to the autograd bridge;
//   * non-overlapping k x k average pooling over NHWC, forward and backward (the angle head's
//     AvgPool2d(4) on its 4 x 4 map).
//
// Activations are NHWC [N, H, W, cs] fp32 with cs % 4 == 0 (engine.Buf).
#include "egn_internal.h"

static inline int heads_grid(size_t work_items, int block) {
  size_t g = (work_items + block - 1) / block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------------------
// Heat-map criterion on pixel-shuffled maps.
//   pre-shuffle x [N, h, w, cs], channel j*f*f + dy*f + dx  <->  map[n, j, y*f + dy, x*f + dx]
//   target NCHW [N, J, f*h, f*w];  tw [N, J] or null (JointsMSELoss use_target_weight)
//   loss += weight * mean(c(pred*w - tgt*w));  dx = weight * c'(pred*w - tgt*w) / total * w
// One block = one pre-shuffle row segment of TW pixels: its TW*cs floats are contiguous in x
// (16-byte loads into LDS), the same pixels' target rows are contiguous runs of TW*f floats per
// (j, dy) (16-byte loads where the map width allows it).  The gradient overwrites the prediction
// in LDS (each slot is read and written by the one thread that owns the output element) and
// leaves as contiguous 16-byte rows, pad channels zeroed.  LDS pitch cs + 1: the f-strided
// pixel walk of stage 2 spreads over the banks.
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void pixshuf_loss_kernel(const float* __restrict__ x, const float* __restrict__ tgt,
                                                           const float* __restrict__ tw, int h, int w, int J, int f,
                                                           int cs, int TW, int crit, double inv,
                                                           float* __restrict__ dx, double* __restrict__ loss) {
  extern __shared__ float lds[];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int pitch = cs + 1;
  const int ntw = (w + TW - 1) / TW;
  const int tile = blockIdx.x % ntw;
  const int row = blockIdx.x / ntw;            // n * h + y
  const int n = row / h, y = row - n * h;
  const int w0 = tile * TW;
  const int npx = min(TW, w - w0);
  const size_t xoff = ((size_t)row * w + w0) * cs;
  const int nq = npx * cs / 4;
  const float4* xr = reinterpret_cast<const float4*>(x + xoff);
  for (int q = tid; q < nq; q += 256) {
    const float4 v = xr[q];
    const int e = q * 4;
    const int px = e / cs, c = e - px * cs;
    float* d = lds + px * pitch + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();

  const int ff = f * f;
  const int segw = npx * f;                   // target floats per (j, dy) row run
  const int per_j = f * segw;
  const int tot = J * per_j;
  const size_t fH = (size_t)h * f, fW = (size_t)w * f;
  double acc = 0.0;
  auto one = [&](int j, int dyy, int ox, float t) {
    const int px = ox / f, dxx = ox - px * f;
    float* slot = lds + px * pitch + j * ff + dyy * f + dxx;
    const float wj = tw ? tw[(size_t)n * J + j] : 1.f;
    const float d = tw ? (*slot * wj - t * wj) : (*slot - t);
    const float ad = fabsf(d);
    double v, gd;
    if (crit == 0) { v = (double)d * d; gd = 2.0 * d; }
    else if (crit == 1) { v = ad; gd = d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0); }
    else if (ad < 1.f) { v = 0.5 * (double)d * d; gd = d; }
    else { v = (double)ad - 0.5; gd = d > 0.f ? 1.0 : -1.0; }
    acc += v;
    const float g = (float)(gd * inv);
    *slot = tw ? g * wj : g;
  };
  if (VEC) {
    for (int q = tid; q < tot / 4; q += 256) {
      const int e = q * 4;
      const int j = e / per_j, r = e - j * per_j;
      const int dyy = r / segw, ox = r - dyy * segw;
      const float4 t4 = *reinterpret_cast<const float4*>(
          tgt + ((size_t)(n * J + j) * fH + (size_t)y * f + dyy) * fW + (size_t)w0 * f + ox);
      one(j, dyy, ox, t4.x);
      one(j, dyy, ox + 1, t4.y);
      one(j, dyy, ox + 2, t4.z);
      one(j, dyy, ox + 3, t4.w);
    }
  } else {
    for (int e = tid; e < tot; e += 256) {
      const int j = e / per_j, r = e - j * per_j;
      const int dyy = r / segw, ox = r - dyy * segw;
      one(j, dyy, ox, tgt[((size_t)(n * J + j) * fH + (size_t)y * f + dyy) * fW + (size_t)w0 * f + ox]);
    }
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();                             // (also: every gradient slot of LDS is written)
  if (tid == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);
  if (dx) {
    const int C = J * ff;
    float4* dr = reinterpret_cast<float4*>(dx + xoff);
    for (int q = tid; q < nq; q += 256) {
      const int e = q * 4;
      const int px = e / cs, c = e - px * cs;
      const float* s = lds + px * pitch + c;
      dr[q] = make_float4(c < C ? s[0] : 0.f, c + 1 < C ? s[1] : 0.f, c + 2 < C ? s[2] : 0.f, c + 3 < C ? s[3] : 0.f);
    }
  }
}

extern "C" int egn_pixshuf_loss_f32(const float* x, const float* tgt, const float* tw, int N, int H, int W, int C,
                                    int up, int cs, int crit, float weight, float* dx, double* loss, void* stream) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || up < 1 || cs % 4 || cs < C * up * up || crit < 0 || crit > 2 || !x ||
      !tgt || !loss)
    return EGN_E_BADARG;
  if (((uintptr_t)x | (uintptr_t)dx) & 15) return EGN_E_BADARG;
  int TW = 16;
  while (TW > 1 && (size_t)TW * (cs + 1) * 4 > 65024) TW >>= 1;      // + the block's reduction words <= 64 KiB
  const size_t lds = (size_t)TW * (cs + 1) * 4;
  if (lds > 65024) return EGN_E_BADARG;
  const size_t blocks = (size_t)N * H * ((W + TW - 1) / TW);
  if (blocks > 0x7fffffff) return EGN_E_BADARG;
  const double total = (double)N * C * H * up * W * up;
  const double inv = (double)weight / total;
  const bool vec = ((W * up) % 4 == 0) && ((TW * up) % 4 == 0) && !((uintptr_t)tgt & 15);
  if (vec)
    hipLaunchKernelGGL(pixshuf_loss_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, tgt,
                       tw, H, W, C, up, cs, TW, crit, inv, dx, loss);
  else
    hipLaunchKernelGGL(pixshuf_loss_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x,
                       tgt, tw, H, W, C, up, cs, TW, crit, inv, dx, loss);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// PixelUnshuffle(up) fused with the NCHW -> padded NHWC hand-over, the exact inverse of
// pixel_shuffle_kernel (elementwise.hip):  y[n, h, w, j*up*up + a*up + b] = x[n, j, h*up + a, w*up + b],
// pad channels (>= C*up*up) zero.  One thread per 16-byte group of y.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pixel_unshuffle_kernel(const float* __restrict__ x, float4* __restrict__ y,
                                                              int N, int C, int H, int W, int cs, int up) {
  const int uu = up * up, CC = C * uu;
  const size_t Ho = (size_t)H * up, Wo = (size_t)W * up;
  const size_t total = (size_t)N * H * W * (cs / 4);
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    const size_t pix = e / cs;
    const int c0 = (int)(e - pix * cs);
    const int ww = (int)(pix % W);
    const int hh = (int)((pix / W) % H);
    const int n = (int)(pix / ((size_t)W * H));
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k;
      if (c < CC) {
        const int j = c / uu, r = c - j * uu, a = r / up, b = r - a * up;
        v[k] = x[(((size_t)n * C + j) * Ho + (size_t)hh * up + a) * Wo + (size_t)ww * up + b];
      } else {
        v[k] = 0.f;
      }
    }
    y[q] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

extern "C" int egn_pixel_unshuffle_nchw_to_nhwc_f32(const float* x, float* y, int N, int C, int H, int W, int cs,
                                                    int up, void* stream) {
  if (!x || !y || N < 1 || H < 1 || W < 1 || up < 1 || C < 1 || cs % 4 || cs < C * up * up || ((uintptr_t)y & 15))
    return EGN_E_BADARG;
  const size_t total = (size_t)N * H * W * (cs / 4);
  hipLaunchKernelGGL(pixel_unshuffle_kernel, dim3(heads_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x,
                     reinterpret_cast<float4*>(y), N, C, H, W, cs, up);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// AvgPool2d(k) (stride k, no padding, floor) over NHWC: [N, H, W, cs] -> [N, H/k, W/k, cs].
// Forward: the k*k taps summed in row-major order, then / (k*k) (torch's order of operations).
// Backward: dx = dy / (k*k) broadcast over each window (= or += with accumulate); the rows /
// columns a floor-sized window leaves out get 0 (or stay).  One thread per 16-byte group.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const float4* __restrict__ x, float4* __restrict__ y, int N,
                                                          int H, int W, int cq, int k) {
  const int Ho = H / k, Wo = W / k;
  const float div = (float)(k * k);
  const size_t total = (size_t)N * Ho * Wo * cq;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % cq);
    const size_t pix = e / cq;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((size_t)Wo * Ho));
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int u = 0; u < k; ++u) {
      const float4* r = x + (((size_t)n * H + oy * k + u) * W + (size_t)ox * k) * cq + c;
      for (int v = 0; v < k; ++v) {
        const float4 t = r[(size_t)v * cq];
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
    }
    y[e] = make_float4(s.x / div, s.y / div, s.z / div, s.w / div);
  }
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float4* __restrict__ dy, float4* __restrict__ dx, int N,
                                                          int H, int W, int cq, int k, int accumulate) {
  const int Ho = H / k, Wo = W / k;
  const float div = (float)(k * k);
  const size_t total = (size_t)N * H * W * cq;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % cq);
    const size_t pix = e / cq;
    const int xx = (int)(pix % W);
    const int yy = (int)((pix / W) % H);
    const int n = (int)(pix / ((size_t)W * H));
    const int oy = yy / k, ox = xx / k;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (oy < Ho && ox < Wo) {
      const float4 t = dy[(((size_t)n * Ho + oy) * Wo + ox) * cq + c];
      g = make_float4(t.x / div, t.y / div, t.z / div, t.w / div);
    }
    if (accumulate) {
      const float4 o = dx[e];
      g = make_float4(o.x + g.x, o.y + g.y, o.z + g.z, o.w + g.w);
    }
    dx[e] = g;
  }
}

extern "C" int egn_avgpool_fwd_f32(const float* x, float* y, int N, int H, int W, int cs, int k, void* stream) {
  if (!x || !y || N < 1 || k < 1 || H < k || W < k || cs < 4 || cs % 4 || (((uintptr_t)x | (uintptr_t)y) & 15))
    return EGN_E_BADARG;
  const size_t total = (size_t)N * (H / k) * (W / k) * (cs / 4);
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(heads_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), N, H, W, cs / 4, k);
  return (int)hipGetLastError();
}

extern "C" int egn_avgpool_bwd_f32(const float* dy, float* dx, int N, int H, int W, int cs, int k, int accumulate,
                                   void* stream) {
  if (!dy || !dx || N < 1 || k < 1 || H < k || W < k || cs < 4 || cs % 4 || (((uintptr_t)dy | (uintptr_t)dx) & 15))
    return EGN_E_BADARG;
  const size_t total = (size_t)N * H * W * (cs / 4);
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(heads_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(dy), reinterpret_cast<float4*>(dx), N, H, W, cs / 4, k,
                     accumulate);
  return (int)hipGetLastError();
}
