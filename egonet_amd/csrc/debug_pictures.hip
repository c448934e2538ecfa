// debug_pictures.hip -- the training debug pictures of libs/visualization/debug.py composed on the device
// (definition: debug_pictures_math.h): the range of the crops, the grid of crops and the heat-map mosaic, each with a
// host twin built from the same header.  Bandwidth-bound, no floating-point colour math (the colour map is a table
// handed in as data), no drawing: markers go through overlay.hip on the finished picture.
//
// Range: one block per (channel plane, chunk of DP_RANGE_CHUNK floats) writes its {lo, hi} with plain stores, one block
// folds them in index order and stores lohi; min / max are exact, so any order gives the same bits.
// Grid: a thread owns four pixels of a picture row (12 bytes); padding and empty cells are zeros.
// Mosaic: a block owns one crop x a strip of thumbnail rows (x a chunk of columns when a map is wider than
// DP_STRIP_PX, x a share of the joints when there are few blocks).  It builds its strip of the thumbnail once in LDS,
// reading only the crop pixels the bilinear taps name, then walks its joints: float4 loads along w where the maps
// allow, 4 pixels = 12 bytes per store, a tail for w % 4 != 0.  Rows are addressed by bytes.
#include "egn_internal.h"
#include "debug_pictures_math.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_RANGE_CHUNK = 4096;   // floats per block of the range's first pass
constexpr int DP_STRIP_PX = 1024;      // thumbnail pixels a mosaic block keeps in LDS (3 KB); a multiple of 4
constexpr int DP_RUN = 4;              // pixels per thread and store
constexpr int DP_MAX_JSPLIT = 8;

// 3 * npx bytes to dst: three dwords where the run is whole and dst is dword-aligned, else bytes
__device__ inline void dp_store_run(uint8_t* dst, const unsigned (&px)[DP_RUN * 3], int npx) {
  if (npx == DP_RUN && ((uintptr_t)dst & 3u) == 0) {
    uint32_t* d = (uint32_t*)dst;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      d[k] = px[4 * k] | px[4 * k + 1] << 8 | px[4 * k + 2] << 16 | px[4 * k + 3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < DP_RUN * 3; ++k)
      if (k < 3 * npx) dst[k] = (uint8_t)px[k];
  }
}

struct dp_range_shape {
  int64_t rows, chunks, parts;
};
// false = a negative size or more partials than a grid holds; parts == 0 = nothing to do
bool dp_range_shape_of(int n, int c, int c_used, int hw, dp_range_shape* s) {
  if (n < 0 || c < 0 || c_used < 0 || hw < 0 || c_used > c) return false;
  s->rows = (int64_t)n * c_used;
  s->chunks = ((int64_t)hw + DP_RANGE_CHUNK - 1) / DP_RANGE_CHUNK;
  s->parts = s->rows * s->chunks;
  return s->parts <= 0x7fffffff;
}

}  // namespace

__global__ __launch_bounds__(DP_THREADS) void debug_range_partial_kernel(const float* __restrict__ x, int c, int c_used,
                                                                         int hw, int chunks, float* __restrict__ part,
                                                                         int vec) {
  __shared__ float s_lo[DP_THREADS / 64], s_hi[DP_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / (unsigned)chunks, ck = blockIdx.x % (unsigned)chunks;
  const float* p = x + ((size_t)(row / c_used) * (size_t)c + (size_t)(row % c_used)) * (size_t)hw;
  const int64_t e0 = ck * DP_RANGE_CHUNK;
  const int64_t e1 = e0 + DP_RANGE_CHUNK < hw ? e0 + DP_RANGE_CHUNK : hw;
  float lo, hi;
  egn_dbg_range_init(lo, hi);
  if (vec) {   // hw % 4 == 0 and x 16-byte aligned: every plane and chunk starts on a float4, e1 is a multiple of 4
    for (int64_t e = e0 + 4 * tid; e < e1; e += 4 * DP_THREADS) {
      const float4 v = *(const float4*)(p + e);
      egn_dbg_range_step(v.x, lo, hi);
      egn_dbg_range_step(v.y, lo, hi);
      egn_dbg_range_step(v.z, lo, hi);
      egn_dbg_range_step(v.w, lo, hi);
    }
  } else {
    for (int64_t e = e0 + tid; e < e1; e += DP_THREADS) egn_dbg_range_step(p[e], lo, hi);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {   // lo / hi hold no NaN: +-inf until a value was seen
    lo = egn_dbg_min(lo, __shfl_xor(lo, off, 64));
    hi = egn_dbg_max(hi, __shfl_xor(hi, off, 64));
  }
  if ((tid & 63) == 0) {
    s_lo[tid >> 6] = lo;
    s_hi[tid >> 6] = hi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < DP_THREADS / 64; ++k) {
      lo = egn_dbg_min(lo, s_lo[k]);
      hi = egn_dbg_max(hi, s_hi[k]);
    }
    part[2 * (size_t)blockIdx.x] = lo;
    part[2 * (size_t)blockIdx.x + 1] = hi;
  }
}

__global__ __launch_bounds__(DP_THREADS) void debug_range_fold_kernel(const float* __restrict__ part, int parts,
                                                                      float* __restrict__ lohi) {
  __shared__ float s_lo[DP_THREADS / 64], s_hi[DP_THREADS / 64];
  const int tid = threadIdx.x;
  float lo, hi;
  egn_dbg_range_init(lo, hi);
  for (int64_t k = tid; k < parts; k += DP_THREADS) {
    lo = egn_dbg_min(lo, part[2 * k]);
    hi = egn_dbg_max(hi, part[2 * k + 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = egn_dbg_min(lo, __shfl_xor(lo, off, 64));
    hi = egn_dbg_max(hi, __shfl_xor(hi, off, 64));
  }
  if ((tid & 63) == 0) {
    s_lo[tid >> 6] = lo;
    s_hi[tid >> 6] = hi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < DP_THREADS / 64; ++k) {
      lo = egn_dbg_min(lo, s_lo[k]);
      hi = egn_dbg_max(hi, s_hi[k]);
    }
    egn_dbg_range_finish(lo, hi);
    lohi[0] = lo;
    lohi[1] = hi;
  }
}

__global__ __launch_bounds__(DP_THREADS) void debug_grid_kernel(const float* __restrict__ img, int N, int C, int H,
                                                                int W, int pad, egn_dbg_grid g,
                                                                const float* __restrict__ lohi,
                                                                uint8_t* __restrict__ out, int64_t stride) {
  const int groups = (g.gw + DP_RUN - 1) / DP_RUN;
  const int64_t item = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x;
  if (item >= (int64_t)g.gh * groups) return;
  const int Y = (int)(item / groups), X0 = (int)(item % groups) * DP_RUN;
  const int npx = g.gw - X0 < DP_RUN ? g.gw - X0 : DP_RUN;
  const float lo = lohi[0], hi = lohi[1];
  unsigned px[DP_RUN * 3];
#pragma unroll
  for (int k = 0; k < DP_RUN; ++k) {
    int kk = 0, y = 0, x = 0;
    const bool in = k < npx && egn_dbg_grid_source(g, N, H, W, pad, Y, X0 + k, &kk, &y, &x);
    const float* p = img + (size_t)kk * (size_t)C * (size_t)H * (size_t)W + (size_t)y * (size_t)W + (size_t)x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) px[3 * k + ch] = in ? egn_dbg_quant_crop(p[(size_t)ch * (size_t)H * (size_t)W], lo, hi) : 0u;
  }
  dp_store_run(out + (size_t)Y * (size_t)stride + 3 * (size_t)X0, px, npx);
}

struct dp_mosaic_plan {
  int nc, cx, rows, strips, jc, jz;   // columns per block, column chunks, rows per strip, strips, joints per block, joint shares
  int64_t blocks;                     // n * strips * cx
};

__global__ __launch_bounds__(DP_THREADS) void debug_mosaic_kernel(const float* __restrict__ img, int C, int H, int W,
                                                                  const float* __restrict__ maps, int J, int h, int w,
                                                                  dp_mosaic_plan pl, const float* __restrict__ lohi,
                                                                  const uint8_t* __restrict__ lut,
                                                                  uint8_t* __restrict__ out, int64_t stride, int vec) {
  __shared__ uint8_t s_thumb[DP_STRIP_PX * 3];
  __shared__ uint8_t s_lut[768];
  const int tid = threadIdx.x;
  // everything up to the barrier is uniform over the block
  const int chunk = (int)(blockIdx.x % (unsigned)pl.cx);
  const int strip = (int)(blockIdx.x / (unsigned)pl.cx % (unsigned)pl.strips);
  const int i = (int)(blockIdx.x / (unsigned)pl.cx / (unsigned)pl.strips);
  const int y0 = strip * pl.rows, x0 = chunk * pl.nc;
  const int nr = h - y0 < pl.rows ? h - y0 : pl.rows;
  const int nc = w - x0 < pl.nc ? w - x0 : pl.nc;
  const int j0 = (int)blockIdx.y * pl.jc;
  const int j1 = j0 + pl.jc < J ? j0 + pl.jc : J;
  const float lo = lohi[0], hi = lohi[1];
  if (J > 0)
    for (int t = tid; t < 768; t += DP_THREADS) s_lut[t] = lut[t];
  const float* crop = img + (size_t)i * (size_t)C * (size_t)H * (size_t)W;
  for (int p = tid; p < nr * nc; p += DP_THREADS) {   // nr * nc <= DP_STRIP_PX
    const egn_dbg_tap ty = egn_dbg_tap_of(y0 + p / nc, H, h), tx = egn_dbg_tap_of(x0 + p % nc, W, w);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      s_thumb[3 * p + ch] = (uint8_t)egn_dbg_thumb(crop + (size_t)ch * (size_t)H * (size_t)W, W, ty, tx, lo, hi);
  }
  __syncthreads();
  const int groups = (nc + DP_RUN - 1) / DP_RUN;
  for (int it = tid; it < nr * groups; it += DP_THREADS) {
    const int r = it / groups, xr = it % groups * DP_RUN;   // xr: column inside the block's chunk
    const int npx = nc - xr < DP_RUN ? nc - xr : DP_RUN;
    uint8_t* orow = out + ((size_t)i * (size_t)h + (size_t)(y0 + r)) * (size_t)stride;
    unsigned th[DP_RUN * 3];
#pragma unroll
    for (int k = 0; k < DP_RUN * 3; ++k) th[k] = k < 3 * npx ? s_thumb[3 * (r * nc + xr) + k] : 0u;
    if (blockIdx.y == 0) dp_store_run(orow + 3 * (size_t)(x0 + xr), th, npx);
    for (int j = j0; j < j1; ++j) {
      const float* m = maps + (((size_t)i * (size_t)J + (size_t)j) * (size_t)h + (size_t)(y0 + r)) * (size_t)w + (size_t)(x0 + xr);
      float v[DP_RUN];
      if (vec && npx == DP_RUN) {   // w % 4 == 0 and maps 16-byte aligned: x0 and xr are multiples of 4
        const float4 q = *(const float4*)m;
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < DP_RUN; ++k) v[k] = k < npx ? m[k] : 0.0f;
      }
      unsigned px[DP_RUN * 3];
#pragma unroll
      for (int k = 0; k < DP_RUN; ++k) {
        const unsigned q = egn_dbg_quant_map(v[k]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) px[3 * k + ch] = egn_dbg_blend(s_lut[3 * q + ch], th[3 * k + ch]);
      }
      dp_store_run(orow + 3 * ((size_t)(j + 1) * (size_t)w + (size_t)(x0 + xr)), px, npx);
    }
  }
}

namespace {

// 1 = nothing to draw, 0 = go on, EGN_E_BADARG
int dp_grid_check(const void* img, int N, int C, int H, int W, int nrow, int pad, const void* lohi, const void* out,
                  long stride, egn_dbg_grid* g) {
  if (N < 0 || C < 0 || H < 0 || W < 0 || nrow < 0 || pad < 0 || stride < 0) return EGN_E_BADARG;
  if (N == 0 || H == 0 || W == 0) return 1;
  if (C < 3 || nrow < 1 || !img || !lohi || !out) return EGN_E_BADARG;
  if (!egn_dbg_grid_of(N, H, W, nrow, pad, g) || stride < 3 * (long)g->gw) return EGN_E_BADARG;
  return 0;
}

int dp_mosaic_check(const void* img, int C, int H, int W, const void* maps, int n, int J, int h, int w,
                    const void* lohi, const void* lut, const void* out, long stride) {
  if (C < 0 || H < 0 || W < 0 || n < 0 || J < 0 || h < 0 || w < 0 || stride < 0) return EGN_E_BADARG;
  if (n == 0 || h == 0 || w == 0) return 1;
  if (C < 3 || H < 1 || W < 1 || !img || !lohi || !out || (J > 0 && (!maps || !lut))) return EGN_E_BADARG;
  if (((int64_t)J + 1) * w > 0x7fffffff / 3 || (int64_t)n * h > 0x7fffffff) return EGN_E_BADARG;
  if (stride < 3 * ((long)J + 1) * w) return EGN_E_BADARG;
  return 0;
}

bool dp_mosaic_plan_of(int n, int J, int h, int w, dp_mosaic_plan* pl) {
  pl->nc = w < DP_STRIP_PX ? w : DP_STRIP_PX;
  pl->cx = (w + pl->nc - 1) / pl->nc;
  const int groups = (pl->nc + DP_RUN - 1) / DP_RUN;
  int rows = DP_THREADS / groups < DP_STRIP_PX / pl->nc ? DP_THREADS / groups : DP_STRIP_PX / pl->nc;
  rows = rows < 1 ? 1 : (rows > h ? h : rows);
  pl->rows = rows;
  pl->strips = (h + rows - 1) / rows;
  pl->blocks = (int64_t)n * pl->strips * pl->cx;
  if (pl->blocks > 0x7fffffff) return false;
  // few blocks: the joints are shared out, each share builds the strip again (two blocks per CU of 256 is the aim)
  int64_t jz = (512 + pl->blocks - 1) / pl->blocks;
  jz = jz > DP_MAX_JSPLIT ? DP_MAX_JSPLIT : jz;
  jz = jz > J ? J : jz;
  jz = jz < 1 ? 1 : jz;
  pl->jc = (int)((J + jz - 1) / jz);
  pl->jz = pl->jc > 0 ? (J + pl->jc - 1) / pl->jc : 1;
  return true;
}

}  // namespace

extern "C" long egn_debug_range_ws_bytes(int n, int c_used, int hw) {
  dp_range_shape s;
  if (!dp_range_shape_of(n, c_used, c_used, hw, &s)) return -1;
  return (long)(s.parts > 0 ? s.parts : 1) * 2 * (long)sizeof(float);
}

extern "C" int egn_debug_range_f32(const float* x, int n, int c, int c_used, int hw, void* ws, long ws_bytes,
                                   float* lohi, void* stream) {
  dp_range_shape s;
  if (!dp_range_shape_of(n, c, c_used, hw, &s)) return EGN_E_BADARG;
  if (s.parts == 0) return 0;
  if (!x || !ws || !lohi || ws_bytes < s.parts * 2 * (long)sizeof(float)) return EGN_E_BADARG;
  const int vec = hw % 4 == 0 && ((uintptr_t)x & 15u) == 0;
  hipLaunchKernelGGL(debug_range_partial_kernel, dim3((unsigned)s.parts), dim3(DP_THREADS), 0, (hipStream_t)stream, x,
                     c, c_used, hw, (int)s.chunks, (float*)ws, vec);
  hipLaunchKernelGGL(debug_range_fold_kernel, dim3(1), dim3(DP_THREADS), 0, (hipStream_t)stream, (const float*)ws,
                     (int)s.parts, lohi);
  egn_count_launches(2);
  return (int)hipGetLastError();
}

extern "C" int egn_debug_range_host_f32(const float* x, int n, int c, int c_used, int hw, float* lohi) {
  dp_range_shape s;
  if (!dp_range_shape_of(n, c, c_used, hw, &s)) return EGN_E_BADARG;
  if (s.parts == 0) return 0;
  if (!x || !lohi) return EGN_E_BADARG;
  float lo, hi;
  egn_dbg_range_init(lo, hi);
  for (int64_t row = 0; row < s.rows; ++row) {
    const float* p = x + ((size_t)(row / c_used) * (size_t)c + (size_t)(row % c_used)) * (size_t)hw;
    for (int e = 0; e < hw; ++e) egn_dbg_range_step(p[e], lo, hi);
  }
  egn_dbg_range_finish(lo, hi);
  lohi[0] = lo;
  lohi[1] = hi;
  return 0;
}

extern "C" int egn_debug_grid_u8(const float* img, int N, int C, int H, int W, int nrow, int pad, const float* lohi,
                                 uint8_t* out, long stride, void* stream) {
  egn_dbg_grid g;
  const int st = dp_grid_check(img, N, C, H, W, nrow, pad, lohi, out, stride, &g);
  if (st) return st < 0 ? st : 0;
  const int64_t items = (int64_t)g.gh * ((g.gw + DP_RUN - 1) / DP_RUN);
  const int64_t blocks = (items + DP_THREADS - 1) / DP_THREADS;
  if (blocks > 0x7fffffff) return EGN_E_BADARG;
  hipLaunchKernelGGL(debug_grid_kernel, dim3((unsigned)blocks), dim3(DP_THREADS), 0, (hipStream_t)stream, img, N, C, H,
                     W, pad, g, lohi, out, (int64_t)stride);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_debug_grid_host_u8(const float* img, int N, int C, int H, int W, int nrow, int pad,
                                      const float* lohi, uint8_t* out, long stride) {
  egn_dbg_grid g;
  const int st = dp_grid_check(img, N, C, H, W, nrow, pad, lohi, out, stride, &g);
  if (st) return st < 0 ? st : 0;
  const size_t plane = (size_t)H * (size_t)W;
  for (int Y = 0; Y < g.gh; ++Y) {
    uint8_t* row = out + (size_t)Y * (size_t)stride;
    for (int X = 0; X < g.gw; ++X) {
      int k, y, x;
      const bool in = egn_dbg_grid_source(g, N, H, W, pad, Y, X, &k, &y, &x);
      for (int ch = 0; ch < 3; ++ch)
        row[3 * (size_t)X + ch] =
            in ? (uint8_t)egn_dbg_quant_crop(img[((size_t)k * C + ch) * plane + (size_t)y * W + x], lohi[0], lohi[1]) : 0;
    }
  }
  return 0;
}

extern "C" int egn_debug_mosaic_u8(const float* img, int C, int H, int W, const float* maps, int n, int J, int h, int w,
                                   const float* lohi, const uint8_t* lut, uint8_t* out, long stride, void* stream) {
  const int st = dp_mosaic_check(img, C, H, W, maps, n, J, h, w, lohi, lut, out, stride);
  if (st) return st < 0 ? st : 0;
  dp_mosaic_plan pl;
  if (!dp_mosaic_plan_of(n, J, h, w, &pl)) return EGN_E_BADARG;
  const int vec = w % 4 == 0 && ((uintptr_t)maps & 15u) == 0;
  hipLaunchKernelGGL(debug_mosaic_kernel, dim3((unsigned)pl.blocks, (unsigned)pl.jz), dim3(DP_THREADS), 0,
                     (hipStream_t)stream, img, C, H, W, maps, J, h, w, pl, lohi, lut, out, (int64_t)stride, vec);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

extern "C" int egn_debug_mosaic_host_u8(const float* img, int C, int H, int W, const float* maps, int n, int J, int h,
                                        int w, const float* lohi, const uint8_t* lut, uint8_t* out, long stride) {
  const int st = dp_mosaic_check(img, C, H, W, maps, n, J, h, w, lohi, lut, out, stride);
  if (st) return st < 0 ? st : 0;
  const size_t plane = (size_t)H * (size_t)W;
  for (int i = 0; i < n; ++i)
    for (int y = 0; y < h; ++y) {
      uint8_t* row = out + ((size_t)i * h + y) * (size_t)stride;
      const egn_dbg_tap ty = egn_dbg_tap_of(y, H, h);
      for (int x = 0; x < w; ++x) {
        const egn_dbg_tap tx = egn_dbg_tap_of(x, W, w);
        for (int ch = 0; ch < 3; ++ch)
          row[3 * (size_t)x + ch] =
              (uint8_t)egn_dbg_thumb(img + ((size_t)i * C + ch) * plane, W, ty, tx, lohi[0], lohi[1]);
      }
      for (int j = 0; j < J; ++j) {
        const float* m = maps + (((size_t)i * J + j) * h + y) * (size_t)w;
        for (int x = 0; x < w; ++x) {
          const unsigned q = egn_dbg_quant_map(m[x]);
          for (int ch = 0; ch < 3; ++ch)
            row[3 * ((size_t)(j + 1) * w + x) + ch] = (uint8_t)egn_dbg_blend(lut[3 * q + ch], row[3 * (size_t)x + ch]);
        }
      }
    }
  return 0;
}
