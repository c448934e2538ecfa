// filter_pack.h -- the packed filter layouts of the conv kernels as code: per layout ONE function that maps a work-unit
// index to its stores, and the counts that size the buffers and the launches.  The layouts themselves are described in
// include/egonet_hip.h (egn_conv_config_kind: the kinds; the pack entries; egn_pack_conv_weights_batch_f32: the work
// units) and nowhere else.  Both packing kernels (filter_pack.hip) are loops over fp_unit.
// Reference: the weights of the Conv2d calls of libs/model/heatmapModel/hrnet.py:24-27 and of FCmodel.py's Linear layers.
#pragma once
#include "egn_internal.h"
#include "wino4_pack.h"

// One (weight, layout, direction) to pack: what egn_pack_conv_weights_batch_f32 reads from device memory (Python
// builds the table with a numpy dtype: size and field order are ABI).  `code` is the field the header lists as `dgrad`.
struct egn_pack_desc {
  const float* w;   // torch weight [Cout][Cin][taps]
  float* dst;
  int Cout, Cin, taps, code;
  long long begin;  // first work unit of this descriptor in the batch's enumeration
};
constexpr int FP_DGRAD = 1;   // code bits: the data-gradient filter (in / out channels swapped, taps rotated by 180 degrees)
constexpr int FP_WINO2 = 2;   //            the F(2x2,3x3) layout (kind 1)
constexpr int FP_WINO4 = 4;   //            the F(4x4,3x3) register-feed layout (kind 3); neither: direct (kind 0)

// floats one work unit stores
__host__ __device__ inline int fp_unit_floats(int code) { return code & FP_WINO4 ? 48 : (code & FP_WINO2 ? 64 : 4); }

// floats of the packed filter; 0: the layout does not take the shape
inline long long fp_floats(int code, int Cout, int Cin, int taps) {
  const int n_out = code & FP_DGRAD ? Cin : Cout, n_in = code & FP_DGRAD ? Cout : Cin;
  if (n_out <= 0 || n_in <= 0 || taps <= 0) return 0;
  if (code & FP_WINO4) return taps == 9 ? egn_wino4_weight_floats(n_out, n_in) : 0;
  if (code & FP_WINO2) return taps == 9 && egn_wino_cot(n_out) && n_in % EGN_CK == 0 ? (long long)n_out * n_in * 16 : 0;
  return (long long)((n_in + EGN_CK - 1) / EGN_CK) * taps * 4 * ((n_out + 15) & ~15) * 4;
}
inline long long fp_units(int code, int Cout, int Cin, int taps) {
  return fp_floats(code, Cout, Cin, taps) / fp_unit_floats(code);
}

// Direct layout: unit le = the float4 at (chunk, tap, quad, o).  `ld` = floats between the rows of w: Cin * taps for a
// conv weight, anything >= the row length for a matrix (taps 1: dgrad = its transposed use).
__device__ __forceinline__ void fp_direct_unit(const egn_pack_desc& d, long long le, int ld) {
  const int dg = d.code & FP_DGRAD;
  const int n_out = dg ? d.Cin : d.Cout, n_in = dg ? d.Cout : d.Cin;
  const int CoP = (n_out + 15) & ~15;
  const int o = (int)(le % CoP);
  long long r_ = le / CoP;
  const int quad = (int)(r_ % 4);
  r_ /= 4;
  const int tap = (int)(r_ % d.taps);
  const int chunk = (int)(r_ / d.taps);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (o < n_out) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = chunk * EGN_CK + quad * 4 + r;
      if (i < n_in)
        v[r] = dg ? d.w[(size_t)i * ld + (size_t)o * d.taps + (d.taps - 1 - tap)]
                  : d.w[(size_t)o * ld + (size_t)i * d.taps + tap];
    }
  }
  reinterpret_cast<float4*>(d.dst)[le] = make_float4(v[0], v[1], v[2], v[3]);
}

// F(2x2,3x3) layout: unit le = one (co-tile, chunk, quad, co) = 4 input channels x 16 frequencies of U = G g G^T
// (float64 arithmetic, one rounding to fp32) = 16 coalesced float4 stores.
__device__ __forceinline__ void fp_wino2_unit(const egn_pack_desc& d, long long le) {
  const int dg = d.code & FP_DGRAD;
  const int n_out = dg ? d.Cin : d.Cout, n_in = dg ? d.Cout : d.Cin;
  const int nchunk = n_in / EGN_CK;
  const int cot = egn_wino_cot(n_out);   // 48 or 32 output channels per co-tile (conv_wino.hip)
  const int col = (int)(le % cot);
  long long r_ = le / cot;
  const int quad = (int)(r_ % 4);
  r_ /= 4;
  const int chunk = (int)(r_ % nchunk);
  const int ct = (int)(r_ / nchunk);
  const int o = ct * cot + col;
  float u[16][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = chunk * EGN_CK + quad * 4 + r;
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        g[a][b] = dg ? (double)d.w[((size_t)i * d.Cin + o) * 9 + (2 - a) * 3 + (2 - b)]
                     : (double)d.w[((size_t)o * d.Cin + i) * 9 + a * 3 + b];
    double t[4][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      t[0][b] = g[0][b];
      t[1][b] = 0.5 * (g[0][b] + g[1][b] + g[2][b]);
      t[2][b] = 0.5 * (g[0][b] - g[1][b] + g[2][b]);
      t[3][b] = g[2][b];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      u[a * 4 + 0][r] = (float)t[a][0];
      u[a * 4 + 1][r] = (float)(0.5 * (t[a][0] + t[a][1] + t[a][2]));
      u[a * 4 + 2][r] = (float)(0.5 * (t[a][0] - t[a][1] + t[a][2]));
      u[a * 4 + 3][r] = (float)t[a][2];
    }
  }
  float4* slab = reinterpret_cast<float4*>(d.dst) + (size_t)(ct * nchunk + chunk) * (16 * 4 * cot);
#pragma unroll
  for (int f = 0; f < 16; ++f) slab[(f * 4 + quad) * cot + col] = make_float4(u[f][0], u[f][1], u[f][2], u[f][3]);
}

// F(4x4,3x3) register-feed layout: unit le = one (co, ci) pair = w4p_pack_pair's 36 stores.  A wavefront covers the
// 16 channels li x 4 input channels kq of one (co sub-tile, k-group): each of its store instructions fills one 1 KB
// block of the (co-tile, k-group, wave) slab.
__device__ __forceinline__ void fp_wino4_unit(const egn_pack_desc& d, long long le) {
  const int dg = d.code & FP_DGRAD;
  const int n_in = dg ? d.Cout : d.Cin;
  const int li = (int)(le & 15), kq = (int)((le >> 4) & 3);
  long long r_ = le >> 6;
  const int nt = (int)(r_ % 3);
  r_ /= 3;
  const int h = (int)(r_ % (n_in >> 2));
  const int ct = (int)(r_ / (n_in >> 2));
  w4p_pack_pair(d.w, d.Cin, dg, ct * W4P_CO + nt * 16 + li, 4 * h + kq, n_in, d.dst);
}

// unit le (< fp_units) of descriptor d
__device__ __forceinline__ void fp_unit(const egn_pack_desc& d, long long le, int ld) {
  if (d.code & FP_WINO4) fp_wino4_unit(d, le);
  else if (d.code & FP_WINO2) fp_wino2_unit(d, le);
  else fp_direct_unit(d, le, ld);
}
__device__ __forceinline__ void fp_unit(const egn_pack_desc& d, long long le) { fp_unit(d, le, d.Cin * d.taps); }
