// softargmax_math.h -- the definition of the differentiable soft-arg-max of softargmax.hip: the per-map arithmetic and
// its order, shared by the kernels and the plain host loops (egn_softargmax_*_host_f32), so both execute the same IEEE
// float32 operations and give the same bits.  Nothing is contracted by the compiler (fp contract off); the fused
// multiply-adds are the explicit fmaf calls, single-rounded on either side.  exp is a polynomial written here -- the
// device's and the host's expf differ in the last bits.  No HIP-only construct.
//
// Operand.  Heat-maps as the training tape keeps them: padded NHWC [N, h, w, cs] float32, channels 0..K-1 live.
// Forward, per map (n, k), pixels p = y * w + x in row-major order:
//     m    = max_p z_p
//     e_p  = egn_sam_exp(z_p - m)                       (0 below -87: less than 2^-125 of the largest term)
//     se = sum e_p,  sx = sum e_p * x_p,  sy = sum e_p * y_p            (fmaf(e_p, x_p, sx))
//     ex = sx / se,  ey = sy / se;   coords = (ex / div_x, ey / div_y);  save = (ex, ey, m, se)
// Summation order.  S = egn_sam_slices(cs) partial sums per map: slice j takes the pixels j, j + S, j + 2S, ... in
//   increasing order, starting from 0 (max: from -inf).  The S partials are folded by the halving tree of
//   egn_sam_tree: for off = P/2, P/4, .., 1 (P = the power of two >= S): part[j] += part[j + off] for j < off where
//   j + off < S.  The total is part[0].  S depends on cs alone, so equal inputs give equal bits on any device.
// Backward, per pixel: s_p = e_p * (1 / se);  dz_p = s_p * fmaf(y_p - ey, gy / div_y, (x_p - ex) * (gx / div_x)).
#pragma once
#include <math.h>
#include <stdint.h>
#include "pose_math.h"   // EGN_HD

constexpr int EGN_SAM_THREADS = 1024;   // threads of a forward block: S slices x CW channels
constexpr int EGN_SAM_MAX_SLICES = 64;

// channels a block works on at once (all of them up to 1024), and the slices S the pixels of a map are dealt to
EGN_HD inline int egn_sam_chan_width(int cs) { return cs < EGN_SAM_THREADS ? cs : EGN_SAM_THREADS; }
EGN_HD inline int egn_sam_slices(int cs) {
  const int s = EGN_SAM_THREADS / egn_sam_chan_width(cs);
  return s > EGN_SAM_MAX_SLICES ? EGN_SAM_MAX_SLICES : s;
}
EGN_HD inline int egn_sam_tree_top(int S) {   // P / 2 of the header comment
  int p = 1;
  while (p < S) p <<= 1;
  return p >> 1;
}

// exp(x) for x <= 0 (x = z - max): Cody-Waite reduction x = n ln2 + r, |r| <= ln2 / 2 (+ rounding), the degree-5
// polynomial of Cephes' expf on r, scaled by 2^n through the exponent field.  Relative error < 2^-22.  NaN -> NaN.
EGN_HD inline float egn_sam_exp(float x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (x < -87.0f) return 0.0f;
  const float n = floorf(fmaf(x, 1.44269504088896341f, 0.5f));
  float r = fmaf(n, -0.693359375f, x);
  r = fmaf(n, 2.12194440e-4f, r);
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  p = fmaf(p, r * r, r) + 1.0f;
  if (!(n >= -126.0f)) return p;            // NaN in: NaN out (x >= -87 keeps n >= -126 otherwise)
  union {
    uint32_t u;
    float f;
  } s;
  s.u = (uint32_t)((int)n + 127) << 23;     // 2^n, n in -126..0
  return p * s.f;
}

struct egn_sam_sums {   // one slice's partial sums of a map
  float se, sx, sy;
};

EGN_HD inline float egn_sam_max(float a, float b) { return b > a ? b : a; }

EGN_HD inline void egn_sam_accum(egn_sam_sums& a, float z, float m, int x, int y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float e = egn_sam_exp(z - m);
  a.se = a.se + e;
  a.sx = fmaf(e, (float)x, a.sx);
  a.sy = fmaf(e, (float)y, a.sy);
}

EGN_HD inline void egn_sam_fold(egn_sam_sums& a, const egn_sam_sums& b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  a.se = a.se + b.se;
  a.sx = a.sx + b.sx;
  a.sy = a.sy + b.sy;
}

// coords[2] and save[4] of a map from its totals
EGN_HD inline void egn_sam_finish(const egn_sam_sums& t, float m, float div_x, float div_y, float* coords, float* save) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float ex = t.sx / t.se, ey = t.sy / t.se;
  coords[0] = ex / div_x;
  coords[1] = ey / div_y;
  save[0] = ex;
  save[1] = ey;
  save[2] = m;
  save[3] = t.se;
}

struct egn_sam_back {   // per map, from save and dcoords
  float ex, ey, m, inv, ax, ay;
};

EGN_HD inline egn_sam_back egn_sam_back_of(const float* save, const float* dcoords, float div_x, float div_y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  egn_sam_back b;
  b.ex = save[0];
  b.ey = save[1];
  b.m = save[2];
  b.inv = 1.0f / save[3];
  b.ax = dcoords[0] / div_x;
  b.ay = dcoords[1] / div_y;
  return b;
}

EGN_HD inline float egn_sam_dz(const egn_sam_back& b, float z, int x, int y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float s = egn_sam_exp(z - b.m) * b.inv;
  const float t = fmaf((float)y - b.ey, b.ay, ((float)x - b.ex) * b.ax);
  return s * t;
}
