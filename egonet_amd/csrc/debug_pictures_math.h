// debug_pictures_math.h -- the definition of the training debug pictures (debug_pictures.hip): the grid of crops and
// the heat-map mosaic of the reference's libs/visualization/debug.py, per pixel.  float64 where floats are needed and
// never contracted, clamps written as comparisons, so the kernels and the plain host loops execute the same IEEE
// operations and give the same bytes.  No HIP-only construct.  The pictures are pinned on THIS definition, not on
// cv2 / torchvision pixels.
//
// Range.  lo / hi = minimum / maximum over the first c_used channels of all crops, NaNs ignored (a comparison with a
//   NaN is false); -0 counts as +0; with no non-NaN value lo = hi = 0.  min / max are exact in any order.
// Crop value x -> grey level (both pictures):
//     s = 255 * ((double(x) - lo) / (double(hi) - lo + 1e-5));   q = s >= 0 ? trunc(s > 255 ? 255 : s) : 0
//   so a NaN s (x NaN, or inf / inf) gives 0.
// Grid.  xmaps = min(nrow, N), ymaps = ceil(N / xmaps); the picture is [ymaps (H + pad) + pad, xmaps (W + pad) + pad, 3];
//   crop k has its corner at row (k / xmaps)(H + pad) + pad, column (k % xmaps)(W + pad) + pad; every other pixel is 0.
// Thumbnail.  The quantised crop resized to w x h, bilinear on the uint8 values with half-pixel centres:
//     sx = double(W) / w;  x = (d + 0.5) sx - 0.5;  x0 = floor(x);  fx = x - x0;  columns x0 and x0 + 1 clamped to
//     [0, W - 1]; the same for rows;  with a b / c d the four grey levels (a = row y0, column x0):
//     top = a (1 - fx) + b fx;  bot = c (1 - fx) + d fx;  v = top (1 - fy) + bot fy;  out = floor(v + 0.5)
// Heat-map value m -> q = s >= 0 ? trunc(s > 255 ? 255 : s) : 0 with s = 255 double(m); colour = lut[q] (256 x 3 uint8
//   handed in as data); tile pixel = (7 colour + 3 thumbnail) / 10 per channel, integer division.
// Mosaic.  [n h, (J + 1) w, 3]: row block i is crop i, tile 0 the thumbnail, tile j + 1 joint j.
#pragma once
#include <math.h>
#include <stdint.h>
#include "pose_math.h"   // EGN_HD

// trunc(min(255, max(0, s))), 0 for a NaN
EGN_HD inline unsigned egn_dbg_level(double s) {
  if (!(s >= 0.0)) return 0u;
  return (unsigned)(s > 255.0 ? 255.0 : s);
}

EGN_HD inline unsigned egn_dbg_quant_crop(float x, float lo, float hi) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double v = ((double)x - (double)lo) / ((double)hi - (double)lo + 1e-5);
  return egn_dbg_level(255.0 * v);
}

EGN_HD inline unsigned egn_dbg_quant_map(float m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return egn_dbg_level(255.0 * (double)m);
}

// folding the range: a NaN never passes a comparison.  Partial results (a lane or block that saw nothing holds
// lo = +inf, hi = -inf) are folded per side, never through egn_dbg_range_step
EGN_HD inline float egn_dbg_min(float a, float b) { return b < a ? b : a; }
EGN_HD inline float egn_dbg_max(float a, float b) { return b > a ? b : a; }
EGN_HD inline void egn_dbg_range_step(float v, float& lo, float& hi) {
  lo = egn_dbg_min(lo, v);
  hi = egn_dbg_max(hi, v);
}
EGN_HD inline void egn_dbg_range_init(float& lo, float& hi) {
  lo = INFINITY;
  hi = -INFINITY;
}
// the stored pair: nothing seen -> 0 0; -0 -> +0
EGN_HD inline void egn_dbg_range_finish(float& lo, float& hi) {
  if (lo > hi) lo = hi = 0.0f;
  lo = lo + 0.0f;
  hi = hi + 0.0f;
}

struct egn_dbg_tap {   // one axis of the bilinear thumbnail: the two source indices and the weight of the second
  int i0, i1;
  double f;
};

EGN_HD inline egn_dbg_tap egn_dbg_tap_of(int d, int src, int dst) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double s = (double)src / (double)dst;
  const double x = ((double)d + 0.5) * s - 0.5;
  const double x0 = floor(x);
  egn_dbg_tap t;
  t.f = x - x0;
  // x lies in (-0.5, src): x0 in [-1, src - 1]
  const int i = (int)x0;
  t.i0 = i < 0 ? 0 : (i > src - 1 ? src - 1 : i);
  t.i1 = i + 1 < 0 ? 0 : (i + 1 > src - 1 ? src - 1 : i + 1);
  return t;
}

EGN_HD inline unsigned egn_dbg_bilinear(unsigned a, unsigned b, unsigned c, unsigned d, double fx, double fy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double top = (double)a * (1.0 - fx) + (double)b * fx;
  const double bot = (double)c * (1.0 - fx) + (double)d * fx;
  const double v = top * (1.0 - fy) + bot * fy;
  return (unsigned)floor(v + 0.5);
}

// one channel of thumbnail pixel (dy, dx) of a crop plane [H][W]
EGN_HD inline unsigned egn_dbg_thumb(const float* plane, int W, const egn_dbg_tap& ty, const egn_dbg_tap& tx, float lo,
                                     float hi) {
  const float* r0 = plane + (size_t)ty.i0 * (size_t)W;
  const float* r1 = plane + (size_t)ty.i1 * (size_t)W;
  return egn_dbg_bilinear(egn_dbg_quant_crop(r0[tx.i0], lo, hi), egn_dbg_quant_crop(r0[tx.i1], lo, hi),
                          egn_dbg_quant_crop(r1[tx.i0], lo, hi), egn_dbg_quant_crop(r1[tx.i1], lo, hi), tx.f, ty.f);
}

EGN_HD inline unsigned egn_dbg_blend(unsigned colour, unsigned thumb) { return (7u * colour + 3u * thumb) / 10u; }

// grid geometry; false = a size does not fit an int
struct egn_dbg_grid {
  int xmaps, ymaps, gh, gw;
};
EGN_HD inline bool egn_dbg_grid_of(int N, int H, int W, int nrow, int pad, egn_dbg_grid* g) {
  g->xmaps = nrow < N ? nrow : N;
  g->ymaps = (N + g->xmaps - 1) / g->xmaps;
  const int64_t gh = (int64_t)g->ymaps * ((int64_t)H + pad) + pad, gw = (int64_t)g->xmaps * ((int64_t)W + pad) + pad;
  if (gh > 0x7fffffff || gw > 0x7fffffff / 3) return false;
  g->gh = (int)gh;
  g->gw = (int)gw;
  return true;
}

// grid pixel (Y, X) -> crop k and its pixel (y, x); false = padding or an empty cell
EGN_HD inline bool egn_dbg_grid_source(const egn_dbg_grid& g, int N, int H, int W, int pad, int Y, int X, int* k, int* y,
                                       int* x) {
  if (Y < pad || X < pad) return false;
  const int r = (Y - pad) / (H + pad), yy = (Y - pad) % (H + pad);
  const int c = (X - pad) / (W + pad), xx = (X - pad) % (W + pad);
  if (yy >= H || xx >= W || r >= g.ymaps || c >= g.xmaps) return false;
  const int64_t kk = (int64_t)r * g.xmaps + c;
  if (kk >= N) return false;
  *k = (int)kk;
  *y = yy;
  *x = xx;
  return true;
}
