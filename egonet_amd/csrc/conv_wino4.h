// conv_wino4.h -- what the F(4x4,3x3) kernel bodies share: w4_body in conv_wino4.hip (12 waves: 16 x 32 / 16 x 16 regions,
// four 8 x 8 images; one 48-channel co-tile per item), w4w_body in conv_wino4w_body.h (round 6: 96 output channels per
// item) and the two probe-only bodies w4h_body (conv_wino4h.hip) and w4r_body (conv_wino4r.hip).
// Geometry constants of the bank-conflict-free halo order, the raw-ISA load / LDS wrappers whose waits the kernels
// place themselves, the item order with the launchers' item set-up (w4_item_setup) and the kernels' item decode, the 1-D
// transforms, the input transform of a wave's third (V = B^T d B), and -- at the end -- the item pipeline: stamps, halo
// pieces, item prologue, the exchange round of the item end.
// Reference: the 3x3 stride-1 convolutions of libs/model/heatmapModel/hrnet.py:49-76.
#pragma once
#include <stdlib.h>

#include "conv_common.h"
#include "wino4_pack.h"

namespace {
constexpr int W4_NW = 12, W4_NTH = 64 * W4_NW;
constexpr int W4_CO = 48;
// Halo of the 16 x 32 region: 18 x 34 pixels x 8 channels, in 8-byte slots (one pixel, one channel PAIR) ordered
// [pair 0..3][x mod 4][y][x div 4 (pitch 10)]: the transform's lane (tile (ty, tx), channel kq of k-group g) reads
// pixel (4 ty + i, 4 tx + j) at slot (2 g + kq / 2) * 720 + 40 ty + tx + const(i, j), dword kq & 1.  ds_read_b32 is
// banked per 32-lane group on dword mod 32 (MI355X_MICROARCH.md): a group = 16 tiles x 2 channels of ONE pair plane,
// dword = 2 (40 ty + tx) + kq + const -> 32 different banks.  History (profiles/r3_wino4_ablations.txt,
// r3_pmc_sq_wino4.txt): pixel-major order put all 16 tiles of a group on one bank (the transform alone took 5 000
// cycles per stage); 16-byte quad planes left a 2-way conflict (SQ_LDS_BANK_CONFLICT 3.9 M cycles per launch).
// The loads fetch pixel-major (32 contiguous bytes per pixel) and each lane stores its two channel pairs.
template <int GEO>
struct W4G {
  static constexpr int ID = GEO;
  static constexpr int NIMG = GEO == 2 ? 4 : 1;         // images of a region (GEO 2: whole 8 x 8 maps)
  static constexpr int RH = GEO == 2 ? 10 : 18, RW = GEO == 0 ? 34 : (GEO == 2 ? 10 : 18);     // halo pixels of an image
  // load-element row pitch: a 16-lane store group = 8 (GEO 0) / 4 ALIGNED pixels of one row
  static constexpr int RWP = GEO == 0 ? 40 : (GEO == 2 ? 12 : 20);
  static constexpr int XD = GEO == 0 ? 10 : (GEO == 2 ? 3 : 5);      // slots per row and plane (x div 4: 0..8 / 0..4 / 0..2)
  // plane / pair pitches carry a bank skew for the halo STORES (ds_write_b64 is served in groups of 16 lanes: 8 pixels x
  // 2 quads, GEO 1 / 2: 4 pixels x 4 quads; without the skew the quads of a pixel fell on one bank: 2- / 4-way conflicts).
  // GEO 0: pixel x -> 8 (x & 3) + 2 (x >> 2) dwords, quad -> + 4: 32 banks.  GEO 1 / 2: pixel -> 2 (x & 3), quad -> 8 q.
  // GEO 3 (conv_wino4h.hip: GEO 1's region with GEO 0's 8-channel stages -- 8 pixels x 2 quads per store group): GEO 0's rule.
  // The transform's READS are per (i, j) and per pair plane: they only see XD and the image bases (bank-free as before).
  static constexpr int PLANE = GEO == 0 ? RH * XD : (GEO == 1 ? 97 : (GEO == 2 ? 145 : 100));     // 2 PLANE mod 32 = 8 / 2 / 2 / 8 dwords
  static constexpr int PAIR = GEO == 0 || GEO == 3 ? 4 * PLANE + 1 : (GEO == 1 ? 394 : 586);   // 8-byte slots per channel pair; 4 PAIR mod 32 = 4 / 8 / 8 / 4 dwords
  static constexpr int QPP = GEO == 1 || GEO == 2 ? 4 : 2;           // channel quads per pixel and stage (16 / 8 channels)
  static constexpr int NP = GEO == 2 ? 3 : 2;           // halo load pieces per wave and stage
  static constexpr int HSLOT = 2 * QPP * PAIR;          // 2884 / 3152 / 4688 / 1604 slots
  static constexpr int HBYTES = (GEO == 2 ? 38 : (GEO == 3 ? 13 : 26)) * 1024;   // halo slots + 1 KB parking for the idle load lanes (GEO 3: none)
  static constexpr int SBYTES = 16 * QPP;               // bytes of a pixel's channels of one stage
  static constexpr int NMT = GEO == 0 ? 2 : 1;          // m-tiles of a region
  static constexpr int NKK = GEO == 1 || GEO == 2 ? 2 : 1;           // k-groups multiplied per filter wait ("k-group pair")
  static constexpr int TWX = GEO == 0 ? 8 : (GEO == 2 ? 2 : 4);      // tiles per image row
  static constexpr int RGW = GEO == 0 ? 32 : (GEO == 2 ? 8 : 16);    // region width in pixels
  static constexpr int RGH = GEO == 2 ? 8 : 16;                      // region height
  static constexpr int VPT = GEO == 3 ? 512 : 1024;     // bytes of a frequency point in a V buffer ([k-groups of a stage][64 lanes] floats)
  // slot of image `img` inside a plane (GEO 2): 30 slots per image + a skew of 4 per image and 4 more per image PAIR, so
  // that the 16 tiles of a read group (img 0..3 x ty 0..1 (12 slots) x tx 0..1) fall on 16 different even dwords mod 32
  __host__ __device__ static constexpr int imgbase(int img) { return GEO == 2 ? 34 * img + 4 * (img >> 1) : 0; }
  // halo slot of lane tile `li` (pixel (0, 0) of the tile, x & 3 == 0 plane)
  __host__ __device__ static constexpr int tileslot(int li, int tw) {
    return GEO == 0 ? 4 * XD * (2 * (tw >> 1) + (li >> 3)) + (li & 7)
                    : (GEO == 2 ? imgbase(li >> 2) + 4 * XD * ((li >> 1) & 1) + (li & 1) : 4 * XD * (li >> 2) + (li & 3));
  }
};
// GEO 1 (tests/test_wino4_design_cpu.py): slot (4 XD ty + tx) -> dword 40 ty + 2 tx + (kq & 1): ty 0..3 -> banks
// +0, +8, +16, +24 -- 32 different banks per 32-lane group again.  GEO 2: slot imgbase(img) + 12 ty + tx -> dwords
// {0, 2, 24, 26} + {0, 68, 144, 212} mod 32 = {0, 4, 16, 20}: 16 different even banks.
constexpr int W4_VBYTES = 36 * 1024;                  // [pt][mt][g][lane] floats (GEO 1 / 2: [pt][g 0..3][lane])
constexpr int W4_V0 = 0, W4_V1 = W4_VBYTES, W4_H0 = 2 * W4_VBYTES;
template <int GEO>
constexpr int w4_lds_bytes() { return W4_H0 + 2 * W4G<GEO>::HBYTES; }      // 126 976 B (GEO 0 / 1), 151 552 B (GEO 2)
constexpr int W4_XBYTES = 36 * 3 * 1024;              // exchange [pt][nt][lane] float4: 110 592 B
static_assert(W4_XBYTES <= w4_lds_bytes<0>(), "the exchange reuses the stage buffers");
static_assert(W4G<0>::HSLOT * 8 + 1024 <= W4G<0>::HBYTES && W4G<1>::HSLOT * 8 + 1024 <= W4G<1>::HBYTES &&
                  W4G<2>::HSLOT * 8 + 1024 <= W4G<2>::HBYTES,
              "the halo and the parking slots of the idle load lanes fit the buffer");
static_assert(W4G<0>::QPP * W4G<0>::RH * W4G<0>::RWP <= W4G<0>::NP * W4_NW * 64 &&
                  W4G<1>::QPP * W4G<1>::RH * W4G<1>::RWP <= W4G<1>::NP * W4_NW * 64 &&
                  W4G<2>::QPP * W4G<2>::NIMG * W4G<2>::RH * W4G<2>::RWP <= W4G<2>::NP * W4_NW * 64,
              "the load pieces of the waves cover the halo");
static_assert(W4G<2>::imgbase(3) + W4G<2>::RH * W4G<2>::XD <= W4G<2>::PLANE && w4_lds_bytes<2>() + 12 * 96 * 8 <= EGN_BIG_LDS_BYTES,
              "GEO 2: four images fit a plane, the buffers fit the CU");
constexpr int W4_UKG = W4_NW * 3 * 64 * 4;            // filter floats of one (co-tile, stage, k-group): 9216 (9 of 12 used)
static_assert(W4_UKG == W4P_UKG && W4_CO == W4P_CO, "wino4_pack.h packs this kernel's layout");
constexpr unsigned W4_PAST = 0x80000000u;             // scalar byte offset past every buffer (tensors stay below 2 GB)
}  // namespace

// one LDS dword at a VGPR byte address + immediate (see conv_wgrad_wino.hip: the compiler's ds_read2 pairing
// costs a v_add per pair); the values are tied to w4_landed's s_waitcnt before use
template <int OFF>
__device__ __forceinline__ float w4_lds(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read_b32 immediate");
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void w4_landed6(float (&a)[6], float (&b)[6]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(b[0]), "+v"(b[1]),
                 "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]));
}
__device__ __forceinline__ void w4_tie6(float (&a)[6]) {
  asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]));
}
// filter loads: dwordx4 (a burst of 20 single-dword loads per wave and stage cost every wave ~1 000 cycles of
// issue time behind the barrier, profiles/r3_wino4_timeline_v1.txt)
template <int OFF>
__device__ __forceinline__ f32x4 w4_gld4(u32x4 rsrc, unsigned voff, unsigned soff) {
  static_assert(OFF >= 0 && OFF < 4096, "the immediate offset of a buffer instruction has 12 bits (the assembler truncates silently)");
  f32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(v) : "v"(voff), "s"(rsrc), "s"(soff), "n"(OFF));
  return v;
}
template <int N>
__device__ __forceinline__ void w4_vm_landed3(f32x4 (&b)[3]) {
  asm volatile("s_waitcnt vmcnt(%3)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]) : "n"(N));
}
template <int N>
__device__ __forceinline__ void w4_vm_landed2(f32x4 (&h)[2]) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(h[0]), "+v"(h[1]) : "n"(N));
}
__device__ __forceinline__ void w4_vm_landedH(f32x4 (&h)[2]) { w4_vm_landed2<0>(h); }
__device__ __forceinline__ void w4_vm_landedH(f32x4 (&h)[3]) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]));
}
// the filter registers of a wait group (one k-group: 3 dwordx4; GEO 1's k-group pair: 6), tied to the s_waitcnt
// (every vector-memory wait of these kernels is vmcnt(0): the note in front of conv_wino4.hip's W4_STAGE)
__device__ __forceinline__ void w4_vm_landedB(f32x4 (&b)[1][3]) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[0][2]));
}
__device__ __forceinline__ void w4_vm_landedB(f32x4 (&b)[2][3]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[0][2]), "+v"(b[1][0]), "+v"(b[1][1]), "+v"(b[1][2]));
}
// The 9-of-12 form of a k-group's filter registers (w4w_body, w4h_body, w4r_body: 18 registers per buffer instead of 24,
// the budget): two slices of wino4_pack.h's layout -- the two co-tiles of a wide item, or the two 12-wave slices of a
// six-point wave -- each the 9 used values p = 3 pl + nt of the 12 per (wave, lane) slot, values 0 .. 7 as two dwordx4,
// value 8 as one dword.  Each body maps its (point, co sub-tile) onto (slice, p) in its own *_bval.
struct W4B9 {
  f32x4 q[4];       // [2 slice + (p >> 2)][p & 3], p < 8
  float s[2];       // value 8 of the slice
  __device__ __forceinline__ float val(int slice, int p) const { return p < 8 ? q[2 * slice + (p >> 2)][p & 3] : s[slice]; }
};
__device__ __forceinline__ void w4_vm_landedB(W4B9& b) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(b.q[0]), "+v"(b.q[1]), "+v"(b.q[2]), "+v"(b.q[3]), "+v"(b.s[0]), "+v"(b.s[1]));
}
template <int OFF>
__device__ __forceinline__ float w4_gld1(u32x4 rsrc, unsigned voff, unsigned soff) {
  static_assert(OFF >= 0 && OFF < 4096, "12-bit immediate");
  float v;
  asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:%4" : "=v"(v) : "v"(voff), "s"(rsrc), "s"(soff), "n"(OFF));
  return v;
}
// so: byte offset of the k-group's first slice (W4_PAST = none), the second one `stride` bytes behind it (a scalar offset:
// the immediate of a buffer instruction has 12 bits)
__device__ __forceinline__ void w4_loadB(W4B9& b, u32x4 ruv, unsigned uvo, unsigned so, unsigned stride) {
  const unsigned so1 = so + stride;
  b.q[0] = w4_gld4<0>(ruv, uvo, so); b.q[1] = w4_gld4<1024>(ruv, uvo, so); b.s[0] = w4_gld1<2048>(ruv, uvo, so);
  b.q[2] = w4_gld4<0>(ruv, uvo, so1); b.q[3] = w4_gld4<1024>(ruv, uvo, so1); b.s[1] = w4_gld1<2048>(ruv, uvo, so1);
}
template <int OFF>
__device__ __forceinline__ void w4_xwr(unsigned addr, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void w4_xwr2(unsigned addr, float a, float b) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {a, b};
  asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}
// frequency point PT of the exchange, XPT bytes per point (the immediates reach 18 points: xr1 = xr0 + 18 XPT)
template <int PT, int XPT>
__device__ __forceinline__ float w4_xrd(unsigned xr0, unsigned xr1) {
  if constexpr (PT < 18) return w4_lds<PT * XPT>(xr0);
  else return w4_lds<(PT - 18) * XPT>(xr1);
}

// Item order: what the XCD of a block (block index mod 8 -- blocks w, w + 8, ... stay on one XCD; a matter of speed only)
// owns.  The transformed filter is 36 x 4 bytes per (ci, co): 21 MB at 384 -> 384 channels, 5.3 MB at 192 -> 192 -- more
// than an XCD's 4 MB of L2, and a layer's filter arrives cold from HBM.
//   0  regions: 8 consecutive regions on the 8 XCDs, every XCD streams the WHOLE filter (small filters: 48 / 96 channels);
//   1  nct in {2, 4} (from W4_COX_MIN_NCT up): co-tile = xcd % nct, the XCD takes every (8 / nct)-th (region, half);
//   2  nct a multiple of 8: co-tile = 8 j + xcd -- each XCD reads its share of the filter once and keeps it, and reads
//      the halos of all regions instead (6 MB per 64 images at 384 channels).
// Measured on the 64-crop network (profiles/r4_wino4c.txt): 384 -> 384 @ 8 x 8 with regions on the XCDs 13.60 ms per
// batch, with co-tiles on them 13.17 ms.
#ifndef W4_COX_MIN_NCT
#define W4_COX_MIN_NCT 4
#endif
__host__ __device__ inline int w4_item_mode(int nct) {
#ifdef W4_NO_COTILE_XCD
  return 0;
#else
  if ((nct & 7) == 0) return 2;
  return nct >= W4_COX_MIN_NCT && (nct == 2 || nct == 4) ? 1 : 0;
#endif
}
__host__ __device__ inline int w4_item_count(int mode, int nreg, int nct, int ks) {
  if (mode == 2) return nreg * nct * ks;
  if (mode == 1) return 8 * ((nreg * ks + 8 / nct - 1) / (8 / nct));
  return ((nreg + 7) >> 3) * nct * ks * 8;
}
// Host: the item set-up of a launcher (a: planned) for nreg regions x nct co-tiles (wide items: co-tile pairs) x ks K
// halves.  Sets the multipliers of the kernels' item index divisions -- one multiply-high each, exact while x * d < 2^32
// (x = the dividend's range) -- and returns the item count, or EGN_E_BADARG where a division would not be exact.
static inline int w4_item_setup(ConvArgs& a, int nct, int ks, int nreg) {
  const int nck = nct * ks, imode = w4_item_mode(nct);
  const int nwork = w4_item_count(imode, nreg, nct, ks);
  if ((unsigned long long)nwork * (unsigned)(8 * nck) >= 0x100000000ull ||
      (unsigned long long)(nreg + 8) * (unsigned)(a.tiles_x * a.tiles_y) >= 0x100000000ull)
    return EGN_E_BADARG;
  a.mg_nct = imode == 1 ? 0u : egn_magic_u32(imode == 2 ? nct / 8 : nck);
  a.mg_txy = egn_magic_u32(a.tiles_x * a.tiles_y);
  a.mg_tx = egn_magic_u32(a.tiles_x);
  return nwork;
}

// Device: item WI -> (region REG, co-tile CT, K half KH), declared here, for the three item modes.  NCT counts what the
// XCDs share out (wide items: co-tile pairs); a.mg_nct is w4_item_setup's multiplier (of NCT * KS in mode 0, of NCT / 8 in
// mode 2; KS is a power of two).  REG >= the region count: (uniform) padding of the last round of the XCDs.
// (A macro -- see "the item pipeline" at the end of this file; uses the body's `a` and `imode`.)
#define W4_ITEM_DECODE(WI, KS, NCT, REG, CT, KH)                                                    \
  int REG, CT, KH;                                                                                   \
  {                                                                                                  \
    const unsigned xq = (WI) & 7u, q_ = (WI) >> 3;                                                   \
    const unsigned qq = egn_udiv_magic(q_, a.mg_nct);                                                \
    if (imode == 0) {                                                                                \
      const int cs_ = (int)(q_ - qq * (unsigned)((NCT) * (KS)));                                     \
      REG = (int)(qq * 8u + xq); CT = cs_ / (KS); KH = cs_ % (KS);                                   \
    } else if (imode == 1) {                                                                         \
      const unsigned lg = (unsigned)(NCT) >> 1;          /* log2 of 2 / 4 */                         \
      const int cs_ = (int)(q_ * (8u >> lg) + (xq >> lg));                                           \
      REG = cs_ / (KS); CT = (int)(xq & ((unsigned)(NCT) - 1u)); KH = cs_ % (KS);                    \
    } else {                                                                                         \
      REG = (int)qq / (KS); CT = (int)((q_ - qq * ((unsigned)(NCT) >> 3)) * 8u + xq); KH = (int)qq % (KS); \
    }                                                                                                \
  }
// region -> (first image, top row, left column) of its output pixels through the magic divisions of w4_item_setup
// (GEO 2: the region is the four images n .. n + 3)
struct W4Region { int n, y0, x0; };
template <int GEO>
__device__ __forceinline__ W4Region w4_item_region(const ConvArgs& a, int reg, int regs_x, int regs_xy) {
  typedef W4G<GEO> Q;
  const unsigned n_ = egn_udiv_magic((unsigned)reg, a.mg_txy);
  const unsigned r_ = (unsigned)reg - n_ * (unsigned)regs_xy;
  const unsigned ry_ = egn_udiv_magic(r_, a.mg_tx);
  return W4Region{(int)n_ * Q::NIMG, (int)ry_ * Q::RGH, (int)(r_ - ry_ * (unsigned)regs_x) * Q::RGW};
}

// 1-D input transform of six values (12 instructions)
__device__ __forceinline__ void w4_bt(const float (&t)[6], float (&o)[6]) {
  o[0] = __builtin_fmaf(4.f, t[0], __builtin_fmaf(-5.f, t[2], t[4]));
  const float u = __builtin_fmaf(-4.f, t[2], t[4]), v = __builtin_fmaf(-4.f, t[1], t[3]);
  o[1] = u + v;
  o[2] = u - v;
  const float p = t[4] - t[2], q = t[3] - t[1];
  o[3] = __builtin_fmaf(2.f, q, p);
  o[4] = __builtin_fmaf(-2.f, q, p);
  o[5] = __builtin_fmaf(4.f, t[1], __builtin_fmaf(-5.f, t[3], t[5]));
}
// 1-D output transform of six values (10 instructions)
__device__ __forceinline__ void w4_at(const float (&m)[6], float (&y)[4]) {
  const float p = m[1] + m[2], q = m[1] - m[2], r = m[3] + m[4], s = m[3] - m[4];
  y[0] = m[0] + p + r;
  y[1] = __builtin_fmaf(2.f, s, q);
  y[2] = __builtin_fmaf(4.f, r, p);
  y[3] = __builtin_fmaf(8.f, s, q) + m[5];
}

// halo of stage parity P -> V, for this wave's (m-tile, k-group) share and its THIRD of the frequency rows:
// PART 0 rows {0, 5}, 1 rows {1, 2}, 2 rows {3, 4} -- 48 VALU instructions, 36 / 24 / 24 LDS reads, 12 writes each.
// hb0: per-lane byte base in halo buffer 0 (the immediates reach both buffers); vw0: base in THIS parity's V buffer.
template <int P, int PART, int GEO>
__device__ __forceinline__ void w4_transform(unsigned hb0, unsigned vw0) {
  typedef W4G<GEO> Q;
  static_assert(Q::HBYTES + (3 * Q::PLANE + 5 * Q::XD + 1) * 8 < 65536, "halo immediates");
  constexpr int HO = P ? Q::HBYTES : 0;
#define W4_D(I, J) w4_lds<HO + (((J) & 3) * Q::PLANE + (I)*Q::XD + ((J) >> 2)) * 8>(hb0)
#define W4_WR(PT, VAL) asm volatile("ds_write_b32 %0, %1 offset:%2" : : "v"(vw0), "v"(VAL), "n"((PT)*Q::VPT) : "memory")
#define W4_ROW(FI, O)                                                                                   \
  W4_WR((FI)*6 + 0, (O)[0]); W4_WR((FI)*6 + 1, (O)[1]); W4_WR((FI)*6 + 2, (O)[2]);                      \
  W4_WR((FI)*6 + 3, (O)[3]); W4_WR((FI)*6 + 4, (O)[4]); W4_WR((FI)*6 + 5, (O)[5]);
#define W4_RD6(DST, I)                                                                                  \
  DST[0] = W4_D(I, 0); DST[1] = W4_D(I, 1); DST[2] = W4_D(I, 2); DST[3] = W4_D(I, 3); DST[4] = W4_D(I, 4); DST[5] = W4_D(I, 5);
  if constexpr (PART == 0) {
    // row 0: T = 4 d0 - 5 d2 + d4; row 5: T = 4 d1 - 5 d3 + d5
    {
      float x[6], y[6], z[6], t[6], o[6];
      W4_RD6(x, 0) W4_RD6(y, 2) W4_RD6(z, 4)
      w4_landed6(x, y);
      w4_tie6(z);
#pragma unroll
      for (int j = 0; j < 6; ++j) t[j] = __builtin_fmaf(4.f, x[j], __builtin_fmaf(-5.f, y[j], z[j]));
      w4_bt(t, o);
      W4_ROW(0, o)
    }
    {
      float x[6], y[6], z[6], t[6], o[6];
      W4_RD6(x, 1) W4_RD6(y, 3) W4_RD6(z, 5)
      w4_landed6(x, y);
      w4_tie6(z);
#pragma unroll
      for (int j = 0; j < 6; ++j) t[j] = __builtin_fmaf(4.f, x[j], __builtin_fmaf(-5.f, y[j], z[j]));
      w4_bt(t, o);
      W4_ROW(5, o)
    }
  } else {
    float d1[6], d2[6], d3[6], d4[6], ta[6], tb[6], o[6];
    W4_RD6(d1, 1) W4_RD6(d2, 2) W4_RD6(d3, 3) W4_RD6(d4, 4)
    w4_landed6(d1, d2);
    w4_tie6(d3);
    w4_tie6(d4);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      if constexpr (PART == 1) {        // rows 1, 2: u = d4 - 4 d2, v = d3 - 4 d1
        const float u = __builtin_fmaf(-4.f, d2[j], d4[j]), v = __builtin_fmaf(-4.f, d1[j], d3[j]);
        ta[j] = u + v;
        tb[j] = u - v;
      } else {                          // rows 3, 4: p = d4 - d2, q = d3 - d1
        const float p = d4[j] - d2[j], q = d3[j] - d1[j];
        ta[j] = __builtin_fmaf(2.f, q, p);
        tb[j] = __builtin_fmaf(-2.f, q, p);
      }
    }
    w4_bt(ta, o);
    if constexpr (PART == 1) { W4_ROW(1, o) } else { W4_ROW(3, o) }
    w4_bt(tb, o);
    if constexpr (PART == 1) { W4_ROW(2, o) } else { W4_ROW(4, o) }
  }
#undef W4_RD6
#undef W4_D
#undef W4_WR
#undef W4_ROW
}
// ---------------------------------------------------------------------------------------------------------------------
// The item pipeline the four bodies share.  A body owns its accumulators with W4_MUL6 / W4_MUL, its filter loads' W4_LOADB,
// the k-groups per stage in W4_STAGE and what only it has (w4_body: K split, tickets, ST statistics, ablations, several
// images per region; w4h_body: the LDS-counter barriers and its exchange units; w4r_body: the row pass before the
// exchange).  What follows is a macro where a function did not reproduce the kernels' instruction stream (the compiler
// simplifies and unrolls a function on its own, before it is inlined and sees the ranges of the body's values:
// profiles/w4_body_isa.txt).  The macros use the bodies' common names: a, ABL, Q (the body's W4G), C, lane, wave, tpart, S,
// s_ (the stage of W4_STAGE), rxv, doff, hreg, hws, hb0, vw0, and in the item end rr, ry, vo, sc, sh, rv, yc, xr0, act_lo,
// rowpitch, colpitch.

// ---- stamps (ABL & 64, tools/wino4_clk.py): s_memtime of every wave at the points W4_CLK() marks, NTK per wave in the
// LDS at byte OFF (above what the body uses), dumped into `res` at the end ([block][HDR + waves x NTK] u64, word 0: the
// stamps a wave took).  WAVE: the wave's index in the workgroup.
#define W4_STAMPS(NTK, OFF, WAVE)                                                                                      \
  constexpr int W4_NTK = (NTK);                                                                                        \
  unsigned long long* sT = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(w4_smem) + (OFF));            \
  const int stw = (WAVE);                                                                                              \
  int ntk = 0;
#define W4_CLK()                                                                        \
  {                                                                                     \
    if constexpr ((ABL & 64) != 0) {                                                    \
      if (lane == 0 && ntk < W4_NTK) sT[stw * W4_NTK + ntk] = __builtin_readcyclecounter(); \
      ++ntk;                                                                            \
    }                                                                                   \
  }
template <int NWAVES, int NTK, int HDR>
__device__ __forceinline__ unsigned long long* w4_stamp_dump(const ConvArgs& a, const unsigned long long* sT, int ntk, int tid) {
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(const_cast<float*>(a.res)) + (size_t)blockIdx.x * (NWAVES * NTK + HDR);
  for (int e = tid; e < NWAVES * NTK; e += NWAVES * 64) out[HDR + e] = sT[e];
  if (tid == 0) out[0] = (unsigned long long)ntk;
  return out;
}

// ---- halo pieces.  A wave of NW loads pieces wave, wave + NW (, wave + 2 NW) of a stage; element e -> (pixel e / QPP,
// channel quad e % QPP), pixel-major with the rows padded to whole store groups (hya: GEO 2's images follow each other).
// LOAD order pixel-major, the channel quads of a pixel in neighbouring lanes (32 / 64 contiguous bytes: 32 or 16 cache
// lines per instruction instead of 64); the lane stores its 16 bytes to the pixel's slots of the bank-conflict-free order:
// channels 4 hq, 4 hq + 1 -> pair plane 2 hq, channels 4 hq + 2, + 3 -> pair plane 2 hq + 1.
#define W4_HALO_ELEM(NW, K, LANE)                                   \
  const int e = (wave + (NW) * (K)) * 64 + (LANE);                    \
  const int px = e / Q::QPP, hq = e % Q::QPP;                        \
  const int hya = px / Q::RWP, hx = px - hya * Q::RWP;
// LDS addresses `hws` of a wave's pieces, two variants (H0: byte offset of halo buffer 0).
// Parked (w4_body, w4r_body): lanes past the last pixel park their zeros in the unused tail of the buffer (1 KB); two
// address registers per piece.  Each of the two bodies fills them in its own loop: w4_body splits the rows into the images
// of a region and keeps hyx / hrel beside the slots, and neither form compiles to the other's instructions.
template <int NP>
struct W4HaloParked { unsigned a[NP], b[NP]; };
// Natural (GEO 1 / 3): every lane stores to the NATURAL slot of its element -- the padded columns 18 / 19 of a row fall
// on slots (x & 3) in {2, 3}, x >> 2 = 4 and the rows 18 / 19 past the halo on the slots behind row 17 of a plane; the
// transform reads none of them (rows 0 .. 17 x (x >> 2) 0 .. 4 of the planes of x = 0 .. 17), so the idle lanes need no
// parking area and the second channel pair of a lane sits at a constant + PAIR slots: one address register per piece.
template <int NP>
struct W4HaloNatural { unsigned a[NP]; };
#define W4_HALO_SLOTS_NATURAL(NW, H0)                                                                                  \
  static_assert(Q::NIMG == 1 && Q::NP * (NW) * 64 <= Q::QPP * (19 * Q::RWP + 4) && Q::RH * Q::XD + 5 < Q::PLANE &&     \
                    (2 * Q::QPP - 1) * Q::PAIR + 3 * Q::PLANE + 19 * Q::XD + 5 <= Q::HSLOT && Q::HSLOT * 8 <= Q::HBYTES, \
                "natural slots of the idle lanes (the last element: row 19, column 3)");                               \
  W4HaloNatural<Q::NP> hws;                                                                                            \
  _Pragma("unroll") for (int k = 0; k < Q::NP; ++k) {                                                                  \
    W4_HALO_ELEM(NW, k, lane)                                                                                          \
    const int slot = 2 * hq * Q::PAIR + (hx & 3) * Q::PLANE + hya * Q::XD + (hx >> 2);                                 \
    hws.a[k] = lds0 + (unsigned)((H0) + slot * 8);                                                                     \
  }
// piece k of the wave into the halo buffer at byte OFF (PAIRB: the bytes between a quad's two channel pairs)
template <int OFF, int PAIRB, int NP>
__device__ __forceinline__ void w4_hstore(const W4HaloParked<NP>& h, int k, const f32x4& v) {
  w4_xwr2<OFF>(h.a[k], v[0], v[1]);
  w4_xwr2<OFF>(h.b[k], v[2], v[3]);
}
template <int OFF, int PAIRB, int NP>
__device__ __forceinline__ void w4_hstore(const W4HaloNatural<NP>& h, int k, const f32x4& v) {
  w4_xwr2<OFF>(h.a[k], v[0], v[1]);
  w4_xwr2<OFF + PAIRB>(h.a[k], v[2], v[3]);
}
// The halo goes through REGISTERS (buffer_load_dwordx4 -> ds_write_b64), not LDS-DMA, and every vector-memory wait is
// vmcnt(0): see the note in front of conv_wino4.hip's W4_STAGE.
#define W4_HLOAD(K, STAGE) /* piece K of this wave; STAGE: byte offset of the stage's channels, W4_PAST = none */ \
  if constexpr ((ABL & 16) == 0) hreg[K] = w4_gld4<0>(rxv, doff.v[K], (unsigned)(STAGE));                        \
  else hreg[K] = f32x4{1.f, 2.f, 3.f, (float)lane};
#define W4_HLOADS(STAGE) W4_HLOAD(0, STAGE) W4_HLOAD(1, STAGE) if constexpr (Q::NP == 3) { W4_HLOAD(Q::NP - 1, STAGE) }
#define W4_HSTORE(P) \
  { _Pragma("unroll") for (int k_ = 0; k_ < Q::NP; ++k_) w4_hstore<(P)*Q::HBYTES, Q::PAIR * 8>(hws, k_, hreg[k_]); }
// halo offsets `doff` of an item (stage 0): zero padding by OOB offsets.  W4_HALO_DOFF (one image per region; n, y0, x0:
// the item's) recomputes them from an opaque copy of the lane id per item (not kept over the K loop: registers)
template <int NP>
struct W4HaloOffs { unsigned v[NP]; };
#define W4_HALO_DOFF(NW)                                                                                               \
  W4HaloOffs<Q::NP> doff;                                                                                              \
  {                                                                                                                    \
    int lane_t = lane;                                                                                                 \
    asm volatile("" : "+v"(lane_t));                                                                                   \
    const int base = ((n * a.H + (y0 - 1)) * a.W + (x0 - 1)) * C * 4;                                                  \
    _Pragma("unroll") for (int k = 0; k < Q::NP; ++k) {                                                                \
      W4_HALO_ELEM(NW, k, lane_t)                                                                                      \
      const int hy = hya;                                                                                              \
      const unsigned iy = (unsigned)(y0 - 1 + hy), ix = (unsigned)(x0 - 1 + hx);                                       \
      const bool in = hy < Q::RH && hx < Q::RW && iy < (unsigned)a.H && ix < (unsigned)a.W;                            \
      doff.v[k] = in ? (unsigned)(base + ((hy * a.W + hx) * C + 4 * hq) * 4) : EGN_OOB;                                \
    }                                                                                                                  \
  }

// ---- item prologue, item top -> K loop starts: stage 0's pieces and the first filter wait group (LOADB0) are issued,
// the pieces go to LDS, stage 1's fly during the first transform and follow it.  BAR: the body's barrier.
#define W4_PROLOGUE(LOADB0, BAR)                                                                                       \
  W4_HLOADS(0u)                                                                                                        \
  LOADB0                                                                                                               \
  W4_CLK() /* item top: halo + filter loads issued */                                                                  \
  w4_vm_landedH(hreg); /* stage 0's pieces (and the first filter wait group) */                                        \
  W4_HSTORE(0)                                                                                                         \
  W4_HLOADS((unsigned)Q::SBYTES) /* stage 1's pieces fly during the first transform */                                 \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                   \
  W4_CLK() /* own pieces of stage 0 in LDS */                                                                          \
  BAR                                                                                                                  \
  W4_CLK() /* everyone's */                                                                                            \
  asm volatile("" ::: "memory");                                                                                       \
  if constexpr ((ABL & 1) == 0) {                                                                                      \
    if (tpart == 0) w4_transform<0, 0, Q::ID>(hb0, vw0);                                                               \
    else if (tpart == 1) w4_transform<0, 1, Q::ID>(hb0, vw0);                                                          \
    else w4_transform<0, 2, Q::ID>(hb0, vw0);                                                                          \
  }                                                                                                                    \
  asm volatile("" ::: "memory");                                                                                       \
  /* this wave's pieces of stage 1 (and the filter loads before them) have landed: into LDS with them -- the first  */ \
  /* third transforms stage 1 right behind the barrier */                                                              \
  w4_vm_landedH(hreg);                                                                                                 \
  W4_HSTORE(1)                                                                                                         \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                   \
  W4_CLK() /* stage 0 transformed */                                                                                   \
  BAR                                                                                                                  \
  asm volatile("" ::: "memory");                                                                                       \
  W4_CLK() /* K loop starts */
// The transform of stage s + 1 sits at a different point of the stage for each third of the waves (two of a SIMD's three
// waves always have MFMAs to issue), each a point where only ONE filter buffer is live.  Raised priority: at equal
// priority the SIMD's arbiter hands the transforming wave one VALU issue per MFMA of the two multiplying waves -- 48
// instructions took 1 500-2 000 cycles (profiles/r3_wino4_timeline_v2.txt).  (36 VPT: the bytes of a V buffer.)
#define W4_TRANS(P, PART)                                                                                      \
  if ((ABL & 1) == 0 && s_ + 1 < S && tpart == (PART)) {                                                       \
    __builtin_amdgcn_s_setprio(3);                                                                             \
    w4_transform<1 - (P), PART, Q::ID>(hb0, vw0 + (unsigned)((1 - (P)) * 36 * Q::VPT));                        \
    __builtin_amdgcn_s_setprio(0);                                                                             \
  }

// ---- item end: a round takes a C fragment per (point, co sub-tile) through the exchange so that every lane gets all 36
// points of ONE (tile, co).  Exchange [point][co sub-tile][writer lane] float4 (the C fragment: tiles 4 kq_w .. + 3 of
// channel li_w).  The reader takes ONE dword of 16 writer slots (li = 0..15): a stride of 4 dwords puts li and li + 8 on
// one bank (2-way conflict on all 36 reads of a round).  So writers with li >= 8 store their float4 rotated by two dwords
// (two ds_write_b64 with swapped offsets -- no extra instruction: xwa = slot + 8 (li >> 3), xwb = slot + 8 - 8 (li >> 3)),
// and the reader looks at dword (kq + 2 (li >> 3)) & 3.
template <int OFF>
__device__ __forceinline__ void w4_xw(unsigned xwa, unsigned xwb, const f32x4& v) {
  w4_xwr2<OFF>(xwa, v[0], v[1]);
  w4_xwr2<OFF>(xwb, v[2], v[3]);
}
// the residual of the lane's 4 x 4 output pixels into RV (VO: the lane's byte offset, EGN_OOB = none); uses rr, rowpitch,
// colpitch
#define W4_RES_LOAD(RV, VO)                                                                                            \
  _Pragma("unroll") for (int oa = 0; oa < 4; ++oa) _Pragma("unroll") for (int ob = 0; ob < 4; ++ob)                    \
      RV[oa][ob] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, VO, oa * rowpitch + ob * colpitch, 0));
// exchange read (reader address xr0, XPT bytes per point) with the column pass into yc: M[i][j] = X[6 i + j], two columns
// per batch (12 reads), column pass A^T right away: 24 values stay
#define W4_COLS(J0, XPT)                                                                                \
  {                                                                                                     \
    float ca_[6], cb_[6], ya_[4], yb_[4];                                                               \
    ca_[0] = W4_M(0, J0, XPT); ca_[1] = W4_M(1, J0, XPT); ca_[2] = W4_M(2, J0, XPT); ca_[3] = W4_M(3, J0, XPT);     \
    ca_[4] = W4_M(4, J0, XPT); ca_[5] = W4_M(5, J0, XPT);                                               \
    cb_[0] = W4_M(0, J0 + 1, XPT); cb_[1] = W4_M(1, J0 + 1, XPT); cb_[2] = W4_M(2, J0 + 1, XPT);        \
    cb_[3] = W4_M(3, J0 + 1, XPT); cb_[4] = W4_M(4, J0 + 1, XPT); cb_[5] = W4_M(5, J0 + 1, XPT);        \
    w4_landed6(ca_, cb_);                                                                               \
    w4_at(ca_, ya_);                                                                                    \
    w4_at(cb_, yb_);                                                                                    \
    _Pragma("unroll") for (int oa = 0; oa < 4; ++oa) { yc[oa][J0] = ya_[oa]; yc[oa][J0 + 1] = yb_[oa]; } \
  }
#define W4_M(I, J, XPT) w4_xrd<(I)*6 + (J), XPT>(xr0, xr1)
#define W4_XREAD_COLS(XPT)                      \
  const unsigned xr1 = xr0 + 18u * (unsigned)(XPT); \
  W4_COLS(0, XPT)                               \
  W4_COLS(2, XPT)                               \
  W4_COLS(4, XPT)
// row pass of yc, scale / shift / residual / activation and the 16 stores of the lane; EACH: what the body does with a
// stored value v besides (w4_body's ST statistics).  Uses sc, sh, rv, act_lo, ry, vo, rowpitch, colpitch.
#define W4_ROWS_STORE(EACH)                                                                                            \
  _Pragma("unroll") for (int oa = 0; oa < 4; ++oa) {                                                                   \
    float yo[4];                                                                                                       \
    w4_at(yc[oa], yo);                                                                                                 \
    _Pragma("unroll") for (int ob = 0; ob < 4; ++ob) {                                                                 \
      const float v = fmaxf(__builtin_fmaf(yo[ob], sc, sh) + rv[oa][ob], act_lo);                                      \
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, vo, oa * rowpitch + ob * colpitch, 0); \
      EACH                                                                                                             \
    }                                                                                                                  \
  }
