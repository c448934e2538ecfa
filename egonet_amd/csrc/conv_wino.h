// conv_wino.h -- what the fused Winograd F(2x2,3x3) kernels of conv_wino.hip share: the block-tile geometries
// (WinoGeom / WinoDims) and ONE definition of every part the kernel bodies have in common -- buffer descriptors, the
// item walk, the halo slot table and its DMA offsets, a DMA piece and its place between two scheduling barriers, the
// stamps, the per-item registers, the residual loads, the partial exchange and the BatchNorm statistics.  The
// hazard-sensitive pieces (the wave-uniform skip of the last halo piece, the program order DMA -> residual loads that
// the vmcnt(24) ties count on, the two-barrier exchange, the once-per-block statistics row) are fixed here, once.
//
// The bodies must compile to the instruction streams they had as hand-copied text (profiles/wino_shared_isa.txt).  A
// __forceinline__ function is simplified on its own, before the ranges of the body's values are known; so a part is a
// function where that reproduced the stream and otherwise a macro that relies on BODY-LOCAL NAMES, the same in every
// body:
//   constants   NTH (threads), NT / CO_T (co sub-tiles / output channels per block), KQ / HS / UCH / USL (channel quads
//               per stage, stages per chunk, float4 of a packed chunk / of a filter stage), SLOTS / BUF (halo float4 per
//               stage / per stage buffer), IT / NPIECE (halo / all DMA pieces per lane and stage), WHOLE_PIECES,
//               STAMPS, TH / TW / TNB and G = WinoGeom<TH, TW, TNB>
//   values      a, tid, lane, wave, li, kq, C, Co, nct, nchunk, tiles_xy, ntile, sU, sH, sS, sT, ntk, rxv, ruv, ry, rr,
//               hmeta, hq, urel, og, tile, ct, voff, sc, sh, acc, rv, colpitch, par, nx_issue, nx_ct, nx_ch, keep, send
#pragma once
#include "conv_common.h"

// Output channels per block (co-tile, egn_wino_cot in egn_internal.h): 48 (NT = 3 MFMA column tiles)
// where Cout allows -- the widths of HRNet-W48 (48 / 96 / 192 / 384) -- else 32 (NT = 2): the W32 /
// Pedestrian widths (32 / 64 / 128 / 256) and the 64-channel stem layers.  The SAME rule in the filter
// packing, the planner and the launcher.

namespace {
constexpr int WN_CO = 48;                          // the 4-wave kernel: 48 output channels per block (NT = 3)
constexpr int WN_NT = 3;
constexpr int WN_USLOTS = 16 * EGN_CKQ * WN_CO;    // float4 per (chunk, co-tile) slab of U: 3072 = 48 KB
constexpr int WN_NTH = 256;
constexpr int WN_UIT = WN_USLOTS / WN_NTH;         // 12 DMA instructions per lane and slab
constexpr int WINO_NTK = 48;                       // stamps per wave of a stamp build
}  // namespace

// Geometry of a block tile (64 Winograd tiles = 4 waves x 16) and the LDS image of its halo chunk.
//
// The halo lives in LDS as FOUR CHANNEL-QUAD PLANES  sH[quad][pixel slot]  (16 B per slot), not pixel
// major: a patch read (one ds_read_b128 per lane) is served in 4 groups of 16 lanes, each group holding
// all 16 tiles (li) of the wave with only two quad values, so it is conflict free exactly when the 16
// tiles' pixel slots are distinct mod 16 (and the plane size is a multiple of 256 B).  Tiles step by TWO
// pixels, so plain row-major slots collide; each geometry therefore skews its rows / images:
//   <16,16,1>  tile li = (ty = li>>3, tx = li&7): slot = y*24 + ((y>>1)&1) + x.  The two tile rows of a
//              wave are 2 pixel rows apart = 48 slots (= 0 mod 16) +- 1 from the skew: 2tx + {0,1}.
//   <8,8,4>    wave = tile row, li = (image b = li>>2, tx = li&3): slot = b*112 + g(b) + y*10 + x with
//              g = {0,1,8,9}: 2tx + g(b) covers 0..15.
// (pixel-major slots measured 4-way conflicts: 16 instead of 4 LDS cycles per read, 16 % of a K step.)
template <int TH, int TW, int TNB>
struct WinoGeom;

template <>
struct WinoGeom<16, 16, 1> {
  static constexpr int TH = 16, TW = 16, TNB = 1, HH = 18, HW = 18;
  static constexpr int RP = 24, PLANE = 432;     // 18 rows x 24 slots; 6912 B = 27 x 256
  static constexpr int ROFF = RP;                // slot step of one patch row
  // DMA slot p of a plane -> halo pixel (b, hy, hx) or -1
  static __device__ __forceinline__ int decode(int p) {
    const int y = p / RP, x = p - y * RP - ((y >> 1) & 1);
    return (y < HH && x >= 0 && x < HW) ? ((y << 8) | x) : -1;
  }
  // slot of the patch origin of tile li of wave w, for patch rows {0,1} (k = 0) / {2,3} (k = 1)
  static __device__ __forceinline__ int patch_base(int w, int li, int k) {
    const int tyl = li >> 3, tx = li & 7;
    return (4 * w + 2 * tyl) * RP + 2 * tx + ((tyl + k) & 1);
  }
  // tile index (b << 16 | ty << 8 | tx) of MFMA result row m (0..15) of wave w
  static __device__ __forceinline__ int out_tile(int w, int m) { return ((2 * w + (m >> 3)) << 8) | (m & 7); }
};

template <>
struct WinoGeom<8, 8, 4> {
  static constexpr int TH = 8, TW = 8, TNB = 4, HH = 10, HW = 10;
  static constexpr int RP = 10, IMGP = 112, PLANE = 448;   // 7168 B = 28 x 256
  static constexpr int ROFF = RP;
  static __device__ __forceinline__ int skew(int b) { return (b & 1) + ((b & 2) << 2); }  // 0, 1, 8, 9
  static __device__ __forceinline__ int decode(int p) {
    const int b = p / IMGP, r = p - b * IMGP - skew(b);
    const int y = r / RP, x = r - y * RP;
    return (r >= 0 && r < HH * RP) ? ((b << 16) | (y << 8) | x) : -1;
  }
  static __device__ __forceinline__ int patch_base(int w, int li, int) {
    const int b = li >> 2, tx = li & 3;
    return b * IMGP + skew(b) + 2 * w * RP + 2 * tx;
  }
  static __device__ __forceinline__ int out_tile(int w, int m) { return ((m >> 2) << 16) | (w << 8) | (m & 3); }
};

// half of the 16 x 16 tile (8 rows x 16 columns = 32 Winograd tiles, conv_wino8_kernel with 4 waves): twice
// the work items for maps / batches that leave CUs idle with the 64-tile form.  Same slots, fewer rows.
template <>
struct WinoGeom<8, 16, 1> {
  static constexpr int TH = 8, TW = 16, TNB = 1, HH = 10, HW = 18;
  static constexpr int RP = 24, PLANE = 256;     // 10 rows x 24 slots = 240, padded to 16 x 256 B
  static constexpr int ROFF = RP;
  static __device__ __forceinline__ int decode(int p) {
    const int y = p / RP, x = p - y * RP - ((y >> 1) & 1);
    return (y < HH && x >= 0 && x < HW) ? ((y << 8) | x) : -1;
  }
  static __device__ __forceinline__ int patch_base(int w, int li, int k) {
    const int tyl = li >> 3, tx = li & 7;
    return (4 * w + 2 * tyl) * RP + 2 * tx + ((tyl + k) & 1);
  }
  static __device__ __forceinline__ int out_tile(int w, int m) { return ((2 * w + (m >> 3)) << 8) | (m & 7); }
};

// two 8 x 8 images per block (32 Winograd tiles = 2 m-tiles; conv_wino8_kernel with 4 waves): m-tile mt
// holds tile rows {2mt, 2mt+1} of both images, li = (b = li>>3, row = (li>>2)&1, tx = li&3):
// slot = b*128 + b + y*12 + x -- 2tx + {0, 24 = 8 mod 16} + {0, 1} covers 0..15.
template <>
struct WinoGeom<8, 8, 2> {
  static constexpr int TH = 8, TW = 8, TNB = 2, HH = 10, HW = 10;
  static constexpr int RP = 12, IMGP = 128, PLANE = 256;   // 4096 B = 16 x 256
  static constexpr int ROFF = RP;
  static __device__ __forceinline__ int decode(int p) {
    const int b = p / IMGP, r = p - b * IMGP - b;
    const int y = r / RP, x = r - y * RP;
    return (r >= 0 && r < HH * RP && x < HW) ? ((b << 16) | (y << 8) | x) : -1;
  }
  static __device__ __forceinline__ int patch_base(int mt, int li, int) {
    const int b = li >> 3, tyl = (li >> 2) & 1, tx = li & 3;
    return b * IMGP + b + 2 * (2 * mt + tyl) * RP + 2 * tx;
  }
  static __device__ __forceinline__ int out_tile(int mt, int m) {
    return ((m >> 3) << 16) | ((2 * mt + ((m >> 2) & 1)) << 8) | (m & 3);
  }
};

template <int TH, int TW, int TNB>
struct WinoDims {
  using G = WinoGeom<TH, TW, TNB>;
  static constexpr int SLOTS = EGN_CKQ * G::PLANE;
  static constexpr int IT = (SLOTS + WN_NTH - 1) / WN_NTH;  // DMA instructions per lane and halo chunk
  static constexpr int BUF = IT * WN_NTH;                   // every wave issues IT whole instructions
  static_assert(G::PLANE % 16 == 0, "planes must start on a 256-byte boundary");
  static_assert(TNB * (TH / 2) * (TW / 2) == 64 || TNB * (TH / 2) * (TW / 2) == 32, "m-tiles of 16 Winograd tiles");
};

// ---- buffer descriptors: input (halo DMA), packed filter of U_BYTES bytes (filter DMA), output, residual ----
#define WINO_DESCRIPTORS(U_BYTES)                                                                                    \
  const u32x4 rxv = egn_rsrc(a.x, (size_t)a.N * a.H * a.W * C * 4);                                                  \
  const u32x4 ruv = egn_rsrc(a.w, U_BYTES);                                                                          \
  const unsigned out_bytes = (unsigned)((size_t)a.N * a.Ho * a.Wo * Co * 4);                                         \
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, out_bytes, EGN_RSRC_WORD3);            \
  const __amdgpu_buffer_rsrc_t rr =                                                                                  \
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res ? a.res : a.y), 0, out_bytes, EGN_RSRC_WORD3);

// ---- stamps (tools/wino_clk.py only; STAMPS builds): s_memtime of every wave's lane 0 -- kept in LDS (sT, WINO_NTK
// per wave), copied to the buffer passed as `res` at the end of the kernel (no residual then), so the vmcnt bookkeeping
// is untouched ----
#define WINO_CLK()                                                                                  \
  {                                                                                                 \
    if constexpr (STAMPS) {                                                                         \
      if (lane == 0 && ntk < WINO_NTK) sT[wave * WINO_NTK + ntk] = __builtin_readcyclecounter();    \
      ++ntk;                                                                                        \
    }                                                                                               \
  }
template <int NW>
__device__ __forceinline__ void wino_stamp_dump(const ConvArgs& a, const unsigned long long* sT, int ntk, int tid) {
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(const_cast<float*>(a.res)) +
                            (size_t)blockIdx.x * (NW * WINO_NTK + 1);
  for (int e = tid; e < NW * WINO_NTK; e += 64 * NW) out[1 + e] = sT[e];
  if (tid == 0) out[0] = (unsigned long long)ntk;
}

// ---- item walk: work index w -> (spatial tile, co-tile).  Blocks w, w+8, w+16 ... run on one XCD (block b -> XCD
// b % 8): the co-tiles of ONE spatial tile are consecutive slots of one XCD, so the halo they all read is fetched
// into that XCD's L2 once.  (conv_wino9_kernel's W9_ITEM is the scalar-unit form of the same map.) ----
#define WINO_ITEM(Wi, TILE_, CT_)            \
  {                                          \
    const int x_ = (Wi)&7, q_ = (Wi) >> 3;   \
    TILE_ = (q_ / nct) * 8 + x_;             \
    CT_ = q_ - (q_ / nct) * nct;             \
  }

// ---- halo slot e = it * NTH + tid -> (quad plane, pixel slot) -> (image b, hy, hx); item independent.
// hmeta = b << 16 | hy << 8 | hx, -1 = pad slot; hq = byte offset of the quad e / PLANE ----
#define WINO_HALO_SLOTS()                                                       \
  int hmeta[IT];                                                                \
  unsigned hq[IT];                                                              \
  _Pragma("unroll") for (int it = 0; it < IT; ++it) {                           \
    const int e = it * NTH + tid;                                               \
    const int q = e / G::PLANE;                                                 \
    hmeta[it] = (e < SLOTS && q < EGN_CKQ) ? G::decode(e - q * G::PLANE) : -1;  \
    hq[it] = (unsigned)q * 16u;                                                 \
  }
// halo DMA byte offsets (chunk 0) of a spatial tile; out-of-image and pad slots get the OOB offset
// and are written as zeros by the same DMA (= the convolution's zero padding)
#define WINO_DOFF(TILE_, OUT)                                                                       \
  {                                                                                                 \
    const int tb_ = (TILE_) / tiles_xy;                                                             \
    const int r_ = (TILE_)-tb_ * tiles_xy;                                                          \
    const int ty_ = r_ / a.tiles_x, tx_ = r_ - ty_ * a.tiles_x;                                     \
    const int n0_ = tb_ * TNB, iy0_ = ty_ * TH - 1, ix0_ = tx_ * TW - 1;                            \
    _Pragma("unroll") for (int it = 0; it < IT; ++it) {                                             \
      const int m_ = hmeta[it];                                                                     \
      const int n_ = n0_ + (m_ >> 16), iy_ = iy0_ + ((m_ >> 8) & 255), ix_ = ix0_ + (m_ & 255);     \
      const bool in_ = m_ >= 0 && (TILE_) < ntile && n_ < a.N && iy_ >= 0 && iy_ < a.H && ix_ >= 0 && ix_ < a.W; \
      OUT[it] = in_ ? (unsigned)(((n_ * a.H + iy_) * a.W + ix_) * C) * 4u + hq[it] : EGN_OOB;       \
    }                                                                                               \
  }

// ---- the scalar-unit forms of the two above (conv_wino9_kernel; written to be different: divisions by multiply-high
// with the launcher's multipliers on readfirstlane'd values, per-lane offsets = a wave-uniform base + the relative
// offsets hyx / hb / hrel the body computes once).  w -> (tile, ct) -> (tb, ty, tx): ----
#define W9_ITEM(Wi, TILE_, CT_, TB_, TY_, TX_)                                   \
  {                                                                              \
    const unsigned wi_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(Wi));    \
    const unsigned x_ = wi_ & 7u, q_ = wi_ >> 3;                                 \
    const unsigned qq_ = egn_udiv_magic(q_, a.mg_nct);                           \
    TILE_ = (int)(qq_ * 8u + x_);                                                \
    CT_ = (int)(q_ - qq_ * (unsigned)nct);                                       \
    const unsigned tb_ = egn_udiv_magic((unsigned)TILE_, a.mg_txy);              \
    const unsigned r_ = (unsigned)TILE_ - tb_ * (unsigned)tiles_xy;              \
    const unsigned ty_ = egn_udiv_magic(r_, a.mg_tx);                            \
    TB_ = (int)tb_; TY_ = (int)ty_; TX_ = (int)(r_ - ty_ * (unsigned)a.tiles_x); \
  }
// halo DMA byte offsets (chunk 0) of a tile: uniform base + per-lane relative offset; pad slots and
// out-of-image pixels get the OOB offset (the DMA writes zeros there = the convolution's zero padding)
#define W9_DOFF(TILE_, TB_, TY_, TX_, OUT)                                                                   \
  {                                                                                                          \
    const int n0_ = (TB_)*TNB, iy0_ = (TY_)*TH - 1, ix0_ = (TX_)*TW - 1;                                     \
    const int base_ = ((n0_ * a.H + iy0_) * a.W + ix0_) * C * 4;                                             \
    const bool tok_ = (TILE_) < ntile;                                                                       \
    _Pragma("unroll") for (int it = 0; it < IT; ++it) {                                                      \
      const unsigned iy_ = (unsigned)(iy0_ + (hyx[it] >> 16)), ix_ = (unsigned)(ix0_ + (hyx[it] & 0xffff));  \
      bool in_ = tok_ && hyx[it] >= 0 && iy_ < (unsigned)a.H && ix_ < (unsigned)a.W;                         \
      if (TNB > 1) in_ = in_ && (n0_ + hb[it]) < a.N;                                                        \
      OUT[it] = in_ ? (unsigned)(base_ + hrel[it]) : EGN_OOB;                                                \
    }                                                                                                        \
  }

// ---- filter stage slot e = piece * NTH + tid of a HALF-chunk stage (KQ < EGN_CKQ) -> frequency e / (KQ * CO_T): its
// KQ * CO_T slots sit EGN_CKQ * CO_T apart in the packed chunk.  With whole-chunk stages a piece is contiguous
// (offset tid * 16) and urel is an unused placeholder. ----
#define WINO_FILTER_SLOTS()                                                                  \
  unsigned urel[KQ == EGN_CKQ ? 1 : USL / NTH];                                              \
  if constexpr (KQ != EGN_CKQ) {                                                             \
    _Pragma("unroll") for (int k_ = 0; k_ < USL / NTH; ++k_) {                               \
      const int e = k_ * NTH + tid, f_ = e / (KQ * CO_T);                                    \
      urel[k_] = (unsigned)(f_ * (EGN_CKQ * CO_T) + (e - f_ * (KQ * CO_T))) * 16u;           \
    }                                                                                        \
  }
// ---- DMA instruction K (0 .. NPIECE-1) of a stage into stage buffer P: halo stage CH (chunk CH / HS, quads
// (CH % HS) * KQ ...) of the tile with offsets OFF (K < IT), then the filter stage (CT, CH).  A wave beyond the end of
// the halo image skips its share of the last halo piece (wave-uniform) -- unless the body pads BUF to whole pieces
// (WHOLE_PIECES, conv_wino_kernel: every wave issues all pieces). ----
#define WINO_PIECE(K, P, OFF, CT, CH)                                                                \
  {                                                                                                  \
    if ((K) < IT) {                                                                                  \
      if (WHOLE_PIECES || (K)*NTH + wave * 64 < SLOTS)                                               \
        egn_lds_dma16(rxv, egn_lds_addr(sH + (P)*BUF + wave * 64) + (K)*NTH * 16, OFF[(K) < IT ? (K) : 0], \
                   (unsigned)(CH) * (KQ * 16u));                                                     \
    } else if constexpr (KQ == EGN_CKQ) {                                                            \
      egn_lds_dma16(ruv, egn_lds_addr(sU + (P)*USL + wave * 64) + ((K)-IT) * NTH * 16, (unsigned)tid * 16u, \
                 (unsigned)(((CT)*nchunk + (CH)) * USL) * 16u + ((K)-IT) * NTH * 16);                \
    } else {                                                                                         \
      const unsigned ch_ = (unsigned)(CH) / HS, hs_ = (unsigned)(CH) - ch_ * HS;                     \
      egn_lds_dma16(ruv, egn_lds_addr(sU + (P)*USL + wave * 64) + ((K)-IT) * NTH * 16, urel[(K) >= IT ? (K)-IT : 0], \
                 (((unsigned)(CT)*nchunk + ch_) * UCH + hs_ * (KQ * CO_T)) * 16u);                   \
    }                                                                                                \
  }
// all pieces of a stage at once (the prologue of a block)
#define WINO_ISSUE(P, OFF, CT, CH) \
  { _Pragma("unroll") for (int k_ = 0; k_ < NPIECE; ++k_) WINO_PIECE(k_, P, OFF, CT, CH) }
// piece K of the NEXT stage --(this item, stage c + 1) or (next item, stage 0), offsets OFF -- pinned between two
// scheduling barriers so that it stays where the body puts it among the MFMAs
#define WINO_NEXT(K, OFF)                                  \
  {                                                        \
    __builtin_amdgcn_sched_barrier(0x0106);                \
    if (nx_issue) WINO_PIECE(K, par ^ 1, OFF, nx_ct, nx_ch) \
    __builtin_amdgcn_sched_barrier(0x0106);                \
  }

// ---- per item: output byte offsets of this lane's 4 tiles (MFMA result rows 4kq + r), output row ROW of each
// (0: conv_wino_kernel stores both rows from there; fh: the frequency-halves kernel) ----
#define WINO_VOFF(ROW)                                                                                      \
  unsigned voff[4];                                                                                         \
  {                                                                                                         \
    const int tb_ = tile / tiles_xy;                                                                        \
    const int r_ = tile - tb_ * tiles_xy;                                                                   \
    const int ty_ = r_ / a.tiles_x, tx_ = r_ - ty_ * a.tiles_x;                                             \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                         \
      const int n = tb_ * TNB + (og[r] >> 16);                                                              \
      const int oy = ty_ * TH + 2 * ((og[r] >> 8) & 255) + (ROW), ox = tx_ * TW + 2 * (og[r] & 255);        \
      voff[r] = (tile < ntile && n < a.N && oy < a.Ho && ox < a.Wo)                                         \
                    ? (unsigned)(((n * a.Ho + oy) * a.Wo + ox) * Co + ct * CO_T + li) * 4u                  \
                    : EGN_OOB;                                                                              \
    }                                                                                                       \
  }
// scale / shift of this lane's NT output channels and the NF x NT accumulators of its frequencies, zeroed
#define WINO_SCALE_ACC(NF)                                                                      \
  float sc[NT], sh[NT];                                                                         \
  _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                           \
    sc[nt] = a.scale[ct * CO_T + nt * 16 + li];                                                 \
    sh[nt] = a.shift[ct * CO_T + nt * 16 + li];                                                 \
  }                                                                                             \
  f32x4 acc[NF][NT];                                                                            \
  _Pragma("unroll") for (int f = 0; f < NF; ++f)                                                \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[f][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

// ---- frequency-halves kernels: residual of this lane's outputs rv[tile r][b][nt], loaded behind the LAST DMA piece of
// an item's last stage (without a residual -- ON false: OOB offsets, zeros, the same instruction stream).  The vmcnt(24)
// at the next item's first step counts on the program order DMA -> residual loads -> stores; the asm has no memory
// clobber, so the order is pinned here. ----
#define WINO_RES_LOAD(ON)                                                                                  \
  {                                                                                                        \
    asm volatile("" ::: "memory");                                                                         \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                        \
      const unsigned ro = (ON) ? voff[r] : EGN_OOB;                                                        \
      _Pragma("unroll") for (int pb = 0; pb < 2; ++pb)                                                     \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) rv[r][pb][nt] = egn_buf_load4(rr, ro, pb * colpitch + nt * 64u); \
    }                                                                                                      \
  }

// ---- frequency-halves kernels: the partial exchange between the two waves (wave, wave ^ MTILES) of an m-tile, 24
// floats per lane.  The U buffer of the last K step (par ^ 1 after the toggle) is free once every wave is past its
// MFMAs: barrier, write send[], barrier, read the partner's into keep[] = COMBINE, an expression in keep_ (own) and
// recv_ (the partner's). ----
#define WINO_EXCHANGE(COMBINE)                                                                             \
  {                                                                                                        \
    float4* xch = sU + (par ^ 1) * USL;                                                                    \
    asm volatile("" ::: "memory");                                                                         \
    __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0) only */                                              \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("" ::: "memory");                                                                         \
    _Pragma("unroll") for (int k4 = 0; k4 < 2 * NT; ++k4) {                                                \
      f32x4 v;                                                                                             \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                      \
        const int idx = k4 * 4 + e; /* (nt*4 + r)*2 + pb */                                                \
        v[e] = send[idx >> 3][(idx >> 1) & 3][idx & 1];                                                    \
      }                                                                                                    \
      *reinterpret_cast<f32x4*>(&xch[(wave * 2 * NT + k4) * 64 + lane]) = v;                               \
    }                                                                                                      \
    asm volatile("" ::: "memory");                                                                         \
    __builtin_amdgcn_s_waitcnt(0xC07F);                                                                    \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("" ::: "memory");                                                                         \
    _Pragma("unroll") for (int k4 = 0; k4 < 2 * NT; ++k4) {                                                \
      const f32x4 v = *reinterpret_cast<const f32x4*>(&xch[((wave ^ MTILES) * 2 * NT + k4) * 64 + lane]);  \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                      \
        const int idx = k4 * 4 + e;                                                                        \
        const float keep_ = keep[idx >> 3][(idx >> 1) & 3][idx & 1], recv_ = v[e];                         \
        keep[idx >> 3][(idx >> 1) & 3][idx & 1] = (COMBINE);                                               \
      }                                                                                                    \
    }                                                                                                      \
  }

// ---- BatchNorm batch statistics in the epilogue (training: raw conv output, scale 1 / shift 0).  sS is a small LDS
// table of doubles, [wave][2][CO_T]: each wave zeroes its own rows at block start (no barrier needed before the first
// use), adds its column sums per item, and the block writes ONE partial row at the end of the kernel -- its co-tile is
// the same for all its items (wino8_grid). ----
#define WINO_STATS_ZERO()                                                            \
  if (a.stats != nullptr) {                                                          \
    for (int e = lane; e < 2 * CO_T; e += 64) sS[wave * 2 * CO_T + e] = 0.0;         \
  }
// this wave's column sums st1 / st2 over its 16 tiles x 2 pixels -- lanes li + 16*kq hold the same channel -- added to
// its row
#define WINO_STATS_ADD()                                                             \
  if (a.stats != nullptr) {                                                          \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                              \
      st1[nt] += __shfl_xor(st1[nt], 16);                                            \
      st1[nt] += __shfl_xor(st1[nt], 32);                                            \
      st2[nt] += __shfl_xor(st2[nt], 16);                                            \
      st2[nt] += __shfl_xor(st2[nt], 32);                                            \
    }                                                                                \
    if (kq == 0) {                                                                   \
      double* srow = sS + wave * 2 * CO_T + li;                                      \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                            \
        srow[nt * 16] += (double)st1[nt];                                            \
        srow[CO_T + nt * 16] += (double)st2[nt];                                     \
      }                                                                              \
    }                                                                                \
  }
// one partial row per block: [2][Cout] doubles, the block's CO_T columns (co-tile ct_block) = its waves' sums in wave
// order, zeros elsewhere (egn_bn_stats_finalize_f32 adds the rows of all blocks in a fixed order)
#define WINO_STATS_ROW()                                                             \
  if (a.stats != nullptr) {                                                          \
    __syncthreads();                                                                 \
    double* row = a.stats + (size_t)blockIdx.x * 2 * Co;                             \
    for (int e = tid; e < 2 * Co; e += NTH) {                                        \
      const int which = e / Co, c = e - which * Co;                                  \
      const int cl = c - ct_block * CO_T;                                            \
      double v = 0.0;                                                                \
      if (cl >= 0 && cl < CO_T) {                                                    \
        for (int k = 0; k < NW; ++k) v += sS[(k * 2 + which) * CO_T + cl];           \
      }                                                                              \
      row[e] = v;                                                                    \
    }                                                                                \
  }
