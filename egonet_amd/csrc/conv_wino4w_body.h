// conv_wino4w_body.h -- the body of conv_wino4w_kernel (conv_wino4w.hip: the design notes are there), in a header so
// that conv_wino4_pair_kernel (conv_wino4.hip) can run it as one share of a two-convolution launch.
// Reference: the 3x3 stride-1 convolutions of libs/model/heatmapModel/hrnet.py (BasicBlock :49-76).
#pragma once
#include "conv_wino4.h"

namespace {
typedef W4G<1> QW;
constexpr int W4W_NT = 6;                          // co sub-tiles of an item: two 48-channel co-tiles
constexpr unsigned W4W_KGB = W4_UKG * 4u;          // filter bytes of one (co-tile, k-group)
}  // namespace

// value p = 3 pl + nt' of co-tile c of the pair: the slices of the filter registers (W4B9, conv_wino4.h) are the co-tiles
__device__ __forceinline__ float w4w_bval(const W4B9& b, int c, int p) { return b.val(c, p); }

// ABL (probe builds): bit 6 s_memtime stamps of every wave (tools/wino4_clk.py), dumped into `res`.
// blk / nblk: the block's index in its launch share and the share's size -- blockIdx.x / gridDim.x in conv_wino4w_kernel,
// the first share of conv_wino4_pair_kernel (conv_wino4.hip); the item order assumes block blk runs on XCD blk & 7.
template <int ABL>
__device__ __forceinline__ void w4w_body(const ConvArgs& a, int blk, int nblk) {
  typedef QW Q;
  extern __shared__ float4 w4_smem[];
  const unsigned lds0 = egn_lds_addr(w4_smem);
  const float* smf = reinterpret_cast<const float*>(w4_smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  const int tpart = wave >> 2;             // its third of the frequency rows of the input transform
  const int tw = wave & 3;                 // its k-group of the stage in the transform

  const int C = a.Cin, Co = a.Cout;
  const int nct = Co / W4_CO, ncp = nct >> 1;        // co-tiles, co-tile pairs
  const int S = C / 16;                    // stages of 16 channels

  const u32x4 rxv = egn_rsrc(a.x, (size_t)a.N * a.H * a.W * C * 4);
  const u32x4 ruv = egn_rsrc(a.w, (size_t)nct * (C >> 2) * W4_UKG * 4);
  const unsigned out_bytes = (unsigned)((size_t)a.N * a.Ho * a.Wo * Co * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, out_bytes, EGN_RSRC_WORD3);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res ? a.res : a.y), 0, out_bytes, EGN_RSRC_WORD3);

  // ---- halo loads (geometry 1): pieces wave, wave + 12; element e -> (pixel e / 4, channel quad e % 4), every lane to
  // the natural slot of its element (conv_wino4.h: the rows 18 / 19 fall on slots 90 .. 95 of a plane)
  W4_HALO_SLOTS_NATURAL(W4_NW, W4_H0)
  // ---- transform share: lane (tile li, channel 4 tw + kq of the stage)
  const unsigned hb0 = lds0 + (unsigned)(W4_H0 + ((2 * tw + (kq >> 1)) * Q::PAIR + Q::tileslot(li, tw)) * 8 + (kq & 1) * 4);
  const unsigned vw0 = lds0 + (unsigned)(W4_V0 + tw * 256 + lane * 4);        // V[pt][g][lane]
  // ---- multiply: A operands V[3 wave + pl][g][lane]
  const float* va0 = smf + (W4_V0 / 4) + (3 * wave) * 256 + lane;
  const unsigned uvo = (unsigned)lane * 16u;
  const int regs_x = a.tiles_x, regs_xy = a.tiles_x * a.tiles_y;
  const int nreg = regs_xy * a.N;
  const int imode = w4_item_mode(ncp);     // what the XCD owns, over co-tile PAIRS
  const int nwork = w4_item_count(imode, nreg, ncp, 1);
  const int gsz = __builtin_amdgcn_readfirstlane(nblk);
  const float act_lo = (a.act & EGN_ACT_MASK) == EGN_ACT_RELU ? 0.f : -__builtin_inff();
  const bool has_res = (ABL & 64) ? false : a.res != nullptr;
  const unsigned rowpitch = (unsigned)(a.Wo * Co) * 4u, colpitch = (unsigned)Co * 4u;
  const unsigned ctstride = (unsigned)(C >> 2) * W4W_KGB;        // filter bytes of a co-tile

  W4_STAMPS(96, w4_lds_bytes<1>(), wave)
  W4_CLK()
  for (int w = blk; w < nwork; w += gsz) {
    const unsigned wi = (unsigned)__builtin_amdgcn_readfirstlane(w);
    W4_ITEM_DECODE(wi, 1, ncp, reg, cp, ks_)
    if (reg >= nreg) continue;
    const int ct0 = 2 * cp;
    const W4Region rg_ = w4_item_region<1>(a, reg, regs_x, regs_xy);
    const int n = rg_.n, y0 = rg_.y0, x0 = rg_.x0;
    W4_HALO_DOFF(W4_NW)
    // filter of this wave: k-group h of co-tile ct = [ct][h][wave][3 x dwordx4 per lane], co-tiles ct0 and ct0 + 1.  Raw ISA: the waits are mine (tools/check_wino4_isa.py)
    const unsigned ubase = (unsigned)(ct0 * (C >> 2)) * W4W_KGB + (unsigned)wave * (3u * 64u * 16u);
#define W4_LOADB(DST, HS) w4_loadB(DST, ruv, uvo, HS, ctstride);   /* HS: byte offset of the k-group in co-tile ct0, W4_PAST = none */
    W4B9 b0, b1;
    f32x4 hreg[Q::NP];
    W4_PROLOGUE(W4_LOADB(b0, ubase), __builtin_amdgcn_s_barrier();)

    f32x4 acc[3][W4W_NT];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int nt = 0; nt < W4W_NT; ++nt) acc[pl][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // 18 MFMAs of a k-group in three groups of 6 (one frequency point each); H0 / H1 / H2: the vector-memory
    // instruction issued behind each group (w4_body, conv_wino4.hip: spread, not a burst behind the barrier)
#define W4_MUL6(PL, B)                                                                                         \
  _Pragma("unroll") for (int nt = 0; nt < W4W_NT; ++nt)                                                        \
      acc[PL][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_[PL], w4w_bval(B, nt / 3, (PL)*3 + nt % 3),             \
                                                         acc[PL][nt], 0, 0, 0);
#define W4_MUL(P, G, B, H0, H1, H2)                                                                            \
  {                                                                                                            \
    float av_[3];                                                                                              \
    _Pragma("unroll") for (int pl = 0; pl < 3; ++pl) av_[pl] = va0[((P) ? W4_VBYTES / 4 : 0) + (pl * 4 + (G)) * 64];  \
    W4_MUL6(0, B) __builtin_amdgcn_sched_barrier(0); H0 __builtin_amdgcn_sched_barrier(0);                     \
    W4_MUL6(1, B) __builtin_amdgcn_sched_barrier(0); H1 __builtin_amdgcn_sched_barrier(0);                     \
    W4_MUL6(2, B) __builtin_amdgcn_sched_barrier(0); H2 __builtin_amdgcn_sched_barrier(0);                     \
  }
    // the transform of stage s + 1, one third of the waves at each of three points of the stage -- each point where
    // only ONE filter buffer is live (the other's multiplies are issued, its next load is not): the register budget
    // Stage s (parity P): k-groups 4s .. 4s+3.  Wait group h is issued one multiply (18 MFMAs) before it is awaited,
    // alone in the queue -- except the last wait of the stage, which also retires the halo pieces of stage s + 2
    // issued behind the first MFMA groups of k-group 3: no wait needs a count.
#define W4_STAGE(P, SI)                                                                                        \
  {                                                                                                            \
    const int s_ = (SI);                                                                                       \
    const unsigned dst_ = s_ + 2 < S ? (unsigned)(s_ + 2) * (unsigned)Q::SBYTES : W4_PAST;                     \
    const unsigned u0_ = ubase + (unsigned)(4 * s_) * W4W_KGB;                                                 \
    const unsigned bn_ = s_ + 1 < S ? u0_ + 4u * W4W_KGB : W4_PAST;                                            \
    w4_vm_landedB(b0);                                                                                        \
    W4_CLK() /* 0: k-group 4s landed */                                                                        \
    W4_TRANS(P, 0)                                                                                             \
    W4_LOADB(b1, u0_ + W4W_KGB)                                                                                \
    W4_CLK() /* 1: (transform third 0 +) loads issued */                                                       \
    W4_MUL(P, 0, b0, , , )                                                                                     \
    W4_CLK() /* 2: k-group 0 multiplies issued */                                                              \
    w4_vm_landedB(b1);                                                                                        \
    W4_CLK() /* 3: k-group 4s+1 landed */                                                                      \
    W4_TRANS(P, 1)                                                                                             \
    W4_LOADB(b0, u0_ + 2u * W4W_KGB)                                                                           \
    W4_MUL(P, 1, b1, , , )                                                                                     \
    W4_CLK() /* 4: (transform third 1 +) k-group 1 multiplies issued */                                        \
    w4_vm_landedB(b0);                                                                                        \
    W4_LOADB(b1, u0_ + 3u * W4W_KGB)                                                                           \
    W4_MUL(P, 2, b0, , , )                                                                                     \
    W4_CLK() /* 5: k-group 2 multiplies issued */                                                              \
    w4_vm_landedB(b1);                                                                                        \
    W4_TRANS(P, 2)                                                                                             \
    W4_LOADB(b0, bn_)                                                                                          \
    W4_MUL(P, 3, b1, W4_HLOAD(0, dst_), W4_HLOAD(1, dst_), )                                                   \
    W4_CLK() /* 6: (transform third 2 +) k-group 3 multiplies issued */                                        \
    w4_vm_landedH(hreg);             /* the pieces of stage s + 2 and k-group 4s+4 */                          \
    W4_HSTORE(P)                                                                                               \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                         \
    W4_CLK() /* 7: own pieces of stage s + 2 in LDS, V writes done */                                          \
    __builtin_amdgcn_s_barrier();                                                                              \
    asm volatile("" ::: "memory");                                                                             \
    W4_CLK() /* 8: past the barrier */                                                                         \
  }
    for (int s = 0; s + 1 < S; s += 2) {
      W4_STAGE(0, s)
      W4_STAGE(1, s + 1)
    }
    if (S & 1) W4_STAGE(0, S - 1)            // (every item starts at parity 0)
    // the loads past the end: tied to the wait (w4_body, conv_wino4.hip)
    w4_vm_landedB(b0);
    w4_vm_landedB(b1);
    w4_vm_landedH(hreg);
    W4_CLK()      /* K loop done */
#undef W4_STAGE
#undef W4_MUL
#undef W4_MUL6
#undef W4_LOADB

    // ---- item end: per co-tile, accumulators -> LDS -> one (tile, co) per lane -> Y = A^T M A -> epilogue
    // exchange + output (the rotated write and the round's pieces: conv_wino4.h): this lane finishes tile 4 (wave & 3) + (lane >> 4), co 16 (wave >> 2) + li.
    // Addresses from an opaque copy of the lane id: computed here, not held in registers over the K loop.
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int li_e = lane_e & 15, kq_e = lane_e >> 4;
    const int ont = wave >> 2, okq = wave & 3;
    const unsigned xhi = (unsigned)(li_e >> 3);
    const unsigned xw0 = lds0 + (unsigned)((3 * wave) * 3 * 1024 + lane_e * 16);
    const unsigned xwa = xw0 + 8u * xhi, xwb = xw0 + 8u - 8u * xhi;
    const unsigned xr0 = lds0 + (unsigned)((ont * 64 + okq * 16 + li_e) * 16) + (((unsigned)kq_e + 2u * xhi) & 3u) * 4u;
    const int tile = 4 * okq + kq_e;
    const int ty = tile >> 2, tx = tile & 3;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int cch = (ct0 + r) * W4_CO + ont * 16 + li_e;
      const float sc = a.scale[cch];
      const float sh = a.shift[cch];
      const unsigned vo = (unsigned)((((n * a.Ho + y0 + 4 * ty) * a.Wo + x0 + 4 * tx) * Co + cch) * 4);
      float rv[4][4];
      W4_RES_LOAD(rv, has_res ? vo : EGN_OOB)
      w4_xw<0 * 1024>(xwa, xwb, acc[0][3 * r + 0]); w4_xw<1 * 1024>(xwa, xwb, acc[0][3 * r + 1]); w4_xw<2 * 1024>(xwa, xwb, acc[0][3 * r + 2]);
      w4_xw<3 * 1024>(xwa, xwb, acc[1][3 * r + 0]); w4_xw<4 * 1024>(xwa, xwb, acc[1][3 * r + 1]); w4_xw<5 * 1024>(xwa, xwb, acc[1][3 * r + 2]);
      w4_xw<6 * 1024>(xwa, xwb, acc[2][3 * r + 0]); w4_xw<7 * 1024>(xwa, xwb, acc[2][3 * r + 1]); w4_xw<8 * 1024>(xwa, xwb, acc[2][3 * r + 2]);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xC07F);
      W4_CLK()    /* round: accumulators written */
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      W4_CLK()    /* round: exchange barrier passed */
      float yc[4][6];
      W4_XREAD_COLS(3072)
      W4_ROWS_STORE()
      asm volatile("" ::: "memory");
      W4_CLK()    /* round: output transform done, stores issued */
      __builtin_amdgcn_s_barrier();      // the exchange buffer is free again (next round / next item's halo)
      asm volatile("" ::: "memory");
      W4_CLK()    /* round: end */
    }
  }
  if constexpr ((ABL & 64) != 0) w4_stamp_dump<W4_NW, W4_NTK, 1>(a, sT, ntk, tid);
}
