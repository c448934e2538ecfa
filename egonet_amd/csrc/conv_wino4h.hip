// conv_wino4h.hip -- fused Winograd F(4x4,3x3) in HALF-size blocks, two independent blocks per CU [round 6].
//
// OUTCOME: measured NEGATIVE in both forms, kept for probe builds only (-DEGN_PROBES):
//   conv_wino4h_kernel (two 6-wave workgroups per CU)   64.3 us against conv_wino4_kernel's 51.1 on 48 -> 48 @ 64 x 64, 64 crops:
//                      the two workgroups of a CU are never resident together (profiles/r6_wino4h_timeline.txt);
//   conv_wino4d_kernel (two halves of one 12-wave workgroup, LDS-counter barriers)   52.7 us; 118 000 cycles per CU against
//                      103 000 (profiles/r6_wino4d_timeline.txt).  The start skew (EGN_W4H_SKEW, default 0) changes nothing.
// What follows is the design as it was built.
//
// Why.  An item of conv_wino4_kernel on the 48-channel branch (48 -> 48 @ 64 x 64: 24 % of the forward's kernel time)
// spends 11 % of its cycles in the prologue (first halo pieces, first transform) and 21 % in the item end (exchange,
// Y = A^T M A, stores) with the matrix pipe idle (profiles/r3_wino4_timeline_v2.txt; ablation: -28 % without the item
// end, profiles/r4_wino4_experiments.txt item 6) -- one 12-wave block per CU runs them in lock step.  conv_pw_kernel and
// conv_s2r_kernel (round 5) went from 52-58 % to 65-72 % MFMA busy with "several small independent blocks per CU": one
// block's item end runs under another's MFMAs.  This is that recipe for F(4x4,3x3):
//   * block = 6 waves, item = ONE m-tile (16 tiles = a 16 x 16 pixel region) x 48 output channels, 8-channel stages;
//     wave w owns frequency points 6w .. 6w+5 for the three co sub-tiles: 18 MFMAs per 4-channel k-group, 72 accumulator
//     registers -- per wave the same work per stage as conv_wino4_kernel (36 MFMAs, one third of a k-group's transform,
//     two halo pieces), per block half of it;
//   * LDS 62 KB (two V buffers [36 points][2 k-groups][64] = 18 KB, two halo buffers of 13 KB in GEO 0's store-conflict-
//     free order on GEO 1's region): two blocks per CU, 168 VGPRs = three waves per SIMD as before;
//   * the filter is read in wino4_pack.h's layout as it lies: the wave's 6 points are the slices of the 12-wave
//     kernel's waves 2w and 2w+1 (values 0..7 as two dwordx4, value 8 as a dword: 18 registers per buffer);
//   * item end: the 108 KB exchange image of an m-tile does not fit twice into a CU -- two rounds of 54 KB
//     ([point][6 units of 16 lanes][float4]: a unit = (co sub-tile, tile quad) = a quarter C fragment; round r holds
//     units 6r .. 6r+5, i.e. 1.5 co sub-tiles), reader wave rw finishes unit 6r + rw: every lane one (tile, co).
// Phase: two blocks that start together stay in phase (profiles/r3_wino9_kq2_timeline.txt) and would idle the pipe
// together.  The second block of a CU (its LDS allocation does not start at 0: HW_REG_LDS_ALLOC) therefore starts
// `skew` x 64 cycles late (ConvArgs::spix_off, set by the launcher from EGN_W4H_SKEW; no value helped).
// Every vector-memory wait is vmcnt(0) (conv_wino4.hip).
// Reference: the 3x3 stride-1 convolutions of libs/model/heatmapModel/hrnet.py (BasicBlock :49-76).
#include <stdlib.h>

#include "conv_wino4.h"

namespace {
typedef W4G<3> QH;
constexpr int W4H_NW = 6, W4H_NTH = 64 * W4H_NW;
constexpr int W4H_VBYTES = 36 * QH::VPT;                       // 18 KB
constexpr int W4H_V0 = 0, W4H_H0 = 2 * W4H_VBYTES;
constexpr int W4H_LDS = W4H_H0 + 2 * QH::HBYTES;               // 62 KB
constexpr int W4H_XPT = 6 * 256;                               // exchange bytes per point and round
static_assert(36 * W4H_XPT <= W4H_LDS, "the exchange reuses the stage buffers");
static_assert(QH::QPP * QH::RH * QH::RWP <= QH::NP * W4H_NW * 64, "the load pieces of the waves cover the halo");
constexpr unsigned W4H_KGB = W4_UKG * 4u;                      // filter bytes of one (co-tile, k-group)
}  // namespace

// value of point pl (0..5) and co sub-tile nt: slice o = pl / 3, p = 3 (pl % 3) + nt
// (W4B9, conv_wino4.h: slice o = the 12-wave layout's points 6w + 3o .. + 2)
__device__ __forceinline__ float w4h_bval(const W4B9& b, int pl, int nt) { return b.val(pl / 3, 3 * (pl % 3) + nt); }

// Barrier of the six waves of a half (DUAL): arrive = one ds_add on the half's counter, wait = poll it.  The LDS serves a
// wave's operations in order, so the wave's earlier LDS writes (and reads) are done when its add is; a wave that has seen
// the count issues its reads after the writers' adds.  ~150-250 cycles against s_barrier's tens -- the price of two
// independent instruction streams in one workgroup.
__device__ __forceinline__ void w4h_subbar(unsigned addr, unsigned& target, int lane) {
  target += (unsigned)W4H_NW;
  if (lane == 0) asm volatile("ds_add_u32 %0, %1" : : "v"(addr), "v"(1u) : "memory");
  for (;;) {
    unsigned v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    if ((int)((unsigned)__builtin_amdgcn_readfirstlane((int)v) - target) >= 0) break;
    __builtin_amdgcn_s_sleep(1);
  }
}

// ABL (probe builds): bit 6 s_memtime stamps of every wave (tools/wino4_clk.py), dumped into `res`.
// DUAL (conv_wino4d_kernel): ONE 12-wave workgroup hosts the two independent 6-wave blocks of a CU.  Two separate 6-wave
// workgroups of 168 VGPRs are never resident together: the dispatcher puts the waves of every workgroup on the SIMDs in the
// same cyclic order from the same start (2 / 2 / 1 / 1), and SIMDs 0 and 1 have room for three waves, not four (measured:
// profiles/r6_wino4h_timeline.txt -- 256 of 256 CUs ran their two blocks one after the other).  A 12-wave workgroup is
// placed 3 / 3 / 3 / 3; its halves (waves 0-5 / 6-11) have their own LDS image, their own items and their own barrier:
// s_barrier counts all 12 waves, so a half synchronises through a counter in LDS (w4h_subbar).
template <int ABL, bool DUAL>
__device__ __forceinline__ void w4h_body(const ConvArgs& a) {
  typedef QH Q;
  extern __shared__ float4 w4_smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = DUAL ? (wave_all >= W4H_NW ? 1 : 0) : 0;
  const int wave = wave_all - W4H_NW * half;
  const unsigned lds_wg = egn_lds_addr(w4_smem);
  const unsigned lds0 = lds_wg + (unsigned)(half * W4H_LDS);
  const float* smf = reinterpret_cast<const float*>(w4_smem) + half * (W4H_LDS / 4);
  // the halves' barrier counters (monotonic; zeroed below) behind the two LDS images
  const unsigned cnt_addr = lds_wg + (unsigned)(2 * W4H_LDS + 16 * half);
  unsigned bar_target = 0;
#define W4H_BAR()                                                  \
  {                                                                \
    if constexpr (DUAL) w4h_subbar(cnt_addr, bar_target, lane);    \
    else __builtin_amdgcn_s_barrier();                             \
  }
  const int li = lane & 15, kq = lane >> 4;
  const int tpart = wave >> 1;             // its third of the frequency rows of the input transform
  const int tg = wave & 1;                 // its k-group of the stage in the transform

  const int C = a.Cin, Co = a.Cout;
  const int nct = Co / W4_CO;
  const int S = C / 8;                     // stages of 8 channels

  const u32x4 rxv = egn_rsrc(a.x, (size_t)a.N * a.H * a.W * C * 4);
  const u32x4 ruv = egn_rsrc(a.w, (size_t)nct * (C >> 2) * W4_UKG * 4);
  const unsigned out_bytes = (unsigned)((size_t)a.N * a.Ho * a.Wo * Co * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, out_bytes, EGN_RSRC_WORD3);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res ? a.res : a.y), 0, out_bytes, EGN_RSRC_WORD3);

  // ---- halo loads: pieces wave, wave + 6; element e -> (pixel e / 2, channel quad e % 2), every lane to the natural slot
  // of its element (conv_wino4.h; PLANE = 100: the rows 18 / 19 fall on slots 90 .. 99); OOB offsets load zeros
  W4_HALO_SLOTS_NATURAL(W4H_NW, W4H_H0)
  // ---- transform share: lane (tile li, channel 4 tg + kq of the stage)
  const unsigned hb0 = lds0 + (unsigned)(W4H_H0 + ((2 * tg + (kq >> 1)) * Q::PAIR + Q::tileslot(li, 0)) * 8 + (kq & 1) * 4);
  const unsigned vw0 = lds0 + (unsigned)(W4H_V0 + tg * 256 + lane * 4);         // V[pt][g][lane]
  // ---- multiply: A operands V[6 wave + pl][g][lane]
  const float* va0 = smf + (W4H_V0 / 4) + (6 * wave) * (Q::VPT / 4) + lane;
  const unsigned uvo = (unsigned)lane * 16u;

  const int regs_x = a.tiles_x, regs_xy = a.tiles_x * a.tiles_y;
  const int nreg = regs_xy * a.N;
  const int imode = w4_item_mode(nct);
  const int nwork = w4_item_count(imode, nreg, nct, 1);
  const int gsz = __builtin_amdgcn_readfirstlane((int)gridDim.x);
  const float act_lo = (a.act & EGN_ACT_MASK) == EGN_ACT_RELU ? 0.f : -__builtin_inff();
  const bool has_res = (ABL & 64) ? false : a.res != nullptr;
  const unsigned rowpitch = (unsigned)(a.Wo * Co) * 4u, colpitch = (unsigned)Co * 4u;

  W4_STAMPS(128, DUAL ? 2 * W4H_LDS + 64 : W4H_LDS, wave_all)
  W4_CLK()
  // ---- phase skew: the block whose LDS allocation does not start at 0 shares its CU with an older block
  const unsigned lds_base = __builtin_amdgcn_s_getreg((12 - 1) << 11 | 0 << 6 | 6) & 0xfffu;      // HW_REG_LDS_ALLOC: LDS_BASE
  if constexpr (DUAL) {
    if (tid < 8) reinterpret_cast<unsigned*>(reinterpret_cast<char*>(w4_smem) + 2 * W4H_LDS)[tid] = 0u;
    __syncthreads();             // (the only workgroup barrier of the kernel body)
  }
  if (a.spix_off > 0 && (DUAL ? half != 0 : lds_base != 0u)) {
    const unsigned long long t0 = __builtin_readcyclecounter();
    const unsigned long long d = (unsigned long long)a.spix_off * 64ull;
    while (__builtin_readcyclecounter() - t0 < d) __builtin_amdgcn_s_sleep(8);
  }
  W4_CLK()
  // DUAL: the second halves are blocks gsz .. 2 gsz - 1 of a virtual grid (gsz is a multiple of 8: the same XCD)
  for (int w = blockIdx.x + half * gsz; w < nwork; w += (DUAL ? 2 : 1) * gsz) {
    const unsigned wi = (unsigned)__builtin_amdgcn_readfirstlane(w);
    W4_ITEM_DECODE(wi, 1, nct, reg, ct, ks_)
    if (reg >= nreg) continue;
    const W4Region rg_ = w4_item_region<3>(a, reg, regs_x, regs_xy);
    const int n = rg_.n, y0 = rg_.y0, x0 = rg_.x0;
    // halo offsets of the item: recomputed from the lane id per item (not kept over the K loop: registers)
    W4_HALO_DOFF(W4H_NW)
    // filter of this wave: k-group h = [ct][h][12-wave slice 2w, 2w + 1][3 x dwordx4 per lane] -- 6 KB in a row.
    // Raw ISA: the waits are mine (tools/check_wino4_isa.py)
    const unsigned ubase = (unsigned)(ct * (C >> 2)) * W4H_KGB + (unsigned)wave * (6u * 64u * 16u);
#define W4_LOADB(DST, HS) w4_loadB(DST, ruv, uvo, HS, 3072u);   /* HS: byte offset of the k-group, W4_PAST = none */
    W4B9 b0, b1;
    f32x4 hreg[Q::NP];
    W4_PROLOGUE(W4_LOADB(b0, ubase), W4H_BAR())

    f32x4 acc[6][3];
#pragma unroll
    for (int pl = 0; pl < 6; ++pl)
#pragma unroll
      for (int nt = 0; nt < 3; ++nt) acc[pl][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // 18 MFMAs of a k-group in three groups of 6 (two frequency points each); H0 / H1 / H2: the vector-memory
    // instruction issued behind each group (conv_wino4.hip: spread, not a burst behind the barrier)
#define W4_MUL6(J, B)                                                                                          \
  _Pragma("unroll") for (int x_ = 0; x_ < 2; ++x_) _Pragma("unroll") for (int nt = 0; nt < 3; ++nt)            \
      acc[2 * (J) + x_][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_[2 * (J) + x_], w4h_bval(B, 2 * (J) + x_, nt), \
                                                                   acc[2 * (J) + x_][nt], 0, 0, 0);
#define W4_MUL(P, G, B, H0, H1, H2)                                                                            \
  {                                                                                                            \
    float av_[6];                                                                                              \
    _Pragma("unroll") for (int pl = 0; pl < 6; ++pl)                                                           \
        av_[pl] = va0[((P) ? W4H_VBYTES / 4 : 0) + pl * (Q::VPT / 4) + (G)*64];                                \
    W4_MUL6(0, B) __builtin_amdgcn_sched_barrier(0); H0 __builtin_amdgcn_sched_barrier(0);                     \
    W4_MUL6(1, B) __builtin_amdgcn_sched_barrier(0); H1 __builtin_amdgcn_sched_barrier(0);                     \
    W4_MUL6(2, B) __builtin_amdgcn_sched_barrier(0); H2 __builtin_amdgcn_sched_barrier(0);                     \
  }
    // Stage s (parity P): k-groups 2s, 2s+1 (conv_wino4.hip's GEO 0 stage with one m-tile and six points per wave)
#define W4_STAGE(P, SI)                                                                                        \
  {                                                                                                            \
    const int s_ = (SI);                                                                                       \
    const unsigned dst_ = s_ + 2 < S ? (unsigned)(s_ + 2) * (unsigned)Q::SBYTES : W4_PAST;                     \
    const unsigned u0_ = ubase + (unsigned)(2 * s_) * W4H_KGB;                                                 \
    const unsigned bn_ = s_ + 1 < S ? u0_ + 2u * W4H_KGB : W4_PAST;                                            \
    w4_vm_landedB(b0);                                                                                        \
    W4_CLK() /* 0: k-group 2s landed */                                                                        \
    W4_TRANS(P, 0)                                                                                             \
    W4_LOADB(b1, u0_ + W4H_KGB)                                                                                \
    W4_CLK() /* 1: (transform third 0 +) loads issued */                                                       \
    W4_MUL(P, 0, b0, , , )                                                                                     \
    W4_CLK() /* 2: k-group 0 multiplies issued */                                                              \
    w4_vm_landedB(b1);                                                                                        \
    W4_CLK() /* 3: k-group 2s+1 landed */                                                                      \
    W4_TRANS(P, 1)                                                                                             \
    W4_LOADB(b0, bn_)                                                                                          \
    W4_MUL(P, 1, b1, W4_HLOAD(0, dst_), W4_HLOAD(1, dst_), )                                                   \
    W4_TRANS(P, 2)                                                                                             \
    W4_CLK() /* 4: (transform third 1 +) k-group 1 multiplies issued (+ transform third 2) */                  \
    w4_vm_landedH(hreg);             /* the pieces of stage s + 2 and k-group 2s+2 */                          \
    W4_HSTORE(P)                                                                                               \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                         \
    W4_CLK() /* 5: own pieces of stage s + 2 in LDS, V writes done */                                          \
    W4H_BAR()                                                                              \
    asm volatile("" ::: "memory");                                                                             \
    W4_CLK() /* 6: past the barrier */                                                                         \
  }
    for (int s = 0; s + 1 < S; s += 2) {     // (S is even: Cin % 16 == 0)
      W4_STAGE(0, s)
      W4_STAGE(1, s + 1)
    }
    // the loads past the end: tied to the wait (conv_wino4.hip)
    w4_vm_landedB(b0);
    w4_vm_landedB(b1);
    w4_vm_landedH(hreg);
    W4_CLK()      /* K loop done */
#undef W4_STAGE
#undef W4_MUL
#undef W4_MUL6
#undef W4_LOADB

    // ---- item end.  Unit U = 4 nt + kq (a quarter C fragment: tiles 4 kq .. 4 kq + 3 x 16 channels of sub-tile nt);
    // round r holds units 6 r .. 6 r + 5 at [point][U - 6 r][writer lane li] float4; reader wave rw takes unit 6 r + rw.
    // Addresses from an opaque copy of the lane id: computed here, not held in registers over the K loop.
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int li_e = lane_e & 15, kq_e = lane_e >> 4;
    const unsigned xhi = (unsigned)(li_e >> 3);
    // writer: slot of (nt, kq) in its round; li >= 8 stores its float4 rotated by two dwords (conv_wino4.h: the reader
    // takes one dword of 16 writer slots -- li and li + 8 would share a bank)
    const unsigned xw_ = lds0 + (unsigned)((6 * wave) * W4H_XPT + li_e * 16);
    const unsigned xw_n0 = xw_ + (unsigned)(kq_e * 256);                              // nt 0: round 0, units 0..3
    const unsigned xw_n1 = xw_ + (unsigned)((kq_e < 2 ? 4 + kq_e : kq_e - 2) * 256);  // nt 1: round 0 units 4, 5 | round 1 units 0, 1
    const unsigned xw_n2 = xw_ + (unsigned)((2 + kq_e) * 256);                        // nt 2: round 1, units 2..5
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int U = 6 * r + wave;                       // this wave's unit as a reader
      const int nt_r = U >> 2, kq_w = U & 3;
      const int tile = 4 * kq_w + kq_e;
      const int ty = tile >> 2, tx = tile & 3;
      const int cch = ct * W4_CO + nt_r * 16 + li_e;
      const float sc = a.scale[cch];
      const float sh = a.shift[cch];
      const unsigned vo = (unsigned)((((n * a.Ho + y0 + 4 * ty) * a.Wo + x0 + 4 * tx) * Co + cch) * 4);
      const unsigned xr0 = lds0 + (unsigned)(wave * 256 + li_e * 16) + (((unsigned)kq_e + 2u * xhi) & 3u) * 4u;
      float rv[4][4];
      W4_RES_LOAD(rv, has_res ? vo : EGN_OOB)
#define W4_XWH(ADDR, PL, V) w4_xw<(PL)*W4H_XPT>((ADDR) + 8u * xhi, (ADDR) + 8u - 8u * xhi, V);
#define W4_XW6(ADDR, NT) W4_XWH(ADDR, 0, acc[0][NT]) W4_XWH(ADDR, 1, acc[1][NT]) W4_XWH(ADDR, 2, acc[2][NT])    \
                         W4_XWH(ADDR, 3, acc[3][NT]) W4_XWH(ADDR, 4, acc[4][NT]) W4_XWH(ADDR, 5, acc[5][NT])
      if (r == 0) {
        W4_XW6(xw_n0, 0)
        if (kq_e < 2) { W4_XW6(xw_n1, 1) }
      } else {
        if (kq_e >= 2) { W4_XW6(xw_n1, 1) }
        W4_XW6(xw_n2, 2)
      }
#undef W4_XW6
#undef W4_XWH
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xC07F);
      W4_CLK()    /* round: accumulators written */
      W4H_BAR()
      asm volatile("" ::: "memory");
      W4_CLK()    /* round: exchange barrier passed */
      float yc[4][6];
      W4_XREAD_COLS(W4H_XPT)
      W4_ROWS_STORE()
      asm volatile("" ::: "memory");
      W4_CLK()    /* round: output transform done, stores issued */
      W4H_BAR()      // the exchange buffer is free again (next round / next item's halo)
      asm volatile("" ::: "memory");
      W4_CLK()    /* round: end */
    }
  }
  if constexpr ((ABL & 64) != 0) {
    unsigned long long* out = w4_stamp_dump<(DUAL ? 2 * W4H_NW : W4H_NW), W4_NTK, 2>(a, sT, ntk, tid);
    if (tid == 0) out[1] = ((unsigned long long)lds_base << 32) | ((unsigned long long)(__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 0xfu) << 16) |
                           (__builtin_amdgcn_s_getreg((16 - 1) << 11 | 0 << 6 | 4) & 0xffffu);      /* LDS base | XCC_ID | HW_ID */
  }
#undef W4H_BAR
}

template <int ABL>
__global__ __launch_bounds__(W4H_NTH, 3) void conv_wino4h_kernel(ConvArgs a) { w4h_body<ABL, false>(a); }
template <int ABL>
__global__ __launch_bounds__(2 * W4H_NTH, 1) void conv_wino4d_kernel(ConvArgs a) { w4h_body<ABL, true>(a); }

bool egn_conv_wino4h_applies(const ConvArgs& a) {
  return egn_plain_3x3_s1(a) && a.Cin % 16 == 0 && a.Cout % W4_CO == 0 && a.Ho % 16 == 0 && a.Wo % 16 == 0;
}
// (+ the stamp area of the ABL & 64 build); dual: both halves' images + their barrier counters
size_t egn_conv_wino4h_lds_bytes(int dual) { return dual ? 2 * W4H_LDS + 64 + 12 * 128 * 8 : W4H_LDS + 6 * 128 * 8; }

#ifdef EGN_PROBES
// start delay of a CU's second block in units of 64 cycles (EGN_W4H_SKEW overrides: probes)
static int w4h_default_skew() {
  static int skew = -1;
  if (skew < 0) {
    const char* e = getenv("EGN_W4H_SKEW");
    skew = e ? atoi(e) : 0;
    if (skew < 0) skew = 0;
  }
  return skew;
}
#endif

#ifdef EGN_PROBES
template <int ABL, bool DUAL>
static int wino4h_launch(ConvArgs a, size_t lds, hipStream_t stream) {
  static bool raised[EGN_MAX_DEVICES];
  void (*kern)(ConvArgs) = DUAL ? &conv_wino4d_kernel<ABL> : &conv_wino4h_kernel<ABL>;
  EGN_CHECK_HIP(egn_allow_big_lds(kern, DUAL ? EGN_BIG_LDS_BYTES : 80 * 1024, raised));
  const int nct = a.Cout / W4_CO;
  const int nwork = w4_item_setup(a, nct, 1, a.tiles_x * a.tiles_y * a.N);
  if (nwork < 0) return nwork;
  a.spix_off = w4h_default_skew();
  // (DUAL: a workgroup's halves take items w and w + grid: half as many workgroups as items fill both halves)
  const int want = DUAL ? (nwork / 2 + 8 * nct - 1) / (8 * nct) * (8 * nct) : nwork;
  // blocks per CU: two 6-wave workgroups, or one 12-wave workgroup with two halves; whole XCD rounds of co-tiles
  const int grid = egn_persistent_grid(want, 8 * nct, DUAL ? 1 : 2);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(DUAL ? 2 * W4H_NTH : W4H_NTH), lds, stream, a);
  return (int)hipGetLastError();
}
#endif
// Probe builds only (python -m egonet_amd.build --probes): both forms measured SLOWER than conv_wino4_kernel on the layer
// they were built for (profiles/r6_wino4h_timeline.txt, r6_wino4d_timeline.txt) -- the product library does not compile them.
int egn_conv_launch_wino4h(ConvArgs a, size_t lds, int abl, int dual, hipStream_t stream) {
#ifdef EGN_PROBES
  if (!egn_conv_wino4h_applies(a)) return EGN_E_BADARG;
  switch (abl) {
    case 0: return dual ? wino4h_launch<0, true>(a, lds, stream) : wino4h_launch<0, false>(a, lds, stream);
    case 64: return dual ? wino4h_launch<64, true>(a, lds, stream) : wino4h_launch<64, false>(a, lds, stream);
    default: return EGN_E_BADARG;
  }
#else
  (void)a; (void)lds; (void)abl; (void)dual; (void)stream;
  return EGN_E_BADARG;
#endif
}
