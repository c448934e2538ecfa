// conv_h.hip -- the opt-in f16-OPERAND family: a direct (implicit-GEMM) 3x3 / stride 1 / pad 1 convolution on
// v_mfma_f32_16x16x32_f16 with fp32 accumulators (precision = 'f16', DESIGN "f16-operand mode").  It lives BESIDE the
// config table and the tuner (no kConfigs row, no filter kind of theirs): egn_conv3x3_h_applies is the one predicate.
//
// Activations stay fp32 NHWC in HBM -- except a tensor between two ops of this family that activations = 'f16' stores as f16
// (ConvHArgs::x16 / y16, DESIGN 3.16d: the producer applies h_round_f16, the reader stages the f16 as it lies; the same
// operand bits).  A block owns TM output pixels (TNB images x TH x TW, all powers of two, so a map
// smaller than 8 x 8 packs several images into the tile) x TN output channels.  The input channels are walked in chunks
// of 48: per chunk the block stages the halo tile [TNB][TH+2][TW+2][48] into LDS, converting fp32 -> f16 on the way
// (clamp to +-65504, then the compiler's v_cvt_pk_f16_f32 under the default mode: round-to-nearest-even -- not the
// truncating v_cvt_pkrtz_f16_f32 --, saturating, never inf), and
// runs the chunk's K = 9 * 48 = 432 products.
// K choice: K is FLATTENED per chunk (k = 48 * tap + c) and zero-padded 432 -> 448 = 14 steps of 32.  A lane's fragment
// (8 consecutive k) lies inside one tap because 48 % 8 == 0, so it is ONE 16-byte LDS read of 8 channels of one halo
// pixel; the two fragments past k = 432 are zeros on both sides (the A side reads 16 zero bytes kept in LDS).
//   A (pixels):  lane l holds A[row l & 15][k = 8 (l >> 4) + j], j = 0..7     -- from LDS
//   B (filter):  lane l holds B[k = 8 (l >> 4) + j][col l & 15]               -- straight from HBM / L2, 16 B per lane,
//                pre-packed by engine.pack_conv_weight_f16: [Cout/16][Cin/48][14 steps][64 lanes][8] f16
//   C/D:         col = l & 15 (output channel), row = 4 (l >> 4) + r (pixel)
// Epilogue (the project's): acc * scale + shift, + residual, ReLU / none, through LDS to float4 along the channel axis,
// 16-byte buffer stores; out-of-range pixels get the OOB offset (loads 0, drops the store), as conv_common.h does.
// No BatchNorm statistics, no ticket words, no K split.
//
// STRIDE 2 (precision = 'f16s2', egn_conv3x3s2_h_applies) is the same kernel with S = 2: the same filter pack (its layout
// does not know the stride), the same chunks, K steps, staging and epilogue (no residual: no stride-2 layer has one).  A
// TH x TW output tile (8 x 8, 64 pixels, for both channel tiles; at least 2 x 2) brings a (2 TH + 1) x (2 TW + 1) halo, 1.13x
// its input pixels at 8 x 8, and the A fragment of output pixel (oy, ox) and tap (ky, kx) is halo pixel (2 oy + ky, 2 ox + kx).
// Bank arithmetic (ds_read_b128: a 16-byte quad q = (address / 16) % 16, the 16 rows of a fragment read must hit 16 quads;
// a pixel is 7 quads).  Stride 1: row li of a fragment is pixel x = li, quad 7 li: 16 different ones.  Stride 2 read the
// same way: halo pixel 2 li, quad 14 li -- even quads only, every one twice.  So
//   1. a halo row is stored SPLIT BY COLUMN PARITY: the TW + 1 even columns, then the TW odd ones.  Tap kx of output
//      column x is then entry (kx & 1) (TW + 1) + (kx >> 1) + x of the row: consecutive x are consecutive entries, 7 quads
//      apart, as at stride 1 (x = 0..7: quads 0 7 14 5 12 3 10 1);
//   2. the two tile rows inside a 16-row fragment (TW = 8) are y and y + TH / 2, not y and y + 1 (h_tile_row): 2 * 4 halo
//      rows x 17 pixels x 7 quads = 952 = 8 (mod 16), the other eight quads (8 15 6 13 4 11 2 9).  Rows y and y + 1 would be
//      2 x 17 x 7 = 238 = 14 (mod 16) apart and collide on six of the eight.
// Both hold for the tiles HRNet-W48 has (outputs of 8 x 8 and more); smaller tiles are correct, not conflict-free.  (The
// arithmetic is per channel group, as at stride 1: the hardware's 16-lane groups of a ds_read_b128 mix two of them.)
//
// CHUNKS OF 32 (precision = 'f16x', egn_conv3x3_hx_applies; template parameter CK = 32) run the widths 48 does not
// divide: Cin in {32, 64, 128, 256}, either stride.  K per chunk is 9 * 32 = 288 = 9 steps of 32 exactly: K step ks IS tap
// ks and lane group g IS channel group g, so there is no K-step table, no padding branch and no zero bytes; the filter
// pack is engine.pack_conv_weight_f16x: [Cout/16][Cin/32][9 taps][64 lanes][8] f16.  A halo pixel is 64 bytes of f16
// stored with an 80-byte stride, 5 quads, and the arguments above carry over: stride 1, fragment row li reads quad
// 5 li mod 16 (0 5 10 15 4 9 14 3 8 13 2 7 12 1 6 11); stride 2 with the parity-split row, x = 0..7: quads 0 5 10 15 4 9 14 3,
// and tile row y + TH / 2 is 8 * 17 * 5 = 680 = 8 (mod 16) away: the other eight.  Output-channel tiles: 64 (Cout = 64 /
// 128 / 256, 2 x 2 waves on 64 pixels) and 32 (4 x 1 waves on 128 pixels, stride 2: 64), beside 96 / 48 for 256 -> 96 / 48.
#include <string.h>

#include <atomic>

#include "conv_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// What follows from the input-channel chunk CK (48: the W48 widths; 32: the 32-multiple widths, 'f16x').
template <int CK>
struct ConvHChunk {
  static_assert(CK == 48 || CK == 32, "chunks of 48 or 32 input channels");
  static constexpr int KS = (9 * CK + 31) / 32;   // MFMA K steps per chunk: 14 (432 -> 448) or 9 (288, no padding)
  static constexpr int PIXB = 2 * CK + 16;        // LDS bytes per halo pixel: 112 / 80 (a 7- / 5-quad stride: 16 neighbouring
                                                  // pixels hit 16 bank quads)
  static constexpr int TAB = CK == 48 ? 16 + KS * 4 * 4 : 0;   // CK = 48: 16 zero bytes and the K-step offsets behind sOff
};
constexpr int H_CK = 48;      // input channels per chunk of the 'f16' / 'f16s2' instances
constexpr int H_KS = ConvHChunk<48>::KS;
constexpr float H_F16_MAX = 65504.0f;

// THE rounding of an activation to f16: clamp to +-65504, then round to nearest even.  The fp32 staging applies it to what
// it loads and the f16 epilogue (ConvHArgs::y16) to what it stores, so a tensor stored as f16 holds the very bits its
// reader would have put into LDS.
__device__ __forceinline__ _Float16 h_round_f16(float v) {
  return (_Float16)__builtin_fminf(__builtin_fmaxf(v, -H_F16_MAX), H_F16_MAX);
}

// 8 bytes per lane at voff (a vector store: out-of-range offsets drop it)
__device__ __forceinline__ void egn_buf_store8(__amdgpu_buffer_rsrc_t r, unsigned voff, u32x2 v) {
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, 0, 0);
}

// a 16-byte B fragment: lane offset in a VGPR, wave-uniform offset in an SGPR (non-template wrapper, as conv_common.h's)
__device__ __forceinline__ f16x8 h_load_b(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
  return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

template <int WM, int WN, int MT, int NT>
struct ConvHTile {
  static constexpr int TM = WM * MT * 16, TN = WN * NT * 16;
  static constexpr int SC_LD = NT * 16 + 4;                         // floats per row of a wave's epilogue slab
  static constexpr int EPI_BYTES = WM * WN * MT * 16 * SC_LD * 4;
  // the next chunk's batch 0 in flight during the products: not for the 48-output-channel tile, whose layers in HRNet have
  // one chunk (48 -> 48) and whose staging registers, live across the products, would cost it a wave per SIMD
  // (the same holds for the stride-2 64 x 48 tile)
  // (CK = 32: the 64-channel tile prefetches too; the 32-channel tile's layers have one chunk)
  static constexpr bool PREFETCH = TN == 96 || TN == 64;
};

// Staging items (16 bytes: 4 fp32 or 8 f16 channels of one halo pixel) a thread holds per batch.
//   fp32 input: stride 1, 5 * 256 covers the 100-pixel halo of an 8 x 8 tile at CK = 48; stride 2, the 289-pixel halo of an
//   8 x 8 tile is 13.5 items per thread: two batches of 7 (two round trips to memory, not three; one batch of 14 spills).
//   f16 input (X16): half the items.  Stride 1: 100 pixels are 600 items at CK = 48 (3 per thread) and 400 at CK = 32 (2);
//   stride 2: 289 pixels are 1734 (one batch of 7) and 1156 (one batch of 5).
template <int CK, int S, bool X16>
struct ConvHStage {
  static constexpr int SB = !X16 ? (S == 1 ? 5 : 7) : (S == 1 ? (CK == 48 ? 3 : 2) : (CK == 48 ? 7 : 5));
  static constexpr int CPI = X16 ? 8 : 4;       // channels per item
  static constexpr int EB = X16 ? 2 : 4;        // bytes per element of x
};

// Stride 2: the row bits of a tile row index, rotated right by one.  The 16 rows of an A fragment are then 8 columns of
// the tile rows y and y + TH / 2 instead of y and y + 1 (the bank arithmetic in the header); a bijection on [0, TH).
template <int S>
__device__ __forceinline__ int h_tile_row(int r, int lth) {
  return S == 1 || lth == 0 ? r : (r >> 1) | ((r & 1) << (lth - 1));
}

// X16: x is stored as f16 (the bits h_round_f16 gives): an item is 8 channels, one 16-byte load and one 16-byte LDS write,
// no conversion.  The LDS layout, the fragment reads and the products do not know the difference.
template <int CK, int S, int WM, int WN, int MT, int NT, bool X16>
__global__ __launch_bounds__(256, 4) void conv_h_kernel(const ConvHArgs a) {
  using T = ConvHTile<WM, WN, MT, NT>;
  using G = ConvHStage<CK, S, X16>;
  constexpr int H_CK = CK, H_KS = ConvHChunk<CK>::KS, H_PIXB = ConvHChunk<CK>::PIXB;
  static_assert(WM * WN == 4, "four waves");
  constexpr int SB = G::SB, CPI = G::CPI, EB = G::EB;
  extern __shared__ float4 smem_f4[];
  char* smem = reinterpret_cast<char*>(smem_f4);
  unsigned* sOff = reinterpret_cast<unsigned*>(smem);        // [npix] byte offset of halo pixel (channel 0) in x, or EGN_OOB
  int* sKoff = reinterpret_cast<int*>(smem + a.tab_bytes - H_KS * 4 * 4);   // CK = 48: the last 224 bytes of the table region
  char* slab = smem + a.tab_bytes;                            // [npix][H_PIXB] f16 halo tile; later the epilogue slabs

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 15, g = lane >> 4;

  const int nct = a.Cout / T::TN;
  const int ct = blockIdx.x % nct;
  int tile = blockIdx.x / nct;
  const int tx = tile % a.tiles_x;
  tile /= a.tiles_x;
  const int ty = tile % a.tiles_y;
  const int n_base = (tile / a.tiles_y) * a.TNB;
  const int oy0 = ty * a.TH, ox0 = tx * a.TW;
  const int px_mask = (1 << (a.lth + a.ltw)) - 1;

  for (int p = tid; p < a.npix; p += 256) {
    const int b = p / (a.HH * a.HW);
    const int rem = p - b * (a.HH * a.HW);
    const int hy = rem / a.HW;
    const int col = rem - hy * a.HW;
    const int hx = S == 1 ? col : (col <= a.TW ? 2 * col : 2 * (col - a.TW) - 1);   // stride 2: even columns first
    const int n = n_base + b, iy = S * oy0 + hy - 1, ix = S * ox0 + hx - 1;
    const bool ok = n < a.N && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    sOff[p] = ok ? (unsigned)((n * a.H + iy) * a.W + ix) * (unsigned)(a.Cin * EB) : EGN_OOB;
  }

  // per lane: LDS byte offset of the top-left tap of its MT tile rows, and per K step the offset of its 8 channels
  int abase[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = (wm * MT + mt) * 16 + li;
    const int b = m >> (a.lth + a.ltw);
    const int rem = m & px_mask;
    const int y = h_tile_row<S>(rem >> a.ltw, a.lth), x = rem & (a.TW - 1);
    abase[mt] = a.tab_bytes + ((b * a.HH + S * y) * a.HW + x) * H_PIXB;      // from smem
  }
  // sKoff[4 ks + g]: LDS byte offset of the 8 channels a lane of group g reads at K step ks (tap and channel group of
  // k = 8 (4 ks + g)); -1 past k = 432.  A table in LDS, not 14 registers per lane: the kernel keeps 4 waves per SIMD.
  // CK = 32: K step ks IS tap ks and lane group g IS channel group g -- no table, nothing past K, no zero bytes.
  const int zoff = a.tab_bytes - H_KS * 4 * 4 - 16;   // 16 zero bytes: the A fragment of the padding steps, read without a branch
  if constexpr (CK == 48) {
    if (tid < 4) reinterpret_cast<int*>(smem + zoff)[tid] = 0;
    if (tid < H_KS * 4) {
      const int tap = tid / 6, c8 = tid - tap * 6;
      const int ky = tap / 3, kx = tap - ky * 3;
      const int kcol = S == 1 ? kx : (kx & 1) * (a.TW + 1) + (kx >> 1);   // stride 2: halo column 2 x + kx of the split row
      sKoff[tid] = tid < 54 ? (ky * a.HW + kcol) * H_PIXB + c8 * 16 : -1;
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) abase[mt] += g * 16;
  }

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x), 0, (unsigned)((size_t)a.N * a.H * a.W * a.Cin * EB), EGN_RSRC_WORD3);
  const int nchunk = a.Cin / H_CK;
  const int nstage = a.npix * (H_CK / CPI);   // 16-byte items of a chunk's halo tile
  // B fragments: [cout tile][chunk][step][lane] x 16 bytes -- one lane offset in a register, the rest is wave-uniform
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(a.w), 0, (unsigned)((a.Cout / 16) * nchunk * (H_KS * 1024)), EGN_RSRC_WORD3);
  const unsigned wlane = lane * 16;
  int wb[NT];      // byte offset of (cout tile, chunk 0, step 0)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wb[nt] = (ct * (T::TN / 16) + wn * NT + nt) * nchunk * (H_KS * 1024);

  // Staging of a chunk's halo tile, SB items per thread and batch: all loads of a batch are issued before the first
  // is converted, and (T::PREFETCH) batch 0 of the NEXT chunk is issued before the current chunk's products, so its HBM latency
  // hides behind them (an 8 x 8 tile is one batch, 8 x 16 two; tiles of many tiny images have more).
  f32x4 sv[SB];
  auto stage_load = [&](int chunk, int batch) {
#pragma unroll
    for (int j = 0; j < SB; ++j) {
      const int idx = (batch * SB + j) * 256 + tid;
      const int p = idx / (H_CK / CPI);
      const int ci = idx - p * (H_CK / CPI);
      const unsigned off = idx < nstage ? sOff[p] : EGN_OOB;
      sv[j] = egn_buf_load16(rx, off == EGN_OOB ? EGN_OOB : off + (unsigned)(chunk * H_CK + ci * CPI) * (unsigned)EB);
    }
  };
  auto stage_store = [&](int batch) {
#pragma unroll
    for (int j = 0; j < SB; ++j) {
      const int idx = (batch * SB + j) * 256 + tid;
      const int p = idx / (H_CK / CPI);
      const int ci = idx - p * (H_CK / CPI);
      const f32x4 v = sv[j];
      if constexpr (X16) {       // 8 f16 channels as they lie: 16 bytes at a 16-byte aligned address (H_PIXB % 16 == 0)
        if (idx < nstage) *reinterpret_cast<f32x4*>(slab + p * H_PIXB + ci * 16) = v;
      } else {
        f16x4 h;
        h.x = h_round_f16(v.x);
        h.y = h_round_f16(v.y);
        h.z = h_round_f16(v.z);
        h.w = h_round_f16(v.w);
        if (idx < nstage) *reinterpret_cast<f16x4*>(slab + p * H_PIXB + ci * 8) = h;
      }
    }
  };
  const int nbatch = (nstage + SB * 256 - 1) / (SB * 256);
  __syncthreads();   // sOff is written
  if (T::PREFETCH) stage_load(0, 0);
  // Filter fragments in flight: two K steps; FOUR for the stride-2 64 x 48 tile, whose 3 MFMAs per step hide nothing of an
  // L2 round trip -- its layers (48 -> 48, one chunk, small grids) are bound by the block's latency, so the first ones are
  // also issued before the halo is staged and travel beside it.
  constexpr int BD = S == 2 && MT == 1 ? 4 : 2;
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    f16x8 bf[BD][NT];
    auto b_preload = [&]() {
#pragma unroll
      for (int d = 0; d < BD - 1; ++d)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[d][nt] = h_load_b(rw, wlane, wb[nt] + chunk * (H_KS * 1024) + d * 1024);
    };
    if (BD > 2) b_preload();
    if (chunk) __syncthreads();   // the previous chunk's fragment reads are done
    if (!T::PREFETCH) stage_load(chunk, 0);
    stage_store(0);
    for (int b = 1; b < nbatch; ++b) {
      stage_load(chunk, b);
      stage_store(b);
    }
    __syncthreads();
    if (T::PREFETCH && chunk + 1 < nchunk) stage_load(chunk + 1, 0);

    if (BD == 2) b_preload();
#pragma unroll
    for (int ks = 0; ks < H_KS; ++ks) {
      if (ks + BD - 1 < H_KS) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          bf[(ks + BD - 1) % BD][nt] = h_load_b(rw, wlane, wb[nt] + chunk * (H_KS * 1024) + (ks + BD - 1) * 1024);
      }
      f16x8 af[MT];
      if constexpr (CK == 48) {
        const int koff = sKoff[ks * 4 + g];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const f16x8*>(smem + (koff >= 0 ? abase[mt] + koff : zoff));
      } else {
        const int ky = ks / 3, kx = ks - ky * 3;     // compile-time; the offset is wave-uniform
        const int kcol = S == 1 ? kx : (kx & 1) * (a.TW + 1) + (kx >> 1);
        const int koff = (ky * a.HW + kcol) * H_PIXB;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const f16x8*>(smem + abase[mt] + koff);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf[ks % BD][nt], acc[mt][nt], 0, 0, 0);
    }
  }

  // ---- epilogue: accumulators -> the wave's LDS slab -> float4 along the channel axis ----
  __syncthreads();   // every wave is done with the halo tile
  float* sC = reinterpret_cast<float*>(slab) + wave * (MT * 16) * T::SC_LD;
  const int cbase = ct * T::TN + wn * NT * 16;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float sc = a.scale[cbase + nt * 16 + li];
    const float sh = a.shift[cbase + nt * 16 + li];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sC[(mt * 16 + g * 4 + r) * T::SC_LD + nt * 16 + li] = acc[mt][nt][r] * sc + sh;
  }
  __syncthreads();
  const unsigned ybytes = (unsigned)((size_t)a.N * a.Ho * a.Wo * a.Cout * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, ybytes, EGN_RSRC_WORD3);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res ? a.res : a.y), 0, ybytes, EGN_RSRC_WORD3);
  const __amdgpu_buffer_rsrc_t ry16 = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, ybytes / 2, EGN_RSRC_WORD3);   // y as f16
  constexpr int C4 = NT * 4;   // float4 per slab row
#pragma unroll
  for (int it = 0; it < MT * NT; ++it) {
    const int idx = it * 64 + lane;
    const int row = idx / C4;
    const int c4 = idx - row * C4;
    const int m = wm * MT * 16 + row;
    const int b = m >> (a.lth + a.ltw);
    const int rem = m & px_mask;
    const int n = n_base + b, oy = oy0 + h_tile_row<S>(rem >> a.ltw, a.lth), ox = ox0 + (rem & (a.TW - 1));
    const bool ok = n < a.N && oy < a.Ho && ox < a.Wo;
    const unsigned eoff = (unsigned)(((n * a.Ho + oy) * a.Wo + ox) * a.Cout + cbase + c4 * 4);   // in elements
    const unsigned voff = ok ? eoff * 4u : EGN_OOB;
    f32x4 v = *reinterpret_cast<const f32x4*>(&sC[row * T::SC_LD + c4 * 4]);
    if (a.res) v += egn_buf_load16(rr, voff);
    if (a.act == EGN_ACT_RELU) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if (a.y16) {     // (wave-uniform) f16 storage: the reader's rounding applied here, 8 bytes per lane; never with a residual
      f16x4 h;
      h.x = h_round_f16(v.x);
      h.y = h_round_f16(v.y);
      h.z = h_round_f16(v.z);
      h.w = h_round_f16(v.w);
      egn_buf_store8(ry16, ok ? eoff * 2u : EGN_OOB, __builtin_bit_cast(u32x2, h));
    } else {
      egn_buf_store16(ry, voff, v);
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static bool h_width(int c) { return c == 48 || c == 96 || c == 192 || c == 384; }
static int h_pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
static int h_log2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// 'f16x': the 32-multiple widths, walked in chunks of 32 (K step = tap, lane group = channel group; the header).
static bool hx_cin(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }
static bool hx_cout(int c) { return hx_cin(c) || c == 48 || c == 96; }
// the width classes of a chunk size: one clause per chunk size, here alone
static bool h_widths(int ck, int Cin, int Cout) {
  return ck == 48 ? h_width(Cin) && h_width(Cout) : ck == 32 && hx_cin(Cin) && hx_cout(Cout);
}

// THE predicate of the family, per chunk size `ck`: 1 where its instances run the layer (input N x H x W, output
// (H - 1) / stride + 1 x (W - 1) / stride + 1).  ck = 48: the W48 widths; ck = 32: Cin in {32, 64, 128, 256}, Cout in those or
// {48, 96} (transition1's 256 -> 48 / 256 -> 96).  Unpadded channel strides, a plain epilogue (scale / shift, optional
// residual added before the activation, ReLU or none; no stride-2 layer of HRNet has a residual), stride 1 or 2, tensors
// below 2 GiB (32-bit buffer offsets).
static int h_applies(int ck, int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act, int stride) {
  if (N < 1 || H < 2 || W < 2 || !h_widths(ck, Cin, Cout) || cs_in != Cin || cs_out != Cout) return 0;
  if (act != EGN_ACT_NONE && act != EGN_ACT_RELU) return 0;     // (sigmoid, leaky and RES_AFTER stay on the fp32 kernels)
  if (stride != 1 && stride != 2) return 0;
  if (has_res != 0 && (has_res != 1 || stride == 2)) return 0;
  const long long pxo = (long long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  if ((long long)N * H * W * Cin * 4 >= (1ll << 31) || pxo * Cout * 4 >= (1ll << 31)) return 0;
  return 1;
}

// Host-only, 'f16': the chunks of 48 at stride 1.  The Pedestrian widths (32 / 64 / 128 / 256) and 256 -> 48 are REFUSED:
// 48-channel chunks do not divide them (egn_conv3x3_hx_applies below takes them, in chunks of 32).
extern "C" int egn_conv3x3_h_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act) {
  return h_applies(48, N, H, W, Cin, cs_in, Cout, cs_out, has_res, act, 1);
}

// Host-only, 'f16s2': the chunks of 48 at STRIDE 2, without a residual.  256 -> 96 (transition1) is refused like 256 -> 48.
extern "C" int egn_conv3x3s2_h_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int act) {
  return h_applies(48, N, H, W, Cin, cs_in, Cout, cs_out, 0, act, 2);
}

// Host-only, 'f16x': the chunks of 32 at either stride.
extern "C" int egn_conv3x3_hx_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act,
                                      int stride) {
  return h_applies(32, N, H, W, Cin, cs_in, Cout, cs_out, has_res, act, stride);
}

// Host-only: the family predicate of chunk size ck and stride with the storage flags of its tensors -- x_f16: x holds f16
// (what h_round_f16 gives), y_f16: y is written as f16; both 0: the three predicates above.  f16 output never comes with
// a residual (the residual is fp32 and would be added to an fp32 sum: nothing in HRNet asks for it).  The 2 GiB
// condition stays at fp32 sizes: a layer the family takes with f16 storage is one it takes without.
extern "C" int egn_conv3x3_h16_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act,
                                       int stride, int ck, int x_f16, int y_f16) {
  if ((ck != 48 && ck != 32) || (x_f16 & ~1) || (y_f16 & ~1) || (y_f16 && has_res)) return 0;
  return h_applies(ck, N, H, W, Cin, cs_in, Cout, cs_out, has_res, act, stride);
}

extern "C" long egn_conv3x3_h_wpack_bytes(int Cin, int Cout) {
  if (!h_widths(48, Cin, Cout)) return 0;
  return (long)(Cout / 16) * (Cin / H_CK) * H_KS * 64 * 16;
}

extern "C" long egn_conv3x3_hx_wpack_bytes(int Cin, int Cout) {
  if (!h_widths(32, Cin, Cout)) return 0;
  return (long)(Cout / 16) * (Cin / 32) * ConvHChunk<32>::KS * 64 * 16;
}

// the tile geometry of a layer its predicate has taken (ck: the chunk)
static int h_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int act, int stride, int ck) {
  memset(&a, 0, sizeof(a));
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.act = act;
  a.stride = stride; a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1;
  a.ck = ck;
  // output channels per block: 96 / 48 as the widths allow; CK = 32 also 64 (Cout = 64 / 128 / 256) and 32
  a.tn = Cout % 96 == 0 ? 96 : (Cout % 48 == 0 ? 48 : (Cout % 64 == 0 ? 64 : 32));
  const bool wide = a.tn == 96 || a.tn == 64;        // 2 x 2 waves on 64 pixels, else 4 x 1 on 128 (stride 2: 64) pixels
  const int TM = wide || stride == 2 ? 64 : 128;
  // stride 2: at least 2 x 2, so that the 64 images of a tile of 1 x 1 outputs do not bring 64 3 x 3 halos (65 KiB)
  const int th = h_pow2_ceil(a.Ho) < stride ? stride : h_pow2_ceil(a.Ho), tw = h_pow2_ceil(a.Wo) < stride ? stride : h_pow2_ceil(a.Wo);
  a.TH = th < 8 ? th : 8;
  a.TW = tw < TM / 8 ? tw : TM / 8;
  a.TNB = TM / (a.TH * a.TW);
  a.lth = h_log2(a.TH); a.ltw = h_log2(a.TW);
  a.HH = stride * a.TH + 3 - stride; a.HW = stride * a.TW + 3 - stride;
  a.npix = a.TNB * a.HH * a.HW;
  a.tiles_x = (a.Wo + a.TW - 1) / a.TW;
  a.tiles_y = (a.Ho + a.TH - 1) / a.TH;
  // halo offsets; CK = 48: 16 zero bytes and the K-step offsets (224 bytes)
  a.tab_bytes = (a.npix * 4 + 15) / 16 * 16 + (ck == 48 ? ConvHChunk<48>::TAB : ConvHChunk<32>::TAB);
  const int wn = wide ? 2 : 1;
  const int epi = TM * wn * (a.tn / wn + 4) * 4;      // ConvHTile::EPI_BYTES of the instance egn_conv_h_launch picks
  const int halo = a.npix * (ck == 48 ? ConvHChunk<48>::PIXB : ConvHChunk<32>::PIXB);
  a.lds_bytes = a.tab_bytes + (halo > epi ? halo : epi);
  const long long blocks = (long long)a.tiles_x * a.tiles_y * ((N + a.TNB - 1) / a.TNB) * (Cout / a.tn);
  if (a.lds_bytes > 64 * 1024 || blocks > 0x7fffffffll) return EGN_E_BADARG;
  a.blocks = (int)blocks;
  return 0;
}

int egn_conv_h_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int has_res, int act, int stride) {
  if (stride == 1 ? !egn_conv3x3_h_applies(N, H, W, Cin, Cin, Cout, Cout, has_res, act)
                  : stride != 2 || has_res || !egn_conv3x3s2_h_applies(N, H, W, Cin, Cin, Cout, Cout, act))
    return EGN_E_BADARG;
  return h_plan(a, N, H, W, Cin, Cout, act, stride, 48);
}

int egn_conv_hx_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int has_res, int act, int stride) {
  if (!egn_conv3x3_hx_applies(N, H, W, Cin, Cin, Cout, Cout, has_res, act, stride)) return EGN_E_BADARG;
  return h_plan(a, N, H, W, Cin, Cout, act, stride, 32);
}

// either chunk size with the storage flags (egn_conv3x3_h16_applies): the same geometry, the flags beside it
int egn_conv_h16_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int has_res, int act, int stride, int ck,
                      int x16, int y16) {
  if (!egn_conv3x3_h16_applies(N, H, W, Cin, Cin, Cout, Cout, has_res, act, stride, ck, x16, y16)) return EGN_E_BADARG;
  const int rc = h_plan(a, N, H, W, Cin, Cout, act, stride, ck);
  if (rc) return rc;
  a.x16 = x16; a.y16 = y16;
  return 0;
}

// (x16 picks the instance; y16 is a branch of the epilogue)
#define EGN_H_LAUNCH(CK, S, WM, WN, MT, NT)                                                                              \
  do {                                                                                                                   \
    if (a.x16)                                                                                                           \
      hipLaunchKernelGGL((conv_h_kernel<CK, S, WM, WN, MT, NT, true>), dim3(a.blocks), dim3(256), a.lds_bytes, stream, a);  \
    else                                                                                                                 \
      hipLaunchKernelGGL((conv_h_kernel<CK, S, WM, WN, MT, NT, false>), dim3(a.blocks), dim3(256), a.lds_bytes, stream, a); \
  } while (0)

int egn_conv_h_launch(const ConvHArgs& a, hipStream_t stream) {
  if (!a.x || !a.w || !a.scale || !a.shift || !a.y || (a.x16 & ~1) || (a.y16 & ~1) || (a.y16 && a.res)) return EGN_E_BADARG;
  const int s = a.stride;
  if (a.ck == 48) {
    if (a.tn == 96) { if (s == 2) EGN_H_LAUNCH(48, 2, 2, 2, 2, 3); else EGN_H_LAUNCH(48, 1, 2, 2, 2, 3); }
    else if (a.tn == 48) { if (s == 2) EGN_H_LAUNCH(48, 2, 4, 1, 1, 3); else EGN_H_LAUNCH(48, 1, 4, 1, 2, 3); }
    else return EGN_E_BADARG;
  } else if (a.ck == 32) {
    if (a.tn == 96) { if (s == 2) EGN_H_LAUNCH(32, 2, 2, 2, 2, 3); else EGN_H_LAUNCH(32, 1, 2, 2, 2, 3); }
    else if (a.tn == 48) { if (s == 2) EGN_H_LAUNCH(32, 2, 4, 1, 1, 3); else EGN_H_LAUNCH(32, 1, 4, 1, 2, 3); }
    else if (a.tn == 64) { if (s == 2) EGN_H_LAUNCH(32, 2, 2, 2, 2, 2); else EGN_H_LAUNCH(32, 1, 2, 2, 2, 2); }
    else if (a.tn == 32) { if (s == 2) EGN_H_LAUNCH(32, 2, 4, 1, 1, 2); else EGN_H_LAUNCH(32, 1, 4, 1, 2, 2); }
    else return EGN_E_BADARG;
  } else {
    return EGN_E_BADARG;
  }
  EGN_CHECK_HIP(hipGetLastError());
  return 0;
}
#undef EGN_H_LAUNCH

extern std::atomic<long> g_egn_direct_convs;

// the three direct entry points: plan by the chunk size's predicate, launch
static int h_direct(int ck, const float* x, const void* wpack_f16, const float* scale, const float* shift, const float* res,
                    float* y, int N, int H, int W, int Cin, int Cout, int act, int stride, void* stream) {
  g_egn_direct_convs.fetch_add(1, std::memory_order_relaxed);
  ConvHArgs a;
  int rc = (ck == 48 ? egn_conv_h_plan : egn_conv_hx_plan)(a, N, H, W, Cin, Cout, res != nullptr, act, stride);
  if (rc) return rc;
  a.x = x; a.w = wpack_f16; a.scale = scale; a.shift = shift; a.res = res; a.y = y;
  return egn_conv_h_launch(a, (hipStream_t)stream);
}

extern "C" int egn_conv3x3_h_f32(const float* x, const void* wpack_f16, const float* scale, const float* shift,
                                 const float* res, float* y, int N, int H, int W, int Cin, int Cout, int act,
                                 void* stream) {
  return h_direct(48, x, wpack_f16, scale, shift, res, y, N, H, W, Cin, Cout, act, 1, stream);
}

extern "C" int egn_conv3x3s2_h_f32(const float* x, const void* wpack_f16, const float* scale, const float* shift, float* y,
                                   int N, int H, int W, int Cin, int Cout, int act, void* stream) {
  return h_direct(48, x, wpack_f16, scale, shift, nullptr, y, N, H, W, Cin, Cout, act, 2, stream);
}

extern "C" int egn_conv3x3_hx_f32(const float* x, const void* wpack_f16, const float* scale, const float* shift,
                                  const float* res, float* y, int N, int H, int W, int Cin, int Cout, int act, int stride,
                                  void* stream) {
  return h_direct(32, x, wpack_f16, scale, shift, res, y, N, H, W, Cin, Cout, act, stride, stream);
}

// f16 STORAGE of x and / or y (x_f16, y_f16 in {0, 1}; PoseHighResolutionNet.activations = 'f16'): chunk size ck (48 / 32)
// and stride as egn_conv3x3_h16_applies takes them.
extern "C" int egn_conv3x3_h16_f32(const void* x, const void* wpack_f16, const float* scale, const float* shift,
                                   const float* res, void* y, int N, int H, int W, int Cin, int Cout, int act, int stride,
                                   int ck, int x_f16, int y_f16, void* stream) {
  g_egn_direct_convs.fetch_add(1, std::memory_order_relaxed);
  ConvHArgs a;
  int rc = egn_conv_h16_plan(a, N, H, W, Cin, Cout, res != nullptr, act, stride, ck, x_f16, y_f16);
  if (rc) return rc;
  a.x = (const float*)x; a.w = wpack_f16; a.scale = scale; a.shift = shift; a.res = res; a.y = (float*)y;
  return egn_conv_h_launch(a, (hipStream_t)stream);
}
