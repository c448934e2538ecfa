// conv_wino4w.hip -- fused Winograd F(4x4,3x3), 96 output channels per item ("wide" items) [round 6].
//
// Why.  conv_wino4_kernel's K stage takes ~5 600 cycles for 3 456 cycles of MFMA issue per SIMD (profiles/
// r3_wino4_timeline_v2.txt, r5_pmc_sq_wino4.txt: MFMA busy 43 % of CU-busy).  What it pays beside the MFMAs is per
// (tile, input channel): the input transform V = B^T d B (144 VALU per 64 pairs, each VALU instruction 3-10 cycles of
// matrix-pipe time, profiles/r3_mfma_tax.txt), the halo loads and stores, the A-operand reads -- and per stage a barrier
// over 12 waves (~1 000 cycles of skew).  None of that depends on how many OUTPUT channels multiply the transformed
// tile.  With one 48-channel co-tile per item a (tile, channel) pair feeds 3 MFMAs per frequency point; here an item is
// 16 tiles x 96 output channels = TWO co-tiles of the same packed filter, so a pair feeds 6: half the transform
// instructions, halo bytes, A reads and barriers per MFMA, the same 72 accumulator registers per wave as
// conv_wino4_kernel (3 points x 6 co sub-tiles x 1 m-tile instead of 3 x 3 x 2).
//
// Block = 12 waves, region = 16 x 16 output pixels of one image (conv_wino4b_kernel's geometry 1: halo order, transform
// shares, V layout [point][k-group 0..3][lane], 16-channel stages), wave w owns frequency points 3w .. 3w+2.
// A wait group is ONE 4-channel k-group: 6 buffer_load_dwordx4 per lane (the wave's slices of co-tiles 2p and 2p + 1 in
// wino4_pack.h's layout -- no new packing), 18 MFMAs; four wait groups per stage, two filter buffers in registers.
// The transform thirds sit where only ONE filter buffer is live (72 accumulators + 24 filter + 8 halo + ~40 transform
// registers: 168 is the budget of three waves per SIMD).  Every vector-memory wait is vmcnt(0) (conv_wino4.hip).
// Item end: two exchange rounds (one per co-tile) through the 108 KB [point][co sub-tile][lane] float4 image that
// conv_wino4_kernel uses per m-tile.
// Which layers: 96 -> 96 @ 32 x 32 at 64 crops (256 items; 64 launches of the W48 forward).  192 / 384 channels have
// too few items at 64 crops (128 / 64); the tuner measures, the table decides.
// Reference: the 3x3 stride-1 convolutions of libs/model/heatmapModel/hrnet.py (BasicBlock :49-76).
#include "conv_wino4w_body.h"

template <int ABL>
__global__ __launch_bounds__(W4_NTH, 1) void conv_wino4w_kernel(ConvArgs a) { w4w_body<ABL>(a, (int)blockIdx.x, (int)gridDim.x); }

bool egn_conv_wino4w_applies(const ConvArgs& a) {
  return egn_plain_3x3_s1(a) && a.Cin % 16 == 0 && a.Cin >= 32 && a.Cout % (2 * W4_CO) == 0 && a.Ho % 16 == 0 &&
         a.Wo % 16 == 0;
}

template <int ABL>
static int wino4w_launch(ConvArgs a, size_t lds, hipStream_t stream) {
  static bool raised[EGN_MAX_DEVICES];
  void (*kern)(ConvArgs) = &conv_wino4w_kernel<ABL>;
  EGN_CHECK_HIP(egn_allow_big_lds(kern, EGN_BIG_LDS_BYTES, raised));
  const int ncp = a.Cout / (2 * W4_CO);
  const int nwork = w4_item_setup(a, ncp, 1, a.tiles_x * a.tiles_y * a.N);
  if (nwork < 0) return nwork;
  const int grid = egn_persistent_grid(nwork, 8 * ncp);     // one block per CU, whole XCD rounds
  hipLaunchKernelGGL(kern, dim3(grid), dim3(W4_NTH), lds, stream, a);
  return (int)hipGetLastError();
}
int egn_conv_launch_wino4w(ConvArgs a, size_t lds, int abl, hipStream_t stream) {
  if (!egn_conv_wino4w_applies(a)) return EGN_E_BADARG;
  switch (abl) {
    case 0: return wino4w_launch<0>(a, lds, stream);
#ifdef EGN_PROBES
    case 64: return wino4w_launch<64>(a, lds, stream);
#endif
    default: return EGN_E_BADARG;
  }
}
