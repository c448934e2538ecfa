// conv_plan.hip -- host side of the convolution: the table of tile configurations, the launch planner (spatial
// tile, taps per stage, LDS budget) and the dispatcher.
//
// kConfigs is the one place that says what a config id is (ConvConfig, egn_internal.h): family, kernel, tile, ablation
// value, filter kind, build and kernel symbol are written in the row and read from it; the family launchers take the
// kernel enum and the ablation value.  Families, by id:
//    1..10  Staged  global -> registers -> LDS, one LDS buffer, 2 barriers per stage, 3 blocks per CU    conv_mfma.hip
//   11..30  Dma     buffer_load ... lds into a double-buffered stage, 1 barrier per stage; 11..20 with an
//                   80 KB budget (2 blocks per CU), 21..30 with 53 KB (3 blocks per CU)                   conv_dma.hip
//   31..40  Retired a persistent variant of the Dma pipeline that no shape ever selected (removed in round 2; the
//                   ids stay reserved so measured tables keep their meaning)
//   41..44  C48     filter-resident persistent kernels for the 48 -> 48 3x3 layers                         conv_c48.hip
//   45..63, 65..69  Wino   fused Winograd F(2x2,3x3) for the 3x3 stride-1 layers (conv_wino_kernel, conv_wino8_kernel,
//                   conv_wino9_kernel) and the first F(4x4,3x3) kernel (65 / 66)                           conv_wino.hip
//   64      Stem    3x3 s2, 3 -> 64 channels                                                               conv_stem.hip
//   70..78, 80..84, 86..93  Wino4  fused Winograd F(4x4,3x3), register-fed filter     conv_wino4.hip, conv_wino4w/h/r.hip
//   79      Fc      1x1 row GEMM (the lifter's Linear layers)                                              conv_fc.hip
//   85      S2r     3x3 s2 from the 48-channel branch                                                      conv_s2r.hip
// The engine's tuner times the candidates on the real shape; cfg 0 = cost model (over the Staged family).
#include <stdio.h>
#include <string.h>

#include "egn_internal.h"
#include "plan_format.h"

int egn_conv_launch_staged(const ConvArgs& a, DirectTile tile, size_t lds, hipStream_t stream);   // conv_mfma.hip
int egn_conv_launch_dma(const ConvArgs& a, DirectTile tile, size_t lds, hipStream_t stream);      // conv_dma.hip
int egn_conv_launch_c48(const ConvArgs& a, size_t lds, C48Kernel k, hipStream_t stream);          // conv_c48.hip
bool egn_conv_c48_applies(const ConvArgs& a);
size_t egn_conv_c48_lds_bytes(const ConvArgs& a, C48Kernel k);
int egn_conv_launch_wino(const ConvArgs& a, size_t lds, WinoKernel k, int abl, hipStream_t stream);   // conv_wino.hip
bool egn_conv_wino_applies(const ConvArgs& a, WinoKernel k);
size_t egn_conv_wino_lds_bytes(WinoKernel k, int abl, int cout);
int egn_conv_wino_stats_rows(const ConvArgs& a, WinoKernel k, int abl);
int egn_conv_launch_stem(const ConvArgs& a, size_t lds, hipStream_t stream);   // conv_stem.hip
bool egn_conv_stem_applies(const ConvArgs& a);
size_t egn_conv_stem_lds_bytes();
int egn_conv_launch_wino4(ConvArgs a, size_t lds, Wino4Kernel k, int abl, hipStream_t stream);    // conv_wino4.hip
bool egn_conv_wino4_applies(const ConvArgs& a, Wino4Kernel k);
size_t egn_conv_wino4_lds_bytes(Wino4Kernel k);
int egn_conv_wino4_tickets(const ConvArgs& a, Wino4Kernel k);
int egn_conv_wino4_stats_rows(const ConvArgs& a, Wino4Kernel k);
int egn_conv_launch_s2r(const ConvArgs& a, hipStream_t stream);                         // conv_s2r.hip
bool egn_conv_s2r_applies(const ConvArgs& a);
size_t egn_conv_s2r_lds_bytes();
int egn_conv_launch_fc(const ConvArgs& a, hipStream_t stream);                          // conv_fc.hip
bool egn_conv_fc_applies(const ConvArgs& a);

using F = ConvFamily;
constexpr bool Product = false, ProbeOnly = true;   // ConvConfig::probe_only

// Families that were measured and lost (cfg 41 / 43: 4-wave and register-filter forms of conv_c48.hip; 45 / 46: the
// 4-wave Winograd kernel; 65: the first F(4x4,3x3) kernel; 67 / 68: two 4-wave blocks per CU; 88 / 90 / 92: the
// half-block and row-owner F(4x4,3x3) kernels, profiles/r6_wino4h_*.txt, r6_wino4r_probe.txt) are ProbeOnly: they
// exist only in probe builds (-DEGN_PROBES: python -m egonet_amd.build --probes, used by tools/); the product library
// neither compiles nor plans nor launches them, and the timing-ablation / stamp builds (abl != 0: WRONG RESULTS)
// likewise.  The names of the ablation / stamp rows of the Wino family still print the selector 1..4 (0 for CLK
// builds) where the symbol has the ABL / CLK value: nothing lines those rows up with a kernel trace.
static const ConvConfig kConfigs[] = {
    // id, wm, wn, mt, nt, family, kernel, abl, kind, build,
    //   Staged / Dma: {ai, bi, lds_kb}            others: {}, {TH, TW, TNB, tps[, HH, HW]}, name
    {1, 4, 1, 4, 3, F::Staged, T256x48, 0, 0, Product, {6, 7, 64}},  // 256 x 48   (C = 48 layers)
    {2, 2, 2, 4, 3, F::Staged, T128x96, 0, 0, Product, {6, 8, 64}},  // 128 x 96   (C = 96)
    {3, 2, 2, 4, 2, F::Staged, T128x64, 0, 0, Product, {8, 8, 64}},  // 128 x 64   (C = 64, 192, 256, 384)
    {4, 4, 1, 4, 1, F::Staged, T256x16, 0, 0, Product, {8, 8, 64}},  // 256 x 16
    {5, 4, 1, 4, 2, F::Staged, T256x32, 0, 0, Product, {8, 8, 64}},  // 256 x 32
    {6, 4, 1, 2, 3, F::Staged, T128x48, 0, 0, Product, {8, 8, 64}},  // 128 x 48
    {7, 2, 2, 2, 3, F::Staged, T64x96, 0, 0, Product, {8, 8, 64}},  //  64 x 96
    {8, 2, 2, 2, 2, F::Staged, T64x64, 0, 0, Product, {8, 8, 64}},  //  64 x 64
    {9, 1, 4, 4, 1, F::Staged, T64x64_NWaves, 0, 0, Product, {8, 8, 64}},  //  64 x 64 (one M strip, N across waves)
    {10, 1, 4, 2, 3, F::Staged, T32x192, 0, 0, Product, {8, 8, 64}},  //  32 x 192
    {11, 4, 1, 4, 3, F::Dma, T256x48, 0, 0, Product, {8, 8, 80}},  // the same tile shapes, LDS-DMA pipeline
    {12, 2, 2, 4, 3, F::Dma, T128x96, 0, 0, Product, {8, 8, 80}},
    {13, 2, 2, 4, 2, F::Dma, T128x64, 0, 0, Product, {8, 8, 80}},
    {14, 4, 1, 4, 1, F::Dma, T256x16, 0, 0, Product, {8, 8, 80}},
    {15, 4, 1, 4, 2, F::Dma, T256x32, 0, 0, Product, {8, 8, 80}},
    {16, 4, 1, 2, 3, F::Dma, T128x48, 0, 0, Product, {8, 8, 80}},
    {17, 2, 2, 2, 3, F::Dma, T64x96, 0, 0, Product, {8, 8, 80}},
    {18, 2, 2, 2, 2, F::Dma, T64x64, 0, 0, Product, {8, 8, 80}},
    {19, 1, 4, 4, 1, F::Dma, T64x64_NWaves, 0, 0, Product, {8, 8, 80}},
    {20, 1, 4, 2, 3, F::Dma, T32x192, 0, 0, Product, {8, 8, 80}},
    {21, 4, 1, 4, 3, F::Dma, T256x48, 0, 0, Product, {8, 8, 53}},  // LDS-DMA pipeline with a 53 KB LDS budget (3 blocks / CU:
    {22, 2, 2, 4, 3, F::Dma, T128x96, 0, 0, Product, {8, 8, 53}},  // fewer taps per stage, more barriers, more waves to hide
    {23, 2, 2, 4, 2, F::Dma, T128x64, 0, 0, Product, {8, 8, 53}},  // per-block prologue / epilogue)
    {24, 4, 1, 4, 1, F::Dma, T256x16, 0, 0, Product, {8, 8, 53}},
    {25, 4, 1, 4, 2, F::Dma, T256x32, 0, 0, Product, {8, 8, 53}},
    {26, 4, 1, 2, 3, F::Dma, T128x48, 0, 0, Product, {8, 8, 53}},
    {27, 2, 2, 2, 3, F::Dma, T64x96, 0, 0, Product, {8, 8, 53}},
    {28, 2, 2, 2, 2, F::Dma, T64x64, 0, 0, Product, {8, 8, 53}},
    {29, 1, 4, 4, 1, F::Dma, T64x64_NWaves, 0, 0, Product, {8, 8, 53}},
    {30, 1, 4, 2, 3, F::Dma, T32x192, 0, 0, Product, {8, 8, 53}},
    {31, 4, 1, 4, 3, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},  // 31..40 retired: never planned, never launched
    {32, 2, 2, 4, 3, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {33, 2, 2, 4, 2, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {34, 4, 1, 4, 1, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {35, 4, 1, 4, 2, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {36, 4, 1, 2, 3, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {37, 2, 2, 2, 3, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {38, 2, 2, 2, 2, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {39, 1, 4, 4, 1, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    {40, 1, 4, 2, 3, F::Retired, {}, 0, -1, Product, {}, {}, "(retired)"},
    // 48 -> 48 3x3 s1 only: filter resident in LDS, persistent (conv_c48.hip)
    {41, 4, 1, 2, 3, F::C48, C48_Waves4, 0, 0, ProbeOnly, {}, {8, 16, 1, 9}, "void conv_c48_kernel<4>(ConvArgs)"},
    // the same with 8 waves (two per SIMD)
    {42, 8, 1, 1, 3, F::C48, C48_Waves8, 0, 0, Product, {}, {8, 16, 1, 9}, "void conv_c48_kernel<8>(ConvArgs)"},
    // 4 waves, each with the whole filter in REGISTERS
    {43, 4, 1, 2, 3, F::C48, C48_RegFilter, 0, 0, ProbeOnly, {}, {8, 16, 1, 9}, "conv_c48r_kernel(ConvArgs)"},
    // 8 waves x 2 rows on a 16 x 16 tile, halo as a ring of chunks
    {44, 8, 1, 2, 3, F::C48, C48_Ring, 0, 0, Product, {}, {16, 16, 1, 9}, "conv_c48t_kernel(ConvArgs)"},
    // 16 x 16 pixel tile of one image
    {45, 4, 1, 1, 3, F::Wino, Wino_16x16, 0, 1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino_kernel<16, 16, 1, 0>(ConvArgs)"},
    // four 8 x 8 images per block
    {46, 4, 1, 1, 3, F::Wino, Wino_8x8x4, 0, 1, ProbeOnly, {}, {8, 8, 4, 16}, "void conv_wino_kernel<8, 8, 4, 0>(ConvArgs)"},
    // timing ablations of 45 (WRONG RESULTS, tools/wino_probe.py only):
    {47, 4, 1, 1, 3, F::Wino, Wino_16x16, 15, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino_kernel<16, 16, 1, 1>(ConvArgs)"},
    // no DMA / no input transform / no epilogue memory ops / no barriers
    {48, 4, 1, 1, 3, F::Wino, Wino_16x16, 7, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino_kernel<16, 16, 1, 2>(ConvArgs)"},
    {49, 4, 1, 1, 3, F::Wino, Wino_16x16, 3, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino_kernel<16, 16, 1, 3>(ConvArgs)"},
    {50, 4, 1, 1, 3, F::Wino, Wino_16x16, 11, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino_kernel<16, 16, 1, 4>(ConvArgs)"},
    // the 8-wave Winograd kernel (two per SIMD, frequency halves): 16 x 16 tile
    {51, 8, 1, 1, 3, F::Wino, Wino8_16x16, 0, 1, Product, {}, {16, 16, 1, 16}, "void conv_wino8_kernel<16, 16, 1, 0, 8, 3>(ConvArgs)"},
    // ... four 8 x 8 images
    {52, 8, 1, 1, 3, F::Wino, Wino8_8x8x4, 0, 1, Product, {}, {8, 8, 4, 16}, "void conv_wino8_kernel<8, 8, 4, 0, 8, 3>(ConvArgs)"},
    // timing ablations of 51
    {53, 8, 1, 1, 3, F::Wino, Wino8_16x16, 16, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino8_kernel<16, 16, 1, 1, 8, 3>(ConvArgs)"},
    {54, 8, 1, 1, 3, F::Wino, Wino8_16x16, 7, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino8_kernel<16, 16, 1, 2, 8, 3>(ConvArgs)"},
    {55, 8, 1, 1, 3, F::Wino, Wino8_16x16, 3, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino8_kernel<16, 16, 1, 3, 8, 3>(ConvArgs)"},
    // frequency-halves kernel with 4 waves on two 8 x 8 images (32 tiles per block)
    {56, 4, 1, 1, 3, F::Wino, Wino8_8x8x2, 0, 1, Product, {}, {8, 8, 2, 16}, "void conv_wino8_kernel<8, 8, 2, 0, 4, 3>(ConvArgs)"},
    // ... on an 8 x 16 pixel tile of one image
    {57, 4, 1, 1, 3, F::Wino, Wino8_8x16, 0, 1, Product, {}, {8, 16, 1, 16}, "void conv_wino8_kernel<8, 16, 1, 0, 4, 3>(ConvArgs)"},
    // 51 with s_memtime stamps (tools/wino_clk.py; `res` = the stamp buffer)
    {58, 8, 1, 1, 3, F::Wino, Wino8_16x16, 32, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino8_kernel<16, 16, 1, 4, 8, 3>(ConvArgs)"},
    // conv_wino9_kernel (half the VALU instructions of 51 / 52 / 56 / 57): 16 x 16 tile
    {59, 8, 1, 1, 3, F::Wino, Wino9_16x16, 0, 1, Product, {}, {16, 16, 1, 16}, "void conv_wino9_kernel<16, 16, 1, 8, 3, 0, 4>(ConvArgs)"},
    // ... four 8 x 8 images
    {60, 8, 1, 1, 3, F::Wino, Wino9_8x8x4, 0, 1, Product, {}, {8, 8, 4, 16}, "void conv_wino9_kernel<8, 8, 4, 8, 3, 0, 4>(ConvArgs)"},
    // ... two 8 x 8 images, 4 waves
    {61, 4, 1, 1, 3, F::Wino, Wino9_8x8x2, 0, 1, Product, {}, {8, 8, 2, 16}, "void conv_wino9_kernel<8, 8, 2, 4, 3, 0, 4>(ConvArgs)"},
    // ... 8 x 16 pixel tile, 4 waves
    {62, 4, 1, 1, 3, F::Wino, Wino9_8x16, 0, 1, Product, {}, {8, 16, 1, 16}, "void conv_wino9_kernel<8, 16, 1, 4, 3, 0, 4>(ConvArgs)"},
    // 59 with s_memtime stamps (tools/wino_clk.py)
    {63, 8, 1, 1, 3, F::Wino, Wino9_16x16, 1, -1, ProbeOnly, {}, {16, 16, 1, 16}, "void conv_wino9_kernel<16, 16, 1, 8, 3, 0, 4>(ConvArgs)"},
    // the stem: 3x3 s2, 3 -> 64 channels, K = (tap, channel) (conv_stem.hip)
    {64, 4, 1, 1, 4, F::Stem, {}, 0, 0, Product, {}, {16, 16, 1, 9, 33, 33}, "conv_stem_kernel(ConvArgs)"},
    // fused Winograd F(4x4,3x3), conv_wino43_kernel: filter from egn ... kind 2
    {65, 6, 1, 1, 3, F::Wino, Wino43, 0, 2, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino43_kernel<0>(ConvArgs)"},
    {66, 6, 1, 1, 3, F::Wino, Wino43, 1, -1, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino43_kernel<0>(ConvArgs)"},  // 65 with s_memtime stamps
    // conv_wino9_kernel with 8-channel stages: 8 x 16 tile, 4 waves, TWO blocks per CU
    {67, 4, 1, 1, 3, F::Wino, Wino9h_8x16, 0, 1, ProbeOnly, {}, {8, 16, 1, 16}, "void conv_wino9_kernel<8, 16, 1, 4, 3, 0, 2>(ConvArgs)"},
    // ... two 8 x 8 images
    {68, 4, 1, 1, 3, F::Wino, Wino9h_8x8x2, 0, 1, ProbeOnly, {}, {8, 8, 2, 16}, "void conv_wino9_kernel<8, 8, 2, 4, 3, 0, 2>(ConvArgs)"},
    // 67 with s_memtime stamps (tools/wino_clk.py)
    {69, 4, 1, 1, 3, F::Wino, Wino9h_8x16, 1, -1, ProbeOnly, {}, {8, 16, 1, 16}, "void conv_wino9_kernel<8, 16, 1, 4, 3, 0, 2>(ConvArgs)"},
    // fused Winograd F(4x4,3x3), conv_wino4_kernel (conv_wino4.hip): filter kind 3
    {70, 12, 1, 1, 3, F::Wino4, Wino4, 0, 3, Product, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<0>(ConvArgs)"},
    // timing ablations of 70 (WRONG RESULTS, tools/wino_probe.py only): no input transform
    {71, 12, 1, 1, 3, F::Wino4, Wino4, 1, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<1>(ConvArgs)"},
    {72, 12, 1, 1, 3, F::Wino4, Wino4, 2, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<2>(ConvArgs)"},  // ... no MFMAs
    // ... no exchange / output transform / stores
    {73, 12, 1, 1, 3, F::Wino4, Wino4, 4, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<4>(ConvArgs)"},
    {74, 12, 1, 1, 3, F::Wino4, Wino4, 8, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<8>(ConvArgs)"},  // ... no filter loads
    {75, 12, 1, 1, 3, F::Wino4, Wino4, 16, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<16>(ConvArgs)"},  // ... no halo DMA
    // ... only DMA + filter loads + barriers
    {76, 12, 1, 1, 3, F::Wino4, Wino4, 7, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<7>(ConvArgs)"},
    // ... halo reads without bank conflicts
    {77, 12, 1, 1, 3, F::Wino4, Wino4, 32, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<32>(ConvArgs)"},
    // 70 with s_memtime stamps (tools/wino4_clk.py; `res` = the stamp buffer)
    {78, 12, 1, 1, 3, F::Wino4, Wino4, 64, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4_kernel<64>(ConvArgs)"},
    // 1x1 conv on 1 x 1 maps (the lifter's Linear layers): one 16 x 16 tile per block, K split over the waves
    // (conv_fc.hip)
    {79, 4, 1, 1, 1, F::Fc, {}, 0, 0, Product, {}, {1, 1, 16, 1, 1, 1}, "conv_fc_kernel(ConvArgs)"},
    // conv_wino4b_kernel: F(4x4,3x3) on 16 x 16 pixel regions, 16-channel stages; filter kind 3
    {80, 12, 1, 1, 3, F::Wino4, Wino4b, 0, 3, Product, {}, {16, 16, 1, 36}, "void conv_wino4b_kernel<0>(ConvArgs)"},
    // 80 with s_memtime stamps (tools/wino4_clk.py)
    {81, 12, 1, 1, 3, F::Wino4, Wino4b, 64, -1, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino4b_kernel<64>(ConvArgs)"},
    // conv_wino4c_kernel<0, 1>: F(4x4,3x3) on 8 x 8 maps, four images per region; filter kind 3
    {82, 12, 1, 1, 3, F::Wino4, Wino4c, 0, 3, Product, {}, {8, 8, 4, 36}, "void conv_wino4c_kernel<0, 1>(ConvArgs)"},
    // conv_wino4c_kernel<0, 2>: 82 with the input channels of an item split over two blocks: memset, atomic adds,
    // conv_wino4_finish_kernel
    {83, 12, 1, 1, 3, F::Wino4, Wino4c_KSplit, 0, 3, Product, {}, {8, 8, 4, 36}, "void conv_wino4c_kernel<0, 2>(ConvArgs)"},
    // conv_wino4bk_kernel: 80 with the input channels of an item split over two blocks, as 83
    {84, 12, 1, 1, 3, F::Wino4, Wino4b_KSplit, 0, 3, Product, {}, {16, 16, 1, 36}, "void conv_wino4bk_kernel<0>(ConvArgs)"},
    // conv_s2r_kernel [round 5]: 3x3 stride 2 from the 48-channel branch, filter slice in registers (conv_s2r.hip);
    // direct-packed filter
    {85, 3, 1, 1, 3, F::S2r, {}, 0, 0, Product, {}, {2, 8, 1, 9, 5, 17}, "conv_s2r_kernel(ConvArgs)"},
    // conv_wino4w_kernel [round 6]: F(4x4,3x3), 16 x 16 pixel regions x 96 output channels per item (conv_wino4w.hip);
    // filter kind 3
    {86, 12, 1, 1, 3, F::Wino4, Wino4w, 0, 3, Product, {}, {16, 16, 1, 36}, "void conv_wino4w_kernel<0>(ConvArgs)"},
    // 86 with s_memtime stamps (tools/wino4_clk.py)
    {87, 12, 1, 1, 3, F::Wino4, Wino4w, 64, -1, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino4w_kernel<64>(ConvArgs)"},
    // (probe builds only: NEGATIVE result) conv_wino4h_kernel [round 6]: F(4x4,3x3) in half-size blocks (6 waves, 16
    // tiles x 48 channels, 62 KB), two independent blocks per CU (conv_wino4h.hip); filter kind 3
    {88, 6, 1, 1, 3, F::Wino4, Wino4h, 0, 3, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino4h_kernel<0>(ConvArgs)"},
    // 88 with s_memtime stamps (tools/wino4_clk.py)
    {89, 6, 1, 1, 3, F::Wino4, Wino4h, 64, -1, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino4h_kernel<64>(ConvArgs)"},
    // (probe builds only: NEGATIVE result) conv_wino4d_kernel [round 6]: 88's two blocks of a CU as the independent
    // halves of ONE 12-wave workgroup (LDS-counter barriers per half); filter kind 3
    {90, 12, 1, 1, 3, F::Wino4, Wino4d, 0, 3, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino4d_kernel<0>(ConvArgs)"},
    // 90 with s_memtime stamps (tools/wino4_clk.py)
    {91, 12, 1, 1, 3, F::Wino4, Wino4d, 64, -1, ProbeOnly, {}, {16, 16, 1, 36}, "void conv_wino4d_kernel<64>(ConvArgs)"},
    // (probe builds only: NEGATIVE result) conv_wino4r_kernel [round 6]: F(4x4,3x3) on 16 x 32 regions with ROW-OWNER
    // waves -- the row pass of the output transform in the accumulators, ONE exchange round per item
    // (conv_wino4r.hip); filter kind 3
    {92, 12, 1, 1, 3, F::Wino4, Wino4r, 0, 3, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4r_kernel<0>(ConvArgs)"},
    // 92 with s_memtime stamps (tools/wino4_clk.py)
    {93, 12, 1, 1, 3, F::Wino4, Wino4r, 64, -1, ProbeOnly, {}, {16, 32, 1, 36}, "void conv_wino4r_kernel<64>(ConvArgs)"},
};
static const int kNumConfigs = sizeof(kConfigs) / sizeof(kConfigs[0]);

extern "C" int egn_conv_num_configs(void) { return kNumConfigs; }
const ConvConfig* egn_conv_config(int cfg) {
  return (cfg >= 1 && cfg <= kNumConfigs) ? &kConfigs[cfg - 1] : nullptr;
}
extern "C" int egn_conv_config_info(int cfg, int* tile_m, int* tile_n) {
  if (cfg < 1 || cfg > kNumConfigs) return EGN_E_BADARG;
  if (tile_m) *tile_m = kConfigs[cfg - 1].tile_m();
  if (tile_n) *tile_n = kConfigs[cfg - 1].tile_n();
  return 0;
}

// what this build can plan and launch: not the reserved ids, and the ProbeOnly rows in probe builds only
static bool in_this_build(const ConvConfig& c) {
  if (c.family == F::Retired) return false;
#ifndef EGN_PROBES
  if (c.probe_only) return false;
#endif
  return true;
}
// the filter layout (kind) cfg's kernel reads, -1 = not selectable: include/egonet_hip.h lists the kinds
extern "C" int egn_conv_config_kind(int cfg) {
  if (cfg < 1 || cfg > kNumConfigs || !in_this_build(kConfigs[cfg - 1])) return -1;
  return kConfigs[cfg - 1].kind;
}
// 1 = a probe build (ablation / stamp / retired configurations can be launched through egn_conv2d_f32(cfg))
extern "C" int egn_probe_build(void) {
#ifdef EGN_PROBES
  return 1;
#else
  return 0;
#endif
}

// kernel symbol of a config as rocprofv3 prints it (lets bench.py line its
// hipEvent timings up with the kernel-trace statistics)
// (conv_wino8_kernel / conv_wino9_kernel rows: the symbol of the 48-channel co-tile build, NT = 3: the W48 widths;
// layers with Cout % 48 != 0 run the NT = 2 build of the same kernel)
extern "C" int egn_conv_config_name(int cfg, char* buf, int len) {
  if (cfg < 1 || cfg > kNumConfigs || !buf || len < 8) return EGN_E_BADARG;
  const ConvConfig& c = kConfigs[cfg - 1];
  if (c.family == F::Staged)
    snprintf(buf, len, "void conv_mfma_kernel<%d, %d, %d, %d, %d, %d>(ConvArgs)", c.wm, c.wn, c.mt, c.nt, c.staging.ai,
             c.staging.bi);
  else if (c.family == F::Dma)
    snprintf(buf, len, "void conv_dma_kernel<%d, %d, %d, %d, 8, 8, 0>(ConvArgs)", c.wm, c.wn, c.mt, c.nt);
  else
    snprintf(buf, len, "%s", c.name);
  return 0;
}

// what the ids MEAN, as one number: a plan file (plan.cpp) names configurations by id, and is refused by a library whose
// table gives an id another kind, other tile sizes or another kernel
extern "C" unsigned egn_conv_table_fingerprint(void) {
  uint32_t crc = 0;
  for (int cfg = 1; cfg <= kNumConfigs; ++cfg) {
    char name[256] = {0};
    egn_conv_config_name(cfg, name, (int)sizeof(name));
    const int32_t row[4] = {cfg, egn_conv_config_kind(cfg), kConfigs[cfg - 1].tile_m(), kConfigs[cfg - 1].tile_n()};
    crc = egn_plan_crc32(row, sizeof(row), crc);
    crc = egn_plan_crc32(name, strlen(name), crc);
  }
  return crc;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static bool searched_tile(const ConvConfig& cf) { return cf.family == F::Staged || cf.family == F::Dma; }

// LDS layout of the Staged / Dma kernels: [ K-loop stage buffers | epilogue sC (aliases them) ][ sPix: TM ints ]
static size_t lds_stage_bytes(const ConvArgs& a, const ConvConfig& cf) {
  size_t main_loop = (size_t)(EGN_CKQ * a.npixp + a.tps * EGN_CKQ * cf.tile_n()) * 16;
  if (cf.family == F::Dma) main_loop *= 2;  // double-buffered stage
  // epilogue: 4 waves x (MT*16 rows) x (NT*16 + 4) floats
  const size_t epi = a.out_nchw ? 0 : (size_t)4 * cf.mt * 16 * (cf.nt * 16 + 4) * 4;
  return ((main_loop > epi ? main_loop : epi) + 15) & ~(size_t)15;
}
static size_t lds_bytes_for(const ConvArgs& a, const ConvConfig& cf) {
  switch (cf.family) {
    case F::Staged:
    case F::Dma: return lds_stage_bytes(a, cf) + (size_t)cf.tile_m() * 4;
    case F::Retired: return 0;
    case F::C48: return egn_conv_c48_lds_bytes(a, cf.kernel.c48);
    case F::Wino: return egn_conv_wino_lds_bytes(cf.kernel.wino, cf.abl, a.Cout);
    case F::Stem: return egn_conv_stem_lds_bytes();
    case F::Wino4: return egn_conv_wino4_lds_bytes(cf.kernel.wino4);
    case F::Fc: return 0;
    case F::S2r: return egn_conv_s2r_lds_bytes();
  }
  return 0;
}

// the shapes a fixed-tile family (kernel) takes; a.TH / TW / TNB are the row's
static bool family_applies(const ConvArgs& a, const ConvConfig& cf) {
  switch (cf.family) {
    case F::Staged:
    case F::Dma:
    case F::Retired: return false;
    case F::C48: return egn_conv_c48_applies(a);
    case F::Wino: return egn_conv_wino_applies(a, cf.kernel.wino);
    case F::Stem: return egn_conv_stem_applies(a);
    case F::Wino4: return egn_conv_wino4_applies(a, cf.kernel.wino4);
    case F::Fc: return egn_conv_fc_applies(a);
    case F::S2r: return egn_conv_s2r_applies(a);
  }
  return false;
}

// Choose the spatial tile for a config.  Fixed-tile families: the row's tile where the family takes the shape.
// Staged / Dma: minimise (MFMA work incl. padding + LDS fill work) over power-of-two tile shapes, subject to the row's
// LDS budget and to its per-lane staging depth (ai / bi dwordx4 loads per stage).
static bool plan_tile(ConvArgs& a, const ConvConfig& cf, double* cost_out) {
  if (!in_this_build(cf)) return false;
  if (!searched_tile(cf)) {
    a.TH = cf.tile.TH; a.TW = cf.tile.TW; a.TNB = cf.tile.TNB;
    a.HH = cf.tile.HH ? cf.tile.HH : a.TH + 2; a.HW = cf.tile.HW ? cf.tile.HW : a.TW + 2;
    a.npix = a.TNB * a.HH * a.HW; a.npixp = (a.npix + 15) & ~15; a.tps = cf.tile.tps;
    if (!family_applies(a, cf)) return false;
    a.tiles_x = cdiv(a.Wo, a.TW);
    a.tiles_y = cdiv(a.Ho, a.TH);
    if (cf.family == F::Fc) a.tiles_x = a.tiles_y = 1;   // the row GEMM walks the pixels as rows of one tile column
    if (cost_out) *cost_out = 0.0;
    return true;
  }
  const size_t lds_budget = (size_t)cf.staging.lds_kb * 1024;
  const int tm = cf.tile_m();
  const int tn = cf.tile_n();
  double best = -1.0;
  ConvArgs bestA = a;
  for (int tw = 1; tw <= 64 && tw <= tm; tw *= 2) {
    if (tw < 4 && tw < a.Wo) continue;  // narrow tiles only for maps that narrow
    for (int th = 1; th * tw <= tm; th *= 2) {
      const int tnb = tm / (tw * th);
      if (tnb * tw * th != tm) continue;
      // no point in tiles much larger than the map
      if (tw >= 2 * a.Wo && tw > 1) continue;
      if (th >= 2 * a.Ho && th > 1) continue;
      ConvArgs c = a;
      c.TH = th; c.TW = tw; c.TNB = tnb;
      c.HH = (th - 1) * a.stride + a.KH;
      c.HW = (tw - 1) * a.stride + a.KW;
      c.npix = tnb * c.HH * c.HW;
      c.npixp = (c.npix + 15) & ~15;
      if (c.npix * EGN_CKQ > cf.staging.ai * 256) continue;
      c.tiles_x = cdiv(a.Wo, tw);
      c.tiles_y = cdiv(a.Ho, th);
      const int tiles_b = cdiv(a.N, tnb);
      // taps per stage: as many as fit the LDS budget and the staging depth
      int tps = a.taps;
      c.tps = tps;
      while (tps > 1 && (lds_bytes_for(c, cf) > lds_budget || tps * EGN_CKQ * tn > cf.staging.bi * 256)) {
        --tps;
        c.tps = tps;
      }
      if (lds_bytes_for(c, cf) > lds_budget || tps * EGN_CKQ * tn > cf.staging.bi * 256) continue;
      // balance the stages (e.g. 9 taps -> 5+4 instead of 8+1)
      const int nst = cdiv(a.taps, tps);
      c.tps = cdiv(a.taps, nst);
      const double tiles = (double)c.tiles_x * c.tiles_y * tiles_b * cdiv(a.CoutP, tn);
      const double mfma = (double)tm * tn * a.taps * EGN_CK;  // per chunk per tile
      const double fill = (double)c.npix * EGN_CK * 24.0 + (double)a.taps * EGN_CK * tn * 12.0;
      // ties (1x1 convs have no halo): prefer contiguous pixels over many images
      const double cost = tiles * (mfma + fill + 4000.0 * nst + 64.0 * tnb + 8.0 * th);
      if (best < 0 || cost < best) { best = cost; bestA = c; }
    }
  }
  if (best < 0) return false;
  a = bestA;
  if (cost_out) *cost_out = best;
  return true;
}

int egn_conv_plan(ConvArgs& a, int& cfg_id, size_t& lds_bytes) {
  if (a.N <= 0 || a.H <= 0 || a.W <= 0 || a.Cin <= 0 || a.Cout <= 0) return EGN_E_BADARG;
  if (a.cs_in % 4 || a.cs_in < a.Cin) return EGN_E_BADARG;
  if (!a.out_nchw && (a.cs_out % 4 || a.cs_out < a.Cout)) return EGN_E_BADARG;
  if (a.KH < 1 || a.KW < 1 || a.stride < 1 || a.pad < 0) return EGN_E_BADARG;
  a.Ho = (a.H + 2 * a.pad - a.KH) / a.stride + 1;
  a.Wo = (a.W + 2 * a.pad - a.KW) / a.stride + 1;
  if (a.Ho <= 0 || a.Wo <= 0) return EGN_E_BADARG;
  // 32-bit byte offsets into x (buffer loads) and 32-bit pixel indices
  if ((double)a.N * a.H * a.W * a.cs_in * 4.0 >= 2147483648.0) return EGN_E_BADARG;
  if ((double)a.N * a.Ho * a.Wo >= 2147483648.0) return EGN_E_BADARG;
  a.CoutP = (a.Cout + 15) & ~15;
  a.nchunk = cdiv(a.Cin, EGN_CK);
  a.taps = a.KH * a.KW;
  if (cfg_id >= 1 && cfg_id <= kNumConfigs) {
    const ConvConfig& cf = kConfigs[cfg_id - 1];
    if (!plan_tile(a, cf, nullptr)) return EGN_E_LDS;
  } else {
    // cost model over the staged family (the tuner explores both families)
    double best = -1.0;
    int best_id = 0;
    ConvArgs bestA = a;
    for (int k = 0; k < kNumConfigs; ++k) {
      const ConvConfig& cf = kConfigs[k];
      if (cf.family != F::Staged) continue;
      ConvArgs c = a;
      double cost;
      if (!plan_tile(c, cf, &cost)) continue;
      // mild preference for filling the chip: penalise grids below 256 blocks
      const double blocks = (double)c.tiles_x * c.tiles_y * cdiv(a.N, c.TNB) * cdiv(a.CoutP, cf.tile_n());
      if (blocks < 256.0) cost *= 256.0 / blocks > 4.0 ? 4.0 : 256.0 / blocks;
      if (best < 0 || cost < best) { best = cost; best_id = cf.id; bestA = c; }
    }
    if (best < 0) return EGN_E_LDS;
    a = bestA;
    cfg_id = best_id;
  }
  const ConvConfig& cf = kConfigs[cfg_id - 1];
  a.spix_off = searched_tile(cf) ? (int)(lds_stage_bytes(a, cf) / 16) : 0;   // (read by the Staged / Dma kernels only)
  lds_bytes = lds_bytes_for(a, cf);
  // 32-bit byte offsets into y / res (buffer stores in the NHWC epilogue)
  if (!a.out_nchw && (double)a.N * a.Ho * a.Wo * a.cs_out * 4.0 >= 2147483648.0) return EGN_E_BADARG;
  return 0;
}

// rows of the partial-statistics table a launch with a.stats != NULL writes; 0 = config without fused
// BatchNorm statistics (a must be planned for cfg_id)
int egn_conv_stats_rows(const ConvArgs& a, int cfg_id) {
  if (cfg_id < 1 || cfg_id > kNumConfigs) return 0;
  const ConvConfig& cf = kConfigs[cfg_id - 1];
  if (cf.family == F::Wino4) return cf.abl ? 0 : egn_conv_wino4_stats_rows(a, cf.kernel.wino4);     // [round 5] conv_wino4s_kernel
  return cf.family == F::Wino ? egn_conv_wino_stats_rows(a, cf.kernel.wino, cf.abl) : 0;
}

// ticket words (zeroed unsigned) a launch of cfg_id wants in a.tickets to run as ONE kernel; 0 = the config uses none
int egn_conv_ticket_count(const ConvArgs& a, int cfg_id) {
  if (cfg_id < 1 || cfg_id > kNumConfigs) return 0;
  const ConvConfig& cf = kConfigs[cfg_id - 1];
  return cf.family == F::Wino4 ? egn_conv_wino4_tickets(a, cf.kernel.wino4) : 0;
}

int egn_conv_launch(const ConvArgs& a, int cfg_id, hipStream_t stream) {
  if (cfg_id < 1 || cfg_id > kNumConfigs) return EGN_E_BADARG;
  const ConvConfig& cf = kConfigs[cfg_id - 1];
#ifndef EGN_PROBES
  if (egn_conv_config_kind(cfg_id) < 0) return EGN_E_BADARG;   // ablation / stamp / retired ids: probe builds only
#endif
  const size_t lds = lds_bytes_for(a, cf);
  switch (cf.family) {
    case F::Staged: return egn_conv_launch_staged(a, cf.kernel.direct, lds, stream);
    case F::Dma: return egn_conv_launch_dma(a, cf.kernel.direct, lds, stream);
    case F::Retired: return EGN_E_BADARG;
    case F::C48: return egn_conv_launch_c48(a, lds, cf.kernel.c48, stream);
    case F::Wino: return egn_conv_launch_wino(a, lds, cf.kernel.wino, cf.abl, stream);
    case F::Stem: return egn_conv_launch_stem(a, lds, stream);
    case F::Wino4: return egn_conv_launch_wino4(a, lds, cf.kernel.wino4, cf.abl, stream);
    case F::Fc: return egn_conv_launch_fc(a, stream);
    case F::S2r: return egn_conv_launch_s2r(a, stream);
  }
  return EGN_E_BADARG;
}
