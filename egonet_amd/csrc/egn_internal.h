// Internal declarations shared by the HIP translation units of libegonet_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/egonet_hip.h"

// hipFuncSetAttribute is per device: a flag per device (the reference drives several GPUs from one
// process through nn.DataParallel, one thread each), set on the first launch there
constexpr int EGN_MAX_DEVICES = 64;
static inline bool egn_first_use_on_device(bool* seen) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= EGN_MAX_DEVICES) return true;
  if (seen[d]) return false;
  seen[d] = true;
  return true;
}

#define EGN_CHECK_HIP(expr)                      \
  do {                                           \
    hipError_t _e = (expr);                      \
    if (_e != hipSuccess) return (int)_e;        \
  } while (0)

// A kernel whose dynamic LDS exceeds 64 KB is allowed `bytes` of it on the first launch on each device (`raised`: the
// launcher's own static bool[EGN_MAX_DEVICES]).  EGN_BIG_LDS_BYTES: all a workgroup can have on the 160 KB CU.
constexpr int EGN_BIG_LDS_BYTES = 160 * 1024 - 512;
template <class Kernel>
static inline hipError_t egn_allow_big_lds(Kernel kernel, int bytes, bool* raised) {
  if (!egn_first_use_on_device(raised)) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// CUs of the CURRENT device, looked up once per device; 256 where no device answers
inline int egn_device_cus() {
  static int cus[EGN_MAX_DEVICES];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= EGN_MAX_DEVICES) return 256;
  if (!cus[d]) {
    hipDeviceProp_t prop;
    cus[d] = hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus[d];
}
// Grid of a persistent kernel: all nwork items if they fit blocks_per_cu blocks on every CU, else whole rounds of
// `round` blocks (8 XCDs x the co-tiles: the items w, w + grid, ... of a block then share their co-tile), at least one
static inline int egn_persistent_grid(int nwork, int round, int blocks_per_cu = 1) {
  int cap = blocks_per_cu * egn_device_cus() / round * round;
  if (cap <= 0) cap = round;
  return nwork < cap ? nwork : cap;
}

// ceil(2^32 / d) for egn_udiv_magic (conv_common.h); 0 = the divisor is 1
static inline unsigned egn_magic_u32(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); }

// conv chunking constants (the packed-weight format depends on them)
constexpr int EGN_CK = 16;          // input channels per K chunk
constexpr int EGN_CKQ = EGN_CK / 4; // float4 planes per chunk

struct ConvArgs {
  const float* x;
  const float* w;
  const float* scale;
  const float* shift;
  const float* res;
  float* y;
  int N, H, W, Cin, cs_in;
  int Ho, Wo, Cout, cs_out, CoutP;
  int KH, KW, stride, pad;
  int TH, TW, TNB;   // output tile: TNB images x TH rows x TW cols
  int HH, HW;        // input (halo) tile dims per image
  int npix, npixp;   // halo pixels per tile, rounded up to 16
  int tiles_x, tiles_y;
  int nchunk, taps, tps;  // K chunks, taps = KH*KW, taps per LDS stage
  int act, out_nchw;
  int spix_off;  // LDS offset (float4 units) of the tile-row -> output-pixel table
  // training: per-(tile, wave) partial column sums of the stored outputs, [row][2][Cout] doubles
  // (sum, sum of squares), written by the kernels that support it (conv_wino8_kernel); NULL = off
  double* stats;
  // conv_wino9_kernel: multipliers ceil(2^32 / d) for the item index divisions by nct, tiles_x * tiles_y and
  // tiles_x (0 = the divisor is 1), set by its launcher -- the divisions run on the scalar unit
  unsigned mg_nct, mg_txy, mg_tx;
  // conv_wino4c_kernel<., 2> (input channels of an item split over two blocks): one zeroed word per item pair,
  // egn_conv_ticket_count() of them -- the second block to finish applies the epilogue.  NULL: the launcher zeroes y,
  // both blocks add into it and conv_wino4_finish_kernel applies the epilogue (three launches instead of one).
  unsigned* tickets;
};

// the shared opening of the F(4x4,3x3) `applies` predicates: 3x3, stride 1, pad 1, NHWC with unpadded channel
// strides, activation none / ReLU applied after the residual
static inline bool egn_plain_3x3_s1(const ConvArgs& a) {
  return a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.cs_in == a.Cin && a.cs_out == a.Cout && !a.out_nchw &&
         !(a.act & EGN_ACT_RES_AFTER) &&
         ((a.act & EGN_ACT_MASK) == EGN_ACT_NONE || (a.act & EGN_ACT_MASK) == EGN_ACT_RELU);
}

// One row of kConfigs (conv_plan.hip) says everything about a config id: which family launches it, which of the
// family's kernels, on which tile, with which filter packing, in which build.  Nothing is decoded from it elsewhere.
enum class ConvFamily {
  Staged,   // global -> registers -> LDS, searched tile (conv_mfma.hip)
  Dma,      // LDS-DMA double-buffered pipeline, searched tile (conv_dma.hip)
  Retired,  // reserved ids: never planned, never launched
  C48,      // filter-resident persistent kernels of the 48 -> 48 3x3 layers (conv_c48.hip)
  Wino,     // fused Winograd F(2x2,3x3) and the first F(4x4,3x3) kernel (conv_wino.hip)
  Stem,     // 3x3 s2, 3 -> 64 channels (conv_stem.hip)
  Wino4,    // fused Winograd F(4x4,3x3) (conv_wino4.hip, conv_wino4w/h/r.hip)
  Fc,       // 1x1 row GEMM (conv_fc.hip)
  S2r,      // 3x3 s2 from the 48-channel branch (conv_s2r.hip)
};
// the kernel within its family; the geometry suffix is TH x TW [x TNB images]
enum DirectTile {   // Staged / Dma: block tile M x N (output pixels x output channels)
  T256x48, T128x96, T128x64, T256x16, T256x32, T128x48, T64x96, T64x64, T64x64_NWaves, T32x192
};
enum C48Kernel { C48_Waves4, C48_Waves8, C48_RegFilter, C48_Ring };
enum WinoKernel {
  Wino_16x16, Wino_8x8x4,                                  // conv_wino_kernel (4 waves)
  Wino8_16x16, Wino8_8x8x4, Wino8_8x8x2, Wino8_8x16,       // conv_wino8_kernel (8 waves; 8x8x2 / 8x16: 4 waves)
  Wino9_16x16, Wino9_8x8x4, Wino9_8x8x2, Wino9_8x16,       // conv_wino9_kernel on the same tiles
  Wino9h_8x16, Wino9h_8x8x2,                               // conv_wino9_kernel with 8-channel stages, two blocks per CU
  Wino43,                                                  // conv_wino43_kernel: F(4x4,3x3)
};
enum Wino4Kernel {
  Wino4,                    // conv_wino4_kernel: 16 x 32 regions
  Wino4b, Wino4b_KSplit,    // conv_wino4b_kernel / conv_wino4bk_kernel: 16 x 16 regions
  Wino4c, Wino4c_KSplit,    // conv_wino4c_kernel<., 1 / 2>: four 8 x 8 images per region
  Wino4w,                   // conv_wino4w_kernel: 16 x 16 regions x 96 output channels per item
  Wino4h, Wino4d,           // conv_wino4h_kernel / conv_wino4d_kernel: half-size blocks
  Wino4r,                   // conv_wino4r_kernel: row-owner waves, 16 x 32 regions
};
union ConvKernel {          // the member ConvConfig::family names; families with one kernel leave it empty
  int none;
  DirectTile direct;
  C48Kernel c48;
  WinoKernel wino;
  Wino4Kernel wino4;
  constexpr ConvKernel() : none(0) {}
  constexpr ConvKernel(DirectTile k) : direct(k) {}
  constexpr ConvKernel(C48Kernel k) : c48(k) {}
  constexpr ConvKernel(WinoKernel k) : wino(k) {}
  constexpr ConvKernel(Wino4Kernel k) : wino4(k) {}
};

struct ConvConfig {
  int id;
  // Staged / Dma: waves in M / N, 16x16 sub-tiles per wave in M / N.  Other families: wm = waves of a block and a
  // nominal tile; egn_conv_plan_query exports the four for every id
  int wm, wn, mt, nt;
  ConvFamily family;
  ConvKernel kernel;
  int abl;           // the kernel's ABL / CLK template argument: 0 = the real kernel, else a timing-ablation or stamp build
  int kind;          // filter packing as egn_conv_config_kind returns it; -1 = not selectable (ablation / stamp / retired)
  bool probe_only;   // compiled, planned and launched by -DEGN_PROBES builds only
  struct {           // Staged / Dma (searched tile): dwordx4 staging loads per lane for the halo tile / the weights of a
    int ai, bi;      // stage, and the LDS budget in KiB the search keeps a block within
    int lds_kb;
  } staging;
  struct {           // every other family: the fixed output tile (TNB images x TH rows x TW cols), taps per stage, and
    int TH, TW, TNB, tps;   // the input (halo) tile where it is not (TH + 2) x (TW + 2)
    int HH, HW;
  } tile;
  const char* name;  // kernel symbol as rocprofv3 prints it (Staged / Dma: formatted from wm..nt, egn_conv_config_name)
  int tile_m() const { return wm * mt * 16; }
  int tile_n() const { return wn * nt * 16; }
};

// co-tile of the Winograd kernels (conv_wino.hip): 48 where Cout allows, else 32, 0 = not supported
__host__ __device__ inline int egn_wino_cot(int cout) { return cout % 48 == 0 ? 48 : (cout % 32 == 0 ? 32 : 0); }

int egn_conv_launch(const ConvArgs& a, int cfg_id, hipStream_t stream);
int egn_conv_plan(ConvArgs& a, int& cfg_id, size_t& lds_bytes);
const ConvConfig* egn_conv_config(int cfg);
int egn_conv_stats_rows(const ConvArgs& a, int cfg_id);
int egn_conv_ticket_count(const ConvArgs& a, int cfg_id);   // a planned for cfg_id; 0 = the config uses none

// The paired F(4x4,3x3) launch (conv_wino4.hip): a planned for cfg 86 (conv_wino4w_kernel), b for cfg 82
// (conv_wino4c_kernel<0, 1>).  egn_conv_pair_plan is host-only: 0 and the two grid shares (multiples of 8) where the
// pair applies (both kernels take their shape, no BatchNorm statistics, no ticket words), else EGN_E_BADARG.
constexpr int EGN_PAIR_CFG_A = 86, EGN_PAIR_CFG_B = 82;
int egn_conv_pair_plan(const ConvArgs* a, const ConvArgs* b, int cus, int* blocks_a, int* blocks_b);
int egn_conv_launch_wino4_pair(ConvArgs a, ConvArgs b, int cus, hipStream_t stream);   // cus <= 0: the device's

// The f16-operand 3x3 / pad 1 family (conv_h.hip), stride 1 and stride 2: beside the config table, planned by its own
// predicates.
struct ConvHArgs {
  const float* x;      // (x16: f16)
  const void* w;       // engine.pack_conv_weight_f16 (ck = 48) / pack_conv_weight_f16x (ck = 32)
  const float* scale;
  const float* shift;
  const float* res;    // stride 1 only
  float* y;            // (y16: f16)
  int N, H, W, Cin, Cout, act;
  int stride;          // 1 or 2
  int Ho, Wo;          // output size: (H - 1) / stride + 1, (W - 1) / stride + 1
  int ck;              // input channels per chunk: 48 (egn_conv_h_plan) or 32 (egn_conv_hx_plan)
  int tn;              // output channels per block: 96 / 64 on 64 pixels, 48 / 32 on 128 (stride 2: 64) pixels
  int TH, TW, TNB;     // output tile (powers of two): TNB images x TH rows x TW cols
  int lth, ltw;        // log2 of TH / TW
  int HH, HW, npix;    // halo tile per image (stride * T + 3 - stride a side), halo pixels per block
  int tiles_x, tiles_y;
  int tab_bytes, lds_bytes, blocks;
  int x16, y16;        // 1: x / y is stored as f16, the rounding of the staging applied by the producer (egn_conv_h16_plan)
};
int egn_conv_h_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int has_res, int act, int stride);   // host-only
// the 32-multiple widths in chunks of 32 (egn_conv3x3_hx_applies; precision = 'f16x'), either stride
int egn_conv_hx_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int has_res, int act, int stride);  // host-only
// either chunk size (ck) with f16 storage of x and / or y (egn_conv3x3_h16_applies)
int egn_conv_h16_plan(ConvHArgs& a, int N, int H, int W, int Cin, int Cout, int has_res, int act, int stride, int ck, int x16,
                      int y16);                                                                                    // host-only
int egn_conv_h_launch(const ConvHArgs& a, hipStream_t stream);

// adds n to egn_launch_count() (program.hip): entry points outside programs that want their launches provable
void egn_count_launches(long n);
