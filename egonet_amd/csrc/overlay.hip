// overlay.hip -- draws capsules (overlay_math.h) into a batch of uint8 RGB frames in one launch, and its host twin.
//
// A 256-thread block owns a 32 x 32 pixel tile of one frame; a thread owns a run of four pixels of one row, read once
// into registers and written once (only the pixels some primitive touched).  The block walks the frame's primitives
// in chunks of OV_CAP by index: thread i tests primitive i of the chunk against the tile (the floating-point box of
// egn_overlay_reach, so end points at 1e9 need no integer), the survivors are compacted in ascending index order into
// an LDS list (wave ballot + prefix count over the four waves), and after a barrier every thread runs its pixels
// through the list.  Chunks follow each other by index and the list keeps the order inside a chunk, so painter's
// order holds; the box is conservative, so the bytes equal those of the unbinned loop.  cull = 0 sends every valid
// primitive to every tile (tools/overlay_bench.py measures what the binning buys).
// Rows are addressed by bytes: a KITTI row is 3726 bytes, no multiple of four.
#include "egn_internal.h"
#include "overlay_math.h"

namespace {

constexpr int OV_TW = 32, OV_TH = 32;      // tile
constexpr int OV_RUN = 4;                  // pixels per thread, along x
constexpr int OV_THREADS = (OV_TW / OV_RUN) * OV_TH;
constexpr int OV_CAP = OV_THREADS;         // LDS list length = chunk length: a chunk's survivors always fit
static_assert(OV_THREADS == 256, "four waves");

struct ov_frame {
  int64_t off, H, W, stride, begin, end;
};

__host__ __device__ inline bool ov_frame_ok(const int64_t* f, int n_prims, ov_frame* out) {
  out->off = f[0];
  out->H = f[1];
  out->W = f[2];
  out->stride = f[3];
  out->begin = f[4];
  out->end = f[5];
  return out->off >= 0 && out->H >= 0 && out->W >= 0 && out->H <= 0x7fffffff && out->W <= 0x7fffffff &&
         out->stride >= 3 * out->W && out->begin >= 0 && out->begin <= out->end && out->end <= (int64_t)n_prims;
}

}  // namespace

__global__ __launch_bounds__(OV_THREADS) void overlay_draw_kernel(uint8_t* __restrict__ base,
                                                                  const int64_t* __restrict__ frames,
                                                                  const float* __restrict__ prims,
                                                                  const uint32_t* __restrict__ colors, int n_prims,
                                                                  int antialias, int cull) {
  __shared__ float s_prim[OV_CAP][EGN_OVERLAY_FIELDS];
  __shared__ uint32_t s_col[OV_CAP];
  __shared__ int s_cnt[OV_THREADS / 64];
  ov_frame fr;
  // everything up to the chunk loop is uniform over the block: whole blocks leave, no thread alone
  if (!ov_frame_ok(frames + 6 * (size_t)blockIdx.z, n_prims, &fr)) return;   // a bad row draws nothing
  const int64_t tx0 = (int64_t)blockIdx.x * OV_TW, ty0 = (int64_t)blockIdx.y * OV_TH;
  if (tx0 >= fr.W || ty0 >= fr.H || fr.begin == fr.end) return;
  const int64_t tx1 = (tx0 + OV_TW < fr.W ? tx0 + OV_TW : fr.W) - 1;   // last pixel of the tile inside the frame
  const int64_t ty1 = (ty0 + OV_TH < fr.H ? ty0 + OV_TH : fr.H) - 1;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t y = ty0 + tid / (OV_TW / OV_RUN);
  const int64_t x = tx0 + (tid % (OV_TW / OV_RUN)) * OV_RUN;
  const int npx = y > ty1 || x > tx1 ? 0 : (int)(tx1 - x + 1 < OV_RUN ? tx1 - x + 1 : OV_RUN);   // 0..4 inside
  uint8_t* row = base + (size_t)fr.off + (size_t)y * (size_t)fr.stride + (size_t)x * 3;   // used only when npx > 0
  unsigned px[OV_RUN][3];
#pragma unroll
  for (int k = 0; k < OV_RUN; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) px[k][c] = k < npx ? row[3 * k + c] : 0u;
  unsigned touched = 0;

  for (int64_t c0 = fr.begin; c0 < fr.end; c0 += OV_CAP) {
    const int64_t idx = c0 + tid;
    bool hit = false;
    const float* p = prims + (size_t)(idx < fr.end ? idx : fr.begin) * EGN_OVERLAY_FIELDS;
    if (idx < fr.end && egn_overlay_valid(p)) {
      hit = true;
      if (cull) {
        const egn_overlay_prim q = egn_overlay_load(p, 0u);
        hit = egn_overlay_reaches(q, (double)tx0, (double)tx1, (double)ty0, (double)ty1);
      }
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < OV_THREADS / 64; ++w) {
      before += w < wave ? s_cnt[w] : 0;
      total += s_cnt[w];
    }
    if (hit) {
      const int pos = before + __popcll(m & ((1ull << lane) - 1ull));   // < OV_CAP: at most one per thread
#pragma unroll
      for (int k = 0; k < EGN_OVERLAY_FIELDS; ++k) s_prim[pos][k] = p[k];
      s_col[pos] = colors[idx];
    }
    __syncthreads();
    if (npx > 0) {
      for (int j = 0; j < total; ++j) {
        const egn_overlay_prim q = egn_overlay_load(s_prim[j], s_col[j]);
        if (!egn_overlay_reaches(q, (double)x, (double)(x + npx - 1), (double)y, (double)y)) continue;
#pragma unroll
        for (int k = 0; k < OV_RUN; ++k) {
          if (k >= npx) continue;
          const double w = egn_overlay_weight(q, (double)(x + k), (double)y, antialias);
          if (w > 0.0) {
            px[k][0] = egn_overlay_blend(px[k][0], q.col & 255u, w);
            px[k][1] = egn_overlay_blend(px[k][1], (q.col >> 8) & 255u, w);
            px[k][2] = egn_overlay_blend(px[k][2], (q.col >> 16) & 255u, w);
            touched |= 1u << k;
          }
        }
      }
    }
    __syncthreads();   // the list and the counts are rewritten by the next chunk
  }
#pragma unroll
  for (int k = 0; k < OV_RUN; ++k)
    if (touched & (1u << k))   // only set for k < npx
#pragma unroll
      for (int c = 0; c < 3; ++c) row[3 * k + c] = (uint8_t)px[k][c];
}

namespace {

int ov_check(const void* base, const void* frames, int n_frames, const void* prims, const void* colors, int n_prims) {
  if (n_frames < 0 || n_prims < 0) return EGN_E_BADARG;
  if (n_frames > 0 && (!base || !frames)) return EGN_E_BADARG;
  if (n_prims > 0 && (!prims || !colors)) return EGN_E_BADARG;
  return 0;
}

}  // namespace

extern "C" int egn_overlay_tile_capacity(void) { return OV_CAP; }

extern "C" int egn_overlay_draw_u8(void* base, const int64_t* frames_dev, int n_frames, int max_h, int max_w,
                                   const float* prims_dev, const uint32_t* colors_dev, int n_prims, int antialias,
                                   int cull, void* stream) {
  const int bad = ov_check(base, frames_dev, n_frames, prims_dev, colors_dev, n_prims);
  if (bad) return bad;
  if (max_h < 0 || max_w < 0 || n_frames > 65535) return EGN_E_BADARG;
  if (n_frames == 0 || n_prims == 0 || max_h == 0 || max_w == 0) return 0;
  const long gx = ((long)max_w + OV_TW - 1) / OV_TW, gy = ((long)max_h + OV_TH - 1) / OV_TH;
  if (gy > 65535) return EGN_E_BADARG;
  hipLaunchKernelGGL(overlay_draw_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n_frames), dim3(OV_THREADS), 0,
                     (hipStream_t)stream, (uint8_t*)base, frames_dev, prims_dev, colors_dev, n_prims, antialias,
                     cull);
  egn_count_launches(1);
  return (int)hipGetLastError();
}

// Host twin: the same overlay_math.h as a plain loop over HOST pointers (numpy frames / a CPU model); per primitive
// the pixel loop is clamped to the same conservative box.  Not a fallback of the device path.
extern "C" int egn_overlay_draw_host_u8(void* base, const int64_t* frames, int n_frames, const float* prims,
                                        const uint32_t* colors, int n_prims, int antialias) {
  const int bad = ov_check(base, frames, n_frames, prims, colors, n_prims);
  if (bad) return bad;
  ov_frame fr;
  for (int f = 0; f < n_frames; ++f)
    if (!ov_frame_ok(frames + 6 * (size_t)f, n_prims, &fr)) return EGN_E_BADARG;
  for (int f = 0; f < n_frames; ++f) {
    ov_frame_ok(frames + 6 * (size_t)f, n_prims, &fr);
    if (fr.H == 0 || fr.W == 0) continue;
    uint8_t* img = (uint8_t*)base + (size_t)fr.off;
    for (int64_t i = fr.begin; i < fr.end; ++i) {
      const float* p = prims + (size_t)i * EGN_OVERLAY_FIELDS;
      if (!egn_overlay_valid(p)) continue;
      const egn_overlay_prim q = egn_overlay_load(p, colors[i]);
      if (!egn_overlay_reaches(q, 0.0, (double)(fr.W - 1), 0.0, (double)(fr.H - 1))) continue;
      // the box clamped to the frame while still in floating point: it can lie at +-1e9
      const int64_t xa = q.xlo > 0.0 ? (int64_t)floor(q.xlo) : 0;
      const int64_t xb = q.xhi < (double)(fr.W - 1) ? (int64_t)ceil(q.xhi) : fr.W - 1;
      const int64_t ya = q.ylo > 0.0 ? (int64_t)floor(q.ylo) : 0;
      const int64_t yb = q.yhi < (double)(fr.H - 1) ? (int64_t)ceil(q.yhi) : fr.H - 1;
      for (int64_t y = ya; y <= yb; ++y) {
        uint8_t* row = img + (size_t)y * (size_t)fr.stride;
        for (int64_t x = xa; x <= xb; ++x) {
          const double w = egn_overlay_weight(q, (double)x, (double)y, antialias);
          if (w > 0.0) {
            uint8_t* v = row + 3 * (size_t)x;
            v[0] = (uint8_t)egn_overlay_blend(v[0], q.col & 255u, w);
            v[1] = (uint8_t)egn_overlay_blend(v[1], (q.col >> 8) & 255u, w);
            v[2] = (uint8_t)egn_overlay_blend(v[2], (q.col >> 16) & 255u, w);
          }
        }
      }
    }
  }
  return 0;
}
