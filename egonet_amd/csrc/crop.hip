// crop.hip -- GPU crop front end.
//
// Reference call site: libs/model/egonet.py:68-96 crop_single_instance():
//     trans = get_affine_transform(c, s, 0, (height, width))          img_proc.py:26-64
//     instance = cv2.warpAffine(img, trans, (res0, res1), flags=cv2.INTER_LINEAR)
//     instance = pth_trans(instance)      # ToTensor (/255, HWC->CHW) + Normalize(mean, std)
//                                         # libs/dataset/KITTI/car_instance.py:522-531
// one call per bounding box on the host.  Here: the uint8 image is uploaded once,
// one launch produces the normalised fp32 NCHW crops of ALL its boxes -- what the
// backbone consumes -- so neither the per-box warp nor the 786 KB/crop fp32
// host->device copy exists any more.
//
// cv2 (OpenCV 3.4.2, docs/spec-list.txt) is third party and absent here: PARITY
// UNPINNED.  The kernel restates the published algorithm of cv::warpAffine for
// 8-bit INTER_LINEAR (modules/imgproc/src/imgwarp.cpp): invert the 2x3 matrix in
// double; source coordinates in fixed point with AB_BITS = 10, rounded (half to
// even) per row / per column term, + round_delta 16, shifted to INTER_BITS = 5
// (1/32 pixel); bilinear weights (32-fx)(32-fy).. as 15-bit integers (exactly
// 32x the products, so no table fix-up applies); result (sum + 2^14) >> 15;
// BORDER_CONSTANT 0 per tap.
#include "egn_internal.h"

// The per-pixel scheme exists once (the __device__ helpers below) and serves both entries: the
// one-frame launch of inference and the multi-frame launch of the training-sample front end
// (common/train_samples.py), which cuts the crops of every box of a batch of frames in one launch.

// dst -> src map (cv::warpAffine without WARP_INVERSE_MAP inverts M)
struct InvAffine {
  double i0, i1, i2, i3, i4, i5;
};

__device__ __forceinline__ InvAffine invert_affine(const double* m) {
  double D = m[0] * m[4] - m[1] * m[3];
  D = D != 0.0 ? 1.0 / D : 0.0;
  InvAffine q;
  q.i0 = m[4] * D, q.i1 = -m[1] * D, q.i3 = -m[3] * D, q.i4 = m[0] * D;
  q.i2 = -q.i0 * m[2] - q.i1 * m[5], q.i5 = -q.i3 * m[2] - q.i4 * m[5];
  return q;
}

// per-row term round((a*y + b) * 2^AB_BITS) + round_delta, per-column term round(a*x * 2^AB_BITS)
__device__ __forceinline__ int fx_row(double a, double b, int y) { return (int)rint((a * y + b) * 1024.0) + 16; }
__device__ __forceinline__ int fx_col(double a, int x) { return (int)rint(a * x * 1024.0); }

// One destination pixel: X, Y = row term + column term (1/1024 px, rounding delta included); v[c] the
// bilinear 8-bit level of channel c with BORDER_CONSTANT 0 per tap.
__device__ __forceinline__ void warp_px_u8(const uint8_t* img, int H, int W, int pitch, int X, int Y, int v[3]) {
  X >>= 5, Y >>= 5;
  const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
  const bool x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
  const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H;
  const uint8_t* r0 = img + (size_t)(y0 ? sy : 0) * pitch;
  const uint8_t* r1 = img + (size_t)(y1 ? sy + 1 : 0) * pitch;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int p00 = (y0 && x0) ? r0[sx * 3 + c] : 0;
    const int p01 = (y0 && x1) ? r0[(sx + 1) * 3 + c] : 0;
    const int p10 = (y1 && x0) ? r1[sx * 3 + c] : 0;
    const int p11 = (y1 && x1) ? r1[(sx + 1) * 3 + c] : 0;
    v[c] = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10;
  }
}

// ToTensor: float / 255, Normalize: (t - mean) / std, both in fp32
__device__ __forceinline__ float normalize_level(int v, float mean, float stdv) { return ((float)v / 255.f - mean) / stdv; }

struct CropArgs {
  const uint8_t* img;  // [H][W][3] RGB, row stride `pitch` bytes
  const double* M;     // [n][6] forward affine (image -> crop), row major 2x3
  const float* mean;   // [3]
  const float* stdv;   // [3]
  float* out;          // [n][3][oh][ow]
  int H, W, pitch, n, oh, ow;
};

__global__ __launch_bounds__(256) void crop_warp_normalize_kernel(CropArgs a) {
  const size_t per = (size_t)a.oh * a.ow;
  const size_t total = (size_t)a.n * per;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(e % a.ow);
    const int y = (int)((e / a.ow) % a.oh);
    const int i = (int)(e / per);
    const InvAffine q = invert_affine(a.M + (size_t)i * 6);
    int v[3];
    warp_px_u8(a.img, a.H, a.W, a.pitch, fx_row(q.i1, q.i2, y) + fx_col(q.i0, x), fx_row(q.i4, q.i5, y) + fx_col(q.i3, x),
               v);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      a.out[((size_t)i * 3 + c) * per + (size_t)y * a.ow + x] = normalize_level(v[c], a.mean[c], a.stdv[c]);
  }
}

extern "C" int egn_crop_warp_normalize_u8(const uint8_t* img, int H, int W, int pitch, const double* M, int n,
                                          int out_h, int out_w, const float* mean, const float* stdv, float* out,
                                          void* stream) {
  if (!img || !M || !mean || !stdv || !out || H <= 0 || W <= 0 || pitch < 3 * W || n <= 0 || out_h <= 0 ||
      out_w <= 0)
    return EGN_E_BADARG;
  CropArgs a = {img, M, mean, stdv, out, H, W, pitch, n, out_h, out_w};
  const size_t total = (size_t)n * out_h * out_w;
  size_t g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(crop_warp_normalize_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// ---- multi-frame launch -----------------------------------------------------------------------------
// One block = one box x kRows output rows.  The inverse affine, the kRows row terms and the box's column
// terms (LDS, 2 x out_w ints) are made once per block; a lane then owns 4 consecutive x of one row and
// writes them as one 16 B store per channel.  The kernel only gathers (frame bytes, cache resident) and
// writes: 140 crops of 256^2 are 110 MB out.
constexpr int kCropRows = 16;

struct FramesArgs {
  const uint8_t* frames;  // all frames, packed
  const long long* tab;   // [n_frames][4] byte offset, H, W, row pitch (bytes)
  const int* box_frame;   // [n] frame index of each box
  const double* M;        // [n][6] forward affines image -> crop
  const float* mean;
  const float* stdv;
  float* out;             // [n][3][oh][ow]
  int n_frames, oh, ow, vec;
};

__global__ __launch_bounds__(256) void crop_frames_warp_normalize_kernel(FramesArgs a) {
  extern __shared__ int col_terms[];  // [2][ow]: x and y column terms
  __shared__ int row_x[kCropRows], row_y[kCropRows];
  const int i = blockIdx.y;
  const int y0 = blockIdx.x * kCropRows;
  const int rows = min(kCropRows, a.oh - y0);
  const InvAffine q = invert_affine(a.M + (size_t)i * 6);
  int* cx = col_terms;
  int* cy = col_terms + a.ow;
  for (int x = threadIdx.x; x < a.ow; x += blockDim.x) cx[x] = fx_col(q.i0, x), cy[x] = fx_col(q.i3, x);
  if ((int)threadIdx.x < rows) {
    row_x[threadIdx.x] = fx_row(q.i1, q.i2, y0 + threadIdx.x);
    row_y[threadIdx.x] = fx_row(q.i4, q.i5, y0 + threadIdx.x);
  }
  __syncthreads();
  // an index outside the table reads nothing (H = W = 0: every tap is border)
  const int f = a.box_frame[i];
  const bool ok = f >= 0 && f < a.n_frames;
  const uint8_t* img = a.frames + (ok ? a.tab[(size_t)f * 4 + 0] : 0);
  const int H = ok ? (int)a.tab[(size_t)f * 4 + 1] : 0;
  const int W = ok ? (int)a.tab[(size_t)f * 4 + 2] : 0;
  const int pitch = ok ? (int)a.tab[(size_t)f * 4 + 3] : 0;
  const float m0 = a.mean[0], m1 = a.mean[1], m2 = a.mean[2];
  const float s0 = a.stdv[0], s1 = a.stdv[1], s2 = a.stdv[2];
  const size_t per = (size_t)a.oh * a.ow;
  const int quads = (a.ow + 3) >> 2;
  for (int e = threadIdx.x; e < rows * quads; e += blockDim.x) {
    const int r = e / quads;
    const int x = (e - r * quads) * 4;
    float o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int v[3] = {0, 0, 0};
      if (x + j < a.ow) warp_px_u8(img, H, W, pitch, row_x[r] + cx[x + j], row_y[r] + cy[x + j], v);
      o[0][j] = normalize_level(v[0], m0, s0);
      o[1][j] = normalize_level(v[1], m1, s1);
      o[2][j] = normalize_level(v[2], m2, s2);
    }
    float* dst = a.out + (size_t)i * 3 * per + (size_t)(y0 + r) * a.ow + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a.vec) {
        *reinterpret_cast<float4*>(dst + c * per) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < a.ow) dst[c * per + j] = o[c][j];
      }
    }
  }
}

extern "C" int egn_crop_frames_warp_normalize_u8(const uint8_t* frames, const long long* frame_tab, int n_frames,
                                                 const int* box_frame, const double* M, int n, int out_h, int out_w,
                                                 const float* mean, const float* stdv, float* out, void* stream) {
  if (!frames || !frame_tab || !box_frame || !M || !mean || !stdv || !out || n_frames <= 0 || n <= 0 || n > 65535 ||
      out_h <= 0 || out_w <= 0 || out_w > 4096)
    return EGN_E_BADARG;
  FramesArgs a = {frames, frame_tab, box_frame, M, mean, stdv, out, n_frames, out_h, out_w,
                  (out_w % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0};
  const dim3 grid((unsigned)((out_h + kCropRows - 1) / kCropRows), (unsigned)n);
  hipLaunchKernelGGL(crop_frames_warp_normalize_kernel, grid, dim3(256), 2 * out_w * sizeof(int), (hipStream_t)stream,
                     a);
  egn_count_launches(1);
  return (int)hipGetLastError();
}
