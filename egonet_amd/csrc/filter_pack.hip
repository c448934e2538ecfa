// filter_pack.hip -- torch weights -> the packed filters of the conv kernels, on the device (training weights change
// every step: the host packers of egonet_amd/filters.py cannot feed the tape).  Two kernels over filter_pack.h's
// units: one filter per launch (the four single entries), every filter of a model in one launch (the batch entry).
// Reference: libs/trainer/trainer.py:183-209 (the weights move in every optimizer step).
#include "filter_pack.h"

// One filter: the descriptor by value.  `ld`: fp_direct_unit's row stride.
__global__ __launch_bounds__(256) void pack_one_kernel(const egn_pack_desc d, int ld, long long units) {
  for (long long le = (long long)blockIdx.x * blockDim.x + threadIdx.x; le < units;
       le += (long long)gridDim.x * blockDim.x)
    fp_unit(d, le, ld);
}

static int pack_one(const float* w, float* dst, int Cout, int Cin, int taps, int code, int ld, void* stream) {
  const long long units = fp_units(code, Cout, Cin, taps);
  if (units <= 0) return EGN_E_BADARG;
  const egn_pack_desc d = {w, dst, Cout, Cin, taps, code, 0};
  const long long g = (units + 255) / 256;
  hipLaunchKernelGGL(pack_one_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, (hipStream_t)stream, d, ld,
                     units);
  return (int)hipGetLastError();
}

// a row-major matrix as the direct filter of a 1x1 conv:
//   transpose == 0: W[co][ci] = src[co*ld + ci]   (rows = Cout)
//   transpose == 1: W[co][ci] = src[ci*ld + co]   (rows = Cin): the data-gradient view of a [cin][cout] weight
extern "C" int egn_pack_matrix_f32(const float* src, int ld, int cout, int cin, int transpose, float* dst,
                                   void* stream) {
  if (!src || !dst || cout <= 0 || cin <= 0 || ld < (transpose ? cout : cin)) return EGN_E_BADARG;
  return transpose ? pack_one(src, dst, cin, cout, 1, FP_DGRAD, ld, stream)
                   : pack_one(src, dst, cout, cin, 1, 0, ld, stream);
}

extern "C" long egn_packed_weight_floats(int Cout, int Cin, int KH, int KW, int dgrad) {
  if (KH <= 0 || KW <= 0) return -1;
  const long long f = fp_floats(dgrad ? FP_DGRAD : 0, Cout, Cin, KH * KW);
  return f ? (long)f : -1;
}
extern "C" int egn_pack_conv_weight_f32(const float* w, int Cout, int Cin, int KH, int KW, int dgrad, float* dst,
                                        void* stream) {
  if (!w || !dst || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return EGN_E_BADARG;
  return pack_one(w, dst, Cout, Cin, KH * KW, dgrad ? FP_DGRAD : 0, Cin * KH * KW, stream);
}

extern "C" long egn_wino_weight_floats(int Cout, int Cin, int dgrad) {
  return (long)fp_floats(FP_WINO2 | (dgrad ? FP_DGRAD : 0), Cout, Cin, 9);
}
extern "C" int egn_wino_pack_weight_f32(const float* w, int Cout, int Cin, int dgrad, float* dst, void* stream) {
  if (!w || !dst) return EGN_E_BADARG;
  return pack_one(w, dst, Cout, Cin, 9, FP_WINO2 | (dgrad ? FP_DGRAD : 0), 0, stream);
}

extern "C" long long egn_wino4_pack_weight_floats(int Cout, int Cin, int dgrad) {
  return fp_floats(FP_WINO4 | (dgrad ? FP_DGRAD : 0), Cout, Cin, 9);
}
extern "C" int egn_wino4_pack_weight_f32(const float* w, int Cout, int Cin, int dgrad, float* dst, void* stream) {
  if (!w || !dst) return EGN_E_BADARG;
  return pack_one(w, dst, Cout, Cin, 9, FP_WINO4 | (dgrad ? FP_DGRAD : 0), 0, stream);
}

// All filters of a model in ONE launch: the training step packs every conv weight twice per iteration (forward +
// data-gradient filter, ~600 small launches for HRNet-W48); the weights only change in the optimizer step, so the
// step packs them all up front.  descs (device memory): one egn_pack_desc per (weight, layout, direction), `begin`
// ascending; a thread finds the descriptor of its unit by binary search.
__global__ __launch_bounds__(256) void pack_conv_weights_batch_kernel(const egn_pack_desc* __restrict__ descs, int n,
                                                                      long long total) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {  // last descriptor with begin <= e
      const int mid = (lo + hi + 1) >> 1;
      if (descs[mid].begin <= e) lo = mid; else hi = mid - 1;
    }
    const egn_pack_desc d = descs[lo];
    fp_unit(d, e - d.begin);
  }
}

extern "C" int egn_pack_desc_bytes(void) { return (int)sizeof(egn_pack_desc); }

extern "C" int egn_pack_conv_weights_batch_f32(const void* descs_dev, int n, long total_float4, void* stream) {
  if (!descs_dev || n <= 0 || total_float4 <= 0) return EGN_E_BADARG;
  size_t g = ((size_t)total_float4 + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(pack_conv_weights_batch_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const egn_pack_desc*>(descs_dev), n, (long long)total_float4);
  return (int)hipGetLastError();
}
