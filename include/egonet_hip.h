/*
 * egonet_hip.h -- C ABI of the MI355X (gfx950) hot-path library of egonet_amd.
 *
 * The reference (Nicholasli1995/EgoNet) is pure Python on torch.nn: it has no
 * FFI of its own.  Each entry point below replaces the ATen op sequence issued
 * by the cited reference lines; the Python host layer (egonet_amd/model/...)
 * mirrors the reference's operator API (get_pose_net / get_fc_model / EgoNet)
 * and reaches these functions through ctypes.
 *
 * Conventions
 *   - every function returns int: 0 = ok, >0 = hipError_t, <0 = EGN_E_* below;
 *     no exception crosses this boundary.
 *   - all pointers are DEVICE pointers owned by the caller (torch tensors);
 *     the library never allocates user-visible memory.
 *   - `stream` is a hipStream_t passed as void*; nothing synchronises.
 *   - activations are fp32 NHWC with a channel stride `cs` (multiple of 4,
 *     pad channels hold zeros) unless a parameter says NCHW.
 */
#ifndef EGONET_HIP_H
#define EGONET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGN_E_BADARG   (-1)   /* inconsistent shapes / unsupported parameter  */
#define EGN_E_LDS      (-2)   /* tile does not fit in the 160 KiB LDS          */
#define EGN_E_STATE    (-3)   /* program used in the wrong state               */

#define EGN_ACT_NONE    0
#define EGN_ACT_RELU    1
#define EGN_ACT_SIGMOID 2
#define EGN_ACT_LEAKY   3     /* slope 0.01 (torch LeakyReLU default)          */
#define EGN_ACT_MASK    0x0f
#define EGN_ACT_RES_AFTER 0x10 /* flag: y = res + act(..) instead of act(.. + res)
                                  (FCmodel.py:34-43: out = x + relu(bn(w2(..))))  */

/* library / ABI version: (major<<16)|minor */
int egn_version(void);
/* human readable text for a return code (static storage) */
const char* egn_strerror(int code);

/* ------------------------------------------------------------------------
 * Convolution as fp32-MFMA implicit GEMM, fused  y = act(conv(x)*scale+shift
 * (+res)).  Replaces Conv2d+BatchNorm2d(+add)+ReLU chains:
 *   hrnet.py:76-92 (BasicBlock), :113-133 (Bottleneck), :232-274 (fuse convs),
 *   :482-507 (transitions), :318-323 (stem), :365-371/:427-435 (1x1 heads),
 *   :457 (4x4 valid conv + Sigmoid); FCmodel.py:33-43,92-105 (Linear+BN1d as
 *   1x1 conv on [N,1,1,C]).
 *
 * x      [N,H,W,cs_in]  fp32 NHWC
 * wpack  weights prepacked by egn_conv_pack_size/egonet_amd.engine.pack_conv:
 *        [nchunk][KH*KW][CK/4][CoutP][4] fp32, CK = 16 input channels per chunk,
 *        CoutP = Cout rounded up to 16, zero padded
 * scale, shift  [CoutP] fp32 (folded BatchNorm / bias), zero padded
 * res    optional residual [N,Ho,Wo,cs_out] (NULL = none), added before act
 * y      [N,Ho,Wo,cs_out] NHWC, or [N,Cout,Ho,Wo] when out_nchw != 0
 * cfg    tile configuration id (0 = choose automatically)
 * ---------------------------------------------------------------------- */
int egn_conv2d_f32(const float* x, const float* wpack, const float* scale,
                   const float* shift, const float* res, float* y,
                   int N, int H, int W, int Cin, int cs_in,
                   int Cout, int cs_out, int KH, int KW, int stride, int pad,
                   int act, int out_nchw, int cfg, void* stream);

/* Host-only: the launch plan egn_conv2d_f32 would use (no GPU needed).
 * out[0..11] = cfg, wm, wn, mt, nt, TH, TW, TNB, taps_per_stage, lds_bytes,
 *              grid_x, grid_y */
int egn_conv_plan_query(int N, int H, int W, int Cin, int cs_in, int Cout,
                        int cs_out, int KH, int KW, int stride, int pad,
                        int out_nchw, int cfg, int* out);

/* Host-only: 0 where config cfg takes the shape for a caller with (has_res) or
 * without a residual in another buffer -- egn_conv_plan_query is not told about
 * the residual; the stem and stride-2 kernels and an NCHW output take none. */
int egn_conv_plan_takes(int N, int H, int W, int Cin, int cs_in, int Cout,
                        int cs_out, int KH, int KW, int stride, int pad,
                        int has_res, int out_nchw, int cfg);

/* number of tile configurations compiled in; valid ids are 1..count */
int egn_conv_num_configs(void);
/* describe config id: tile_m (output pixels), tile_n (output channels) */
int egn_conv_config_info(int cfg, int* tile_m, int* tile_n);
/* kernel symbol of config id as rocprofv3 prints it, NUL terminated into buf */
int egn_conv_config_name(int cfg, char* buf, int len);
/* which filter packing config id expects in `wpack`:
 *   0  direct kernels: egn_pack_conv_weight_f32 (layout above)
 *   1  fused Winograd F(2x2,3x3) kernels (3x3, stride 1, pad 1, Cin % 16 == 0,
 *      Cout % 48 == 0 or -- the 8-wave kernels -- Cout % 32 == 0, unpadded channel
 *      strides, act none/ReLU): the TRANSFORMED filter from egn_wino_pack_weight_f32
 *   2  fused Winograd F(4x4,3x3), conv_wino43_kernel: U = G g G^T for points 0, +-1, +-2,
 *      inf packed [Cout/48][Cin/4][f = 6i+j][ci % 4][48] (host: engine.pack_wino43_weight)
 *   3  fused Winograd F(4x4,3x3), conv_wino4_kernel / conv_wino4b_kernel / conv_wino4c_kernel (3x3,
 *      stride 1, pad 1, Cin % 16 == 0, Cout % 48 == 0, maps of whole 16 x 32 / 16 x 16 pixel regions
 *      or 8 x 8 maps): the same U packed for register feeding, [Cout/48][k-group Cin/4][wave 12][3]
 *      [64 lanes][4] floats (9 of 12 used) (egn_wino4_weight_floats; host: engine.pack_wino4_weight).
 *      Configs 83 / 84 (8 x 8 maps / 16 x 16 regions, input channels of a work item split over two
 *      blocks; Cin % 32 == 0):
 *      called through egn_conv2d_f32 it is THREE launches on `stream` (y zeroed, atomic adds, in-place
 *      epilogue; res must not alias y); as an op of a program it is one launch.
 *  -1  not selectable: invalid id, retired family, timing-ablation / stamp build.  The product
 *      library neither plans nor launches such an id (egn_conv2d_f32 returns EGN_E_BADARG);
 *      a probe build (-DEGN_PROBES, tools/ only) compiles them. */
int egn_conv_config_kind(int cfg);
/* 1 = this library is a probe build (python -m egonet_amd.build --probes), 0 = the product */
int egn_probe_build(void);
/* floats of the kind-3 filter of a [Cout][Cin][3][3] weight (0 = shape not supported) */
long long egn_wino4_weight_floats(int Cout, int Cin);
/* The kind-3 filter transform on the device: torch weight [Cout][Cin][3][3] -> U = G g G^T (float64
 * arithmetic, rounded once to fp32) in the register-feed layout of kind 3 -- the device form of
 * engine.pack_wino4_weight; dgrad 1 = the data-gradient filter (channels swapped, taps rotated by
 * 180 degrees).  egn_wino4_pack_weight_floats = floats dst must hold (0 = shape not supported:
 * output channels % 48, input channels % 8, >= 16).  Replaces nothing in the reference (cuDNN
 * transforms filters internally for the Conv2d calls of hrnet.py:24-27); it is what lets weights
 * that change every step (libs/trainer/trainer.py:183-209) feed the F(4x4,3x3) kernels. */
long long egn_wino4_pack_weight_floats(int Cout, int Cin, int dgrad);
int egn_wino4_pack_weight_f32(const float* w, int Cout, int Cin, int dgrad, float* dst, void* stream);
/* Winograd filter transform on the device: torch weight [Cout][Cin][3][3] ->
 * U = G g G^T (float64 arithmetic, rounded once to fp32) packed as
 * [Cout/T][Cin/16][f = 4i+j][quad][T][4] floats (ci = chunk*16 + quad*4 + r),
 * T = 48 if Cout % 48 == 0 else 32 (Cout % 32 == 0): one contiguous slab per
 * (output-channel tile, input-channel chunk).
 * dgrad 1 = the data-gradient filter (channels swapped, taps rotated 180 deg).
 * egn_wino_weight_floats = floats dst must hold (0 = shape not supported).
 * Replaces nothing in the reference (cuDNN picks its Winograd algorithms
 * internally for the Conv2d calls of hrnet.py:24-27); it is the packing step of
 * this library's 3x3 kernels. */
long egn_wino_weight_floats(int Cout, int Cin, int dgrad);
int egn_wino_pack_weight_f32(const float* w, int Cout, int Cin, int dgrad,
                             float* dst, void* stream);

/* ------------------------------------------------------------------------
 * Multi-resolution fuse: y = relu( ((t0 + up(t1)) + up(t2)) + up(t3) ),
 * left-associated in the order given (hrnet.py:291-298); up() = nearest
 * neighbour by 2^shift (hrnet.py:241), shift 0 = same resolution.
 * All tensors NHWC with channel stride cs; y is [N,H,W,cs]; t_i is
 * [N,H>>s_i,W>>s_i,cs].  nterms in 1..4.
 * ---------------------------------------------------------------------- */
int egn_fuse_sum_relu_f32(float* y, int N, int H, int W, int C, int cs,
                          int nterms, const float* const* terms,
                          const int* shifts, int relu, void* stream);

/* layout helpers at the module boundary (reference tensors are NCHW) */
int egn_nchw_to_nhwc_f32(const float* x, float* y, int N, int C, int H, int W,
                         int cs, void* stream);
int egn_nhwc_to_nchw_f32(const float* x, float* y, int N, int C, int H, int W,
                         int cs, void* stream);
/* nn.PixelShuffle(up) of the heat-map upsampler (hrnet.py:373-383, 598-600) fused with
 * the NHWC -> NCHW hand-over: y[n,j,h*up+a,w*up+b] = x[n,h,w,(j*up+a)*up+b];
 * x [N,H,W,cs] with cs >= C*up*up, y [N,C,H*up,W*up] */
int egn_pixel_shuffle_nhwc_to_nchw_f32(const float* x, float* y, int N, int C,
                                       int H, int W, int cs, int up, void* stream);
/* nn.PixelUnshuffle(up) fused with the NCHW -> padded NHWC hand-over, the exact inverse of
 * egn_pixel_shuffle_nhwc_to_nchw_f32: y[n,h,w,(j*up+a)*up+b] = x[n,j,h*up+a,w*up+b], pad
 * channels (>= C*up*up) zero; x [N,C,H*up,W*up], y [N,H,W,cs], cs % 4 == 0 (the backward of
 * the pixel-shuffle head under the autograd bridge) */
int egn_pixel_unshuffle_nchw_to_nhwc_f32(const float* x, float* y, int N, int C, int H,
                                         int W, int cs, int up, void* stream);
/* write the two coordinate ramps linspace(0,1) (hrnet.py:461-467) into
 * channels [c0, c0+1] of an NHWC tensor */
int egn_fill_coord_ramps_f32(float* y, int N, int H, int W, int cs, int c0,
                             void* stream);

/* ------------------------------------------------------------------------
 * Key-point decode, one wavefront per (n,k) map (img_proc.py:608-637 hard
 * arg-max, :678-707 soft-arg-max).  hm is NCHW [N,K,H,W].
 *   out_xy   [N,K,2] fp32   (x,y) in heat-map pixels
 *   out_max  [N,K]   fp32   raw maximum
 *   out_idx  [N,K]   int32  flat arg-max index (first max on ties); may be NULL
 * mode 0 = hard arg-max (coordinates zeroed where max <= 0),
 * mode 1 = soft-arg-max (softmax over H*W, no mask),
 * mode 2 = soft_arg_max_np (img_proc.py:639-676: weights hm/sum(hm),
 *          coordinates zeroed where max <= 0).
 * ---------------------------------------------------------------------- */
int egn_decode_heatmaps_f32(const float* hm, int N, int K, int H, int W,
                            int mode, float* out_xy, float* out_max,
                            int32_t* out_idx, void* stream);

/* ------------------------------------------------------------------------
 * Crop-local key-points -> screen coordinates -> normalised lifter input
 * (egonet.py:436-453 + img_proc.py:26-78 with rot=0, operations.py:20-47).
 *   local   [n,K,2] fp32, multiplied by (mul_x, mul_y) first
 *           (coords head: resolution; soft-arg-max: input/heatmap size)
 *   center  [n,2] f64, scale [n,2] f64 (modify_bbox outputs), crop size (cw,ch)
 *   screen  [n,K*2] f64 out (records['kpts_2d_pred'])
 *   mean_in, std_in [K*2] f64;  lifter_in [n, ld_in] fp32 out (may be NULL)
 * ---------------------------------------------------------------------- */
int egn_keypoints_to_screen_f64(const float* local, int n, int K,
                                double mul_x, double mul_y,
                                const double* center, const double* scale,
                                int crop_w, int crop_h, double* screen,
                                const double* mean_in, const double* std_in,
                                float* lifter_in, int ld_in, void* stream);

/* pred3d[n,D] f64 = y[n,ld] fp32 * std_out + mean_out  (operations.py:49-51): the product rounded, then the sum, as
 * numpy does (no fused multiply-add), so the result is the reference's bit for bit */
int egn_unnormalize_f64(const float* y, int n, int D, int ld,
                        const double* mean_out, const double* std_out,
                        double* pred3d, void* stream);

/* ------------------------------------------------------------------------
 * Batched pose solve (egonet.py:238-295, transformation.py:99-134,
 * egonet.py:203-236): cuboid template from mean edge lengths, Kabsch
 * rotation by 3x3 SVD, euler 'yxz' -> (x,y,z) order, observation angle.
 *   pred3d [n,32,3] f64;  kpt_x [n] f64 = screen x of key-point 0 (proj mode)
 *   euler [n,3] f64, alpha [n] f64;  alpha_mode 0 = 'proj' (needs fx,cx),
 *   1 = 'trans'
 * A cuboid whose points span less than a plane (all 32 equal, say) has no
 * rotation: its euler x, y and its alpha come back NaN, the other instances
 * of the launch are not affected.
 * ---------------------------------------------------------------------- */
int egn_pose_solve_f64(const double* pred3d, int n, const double* kpt_x,
                       double fx, double cx, int alpha_mode,
                       double* euler, double* alpha, void* stream);
/* Host twins of egn_keypoints_to_screen_f64 (without the lifter-input part) and
 * egn_pose_solve_f64: the same arithmetic as plain loops over HOST pointers, no
 * stream.  They serve the reference's CPU plumbing -- EgoNet.get_keypoints(
 * is_cuda=False), get_6d_rep on a CPU model (egonet.py:424-467, 279-295;
 * BASELINE config 1) -- and are never used for CUDA tensors. */
int egn_keypoints_to_screen_host_f64(const float* local, int n, int K,
                                     double mul_x, double mul_y,
                                     const double* center, const double* scale,
                                     int crop_w, int crop_h, double* screen);
int egn_pose_solve_host_f64(const double* pred3d, int n, const double* kpt_x,
                            double fx, double cx, int alpha_mode,
                            double* euler, double* alpha);

/* ------------------------------------------------------------------------
 * KITTI 2D-detection AP + Average Orientation Similarity, the IMAGE-metric path
 * of tools/kitti-eval/evaluate_object_3d_offline.cpp (:131-265, :346-706,
 * :791-850) without Boost.  Host code, no GPU.  Reads gt_dir/%06d.txt and
 * result_dir/data/%06d.txt (KITTI label / result lines).
 *   evaluated [3]       1 if class (car, pedestrian, cyclist) has detections
 *   aos_valid           0 if any detection carries alpha == -10
 *   precision, aos      [3 classes][3 levels easy/moderate/hard][41 recall samples]
 * Returns 0; -1 bad argument; -2 missing ground-truth file; -3 no result files.
 * ---------------------------------------------------------------------- */
int egn_kitti_eval_image(const char* gt_dir, const char* result_dir, int* n_frames,
                         int* evaluated, int* aos_valid, double* precision,
                         double* aos);

/* ------------------------------------------------------------------------
 * The whole KITTI object evaluator: IMAGE (2D AP + AOS), GROUND (bird's-eye-view AP) and BOX3D (3D AP), the three
 * blocks of evaluate_object_3d_offline.cpp:853-911, without Boost.  Per-pair math in csrc/kitti_overlap_math.h, the
 * matching loop in csrc/kitti_eval_core.h (one function for host and device), the host path in csrc/kitti_eval.cpp,
 * the device path in csrc/kitti_eval.hip.
 *
 * A box is 12 doubles: x1 y1 x2 y2 alpha h w l t1 t2 t3 ry.  Type codes: 0 car, 1 pedestrian, 2 cyclist, 3 van,
 * 4 person_sitting, 5 dontcare, 6 anything else.  metrics: bit 0 IMAGE, bit 1 GROUND, bit 2 BOX3D.
 *   evaluated    [3 metrics][3 classes]: the class is scored in the metric (a detection of it has x1 >= 0 /
 *                t1 != -1000 / t2 != -1000) and the metric was asked for
 *   aos_valid    0 if any detection carries alpha == -10
 *   precision    [3 metrics][3 classes][3 levels][41 recall samples]
 *   aos          [3 classes][3 levels][41], IMAGE only
 *   counts       [3 metrics][3 classes][3 levels][41][3]: tp, fp, fn at each score threshold; may be NULL
 *   n_thresholds [3 metrics][3 classes][3 levels]: recall steps reached; may be NULL
 * Rows of combinations that are not scored stay 0.
 *
 * egn_kitti_eval_dirs_host / _dev read gt_dir/%06d.txt and result_dir/data/%06d.txt like egn_kitti_eval_image (same
 * return codes).  egn_kitti_eval_packed_host / _dev take the frames as arrays: frame f owns ground truths
 * gt_off[f] .. gt_off[f + 1] and detections det_off[f] .. det_off[f + 1]; all pointers are HOST pointers.  Offsets
 * that do not start at 0 or decrease, a type code outside the table, more than 2^27 - 1 rows: -1.
 *
 * The _dev entries run on the current device: one packed copy up, four launches on `stream` (overlap table of all
 * (detection, ground truth) pairs; recall pass, one thread per (frame, metric, class, level); precision pass, one
 * wavefront per (frame, metric, class, level) with lane = score threshold; fixed-order fold of the similarity), two
 * synchronisations (the true-positive scores come back once for getThresholds), independent of the number of frames.
 * No capacity per frame.  Integer totals and a fixed-order similarity sum: equal inputs give equal bits, and the
 * results equal the _host entries'.  The workspace is allocated and freed inside the call (hipMalloc / hipFree).
 * Every launch is added to the launch counter; the _host entries launch nothing.
 *
 * egn_kitti_overlap_host_f64 / _dev_f64: pair k is det_box[k] against gt_box[k]; criterion -1 over the union, 0 over
 * the detection, 1 over the ground truth; out [n][4] = image overlap, ground overlap, 3D overlap, bird's-eye-view
 * intersection area.  _dev takes device pointers and is one launch on `stream`.
 * ---------------------------------------------------------------------- */
int egn_kitti_eval_dirs_host(const char* gt_dir, const char* result_dir, int metrics, int* n_frames, int* evaluated,
                             int* aos_valid, double* precision, double* aos, int* counts, int* n_thresholds);
int egn_kitti_eval_dirs_dev(const char* gt_dir, const char* result_dir, int metrics, int* n_frames, int* evaluated,
                            int* aos_valid, double* precision, double* aos, int* counts, int* n_thresholds,
                            void* stream);
int egn_kitti_eval_packed_host(int n_frames, const int* gt_off, const int* det_off, const double* gt_box,
                               const int* gt_type, const double* gt_trunc, const int* gt_occ, const double* det_box,
                               const int* det_type, const double* det_score, int metrics, int* evaluated,
                               int* aos_valid, double* precision, double* aos, int* counts, int* n_thresholds);
int egn_kitti_eval_packed_dev(int n_frames, const int* gt_off, const int* det_off, const double* gt_box,
                              const int* gt_type, const double* gt_trunc, const int* gt_occ, const double* det_box,
                              const int* det_type, const double* det_score, int metrics, int* evaluated,
                              int* aos_valid, double* precision, double* aos, int* counts, int* n_thresholds,
                              void* stream);
int egn_kitti_overlap_host_f64(const double* det_box, const double* gt_box, long n, int criterion, double* out);
int egn_kitti_overlap_dev_f64(const double* det_box, const double* gt_box, long n, int criterion, double* out,
                              void* stream);

/* ------------------------------------------------------------------------
 * Crop front end: all boxes of one image in one launch (egonet.py:68-96:
 * get_affine_transform + cv2.warpAffine(INTER_LINEAR, border 0) + ToTensor +
 * Normalize).  img [H,W,3] uint8 RGB (row pitch in bytes); M [n,6] f64 forward
 * 2x3 affines image -> crop; out [n,3,out_h,out_w] f32 = (bilinear/255 - mean)/std.
 * Restates cv::warpAffine's 8-bit fixed-point scheme (1/32 pixel); OpenCV is
 * absent from the build image: parity with cv2 is unpinned.
 * ---------------------------------------------------------------------- */
int egn_crop_warp_normalize_u8(const uint8_t* img, int H, int W, int pitch,
                               const double* M, int n, int out_h, int out_w,
                               const float* mean, const float* stdv, float* out,
                               void* stream);
/* The same warp + ToTensor + Normalize for the boxes of MANY frames in one launch
 * (training-sample front end, car_instance.py:1272-1299 -> img_proc.py:213-345).
 *   frames     all frames packed in one buffer, each [H,W,3] uint8 RGB
 *   frame_tab  [n_frames][4] int64: byte offset into `frames`, H, W, row pitch (bytes)
 *   box_frame  [n] int32 frame index of each box (outside [0, n_frames): border only)
 *   M          [n,6] f64 forward affines image -> crop; out [n,3,out_h,out_w] f32
 * Per-pixel semantics are exactly those of egn_crop_warp_normalize_u8.  n <= 65535, out_w <= 4096.
 * The launch is added to the launch counter. */
int egn_crop_frames_warp_normalize_u8(const uint8_t* frames, const long long* frame_tab,
                                      int n_frames, const int* box_frame, const double* M,
                                      int n, int out_h, int out_w, const float* mean,
                                      const float* stdv, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Training step building blocks (reference: libs/trainer/trainer.py:183-209
 * zero_grad / forward / loss / backward / optim.step; FCmodel.py Linear +
 * BatchNorm1d (batch statistics) + ReLU + Dropout; function.py:204-215
 * MSELoss1D; optimizer.py:8-40 Adam).  The GEMMs of forward / dgrad / wgrad run
 * on egn_conv2d_f32 (a Linear is a 1x1 conv); matrices are row-major
 * [rows, ld] fp32 with ld % 4 == 0.
 * ---------------------------------------------------------------------- */
/* Weight gradient of a conv / Linear layer (autograd's backward of nn.Conv2d /
 * nn.Linear in trainer.py:194 `loss.backward()`):
 *   dw[co][ci][ky][kx] = sum_{n,oy,ox} dy[n,oy,ox,co] * x[n,oy*s+ky-p,ox*s+kx-p,ci]
 * x [N,H,W,cs_in], dy [N,Ho,Wo,cs_out] NHWC fp32 (pad channels zero), dw in
 * torch's [Cout][Cin][KH][KW] layout.  Split-K over pixel tiles with a
 * deterministic two-pass reduction; ws = scratch of egn_conv2d_wgrad_ws_bytes().
 * KH*KW in {1, 9, 16}.  A Linear is N = rows, H = W = 1.
 * 3x3 / stride 1 / pad 1 layers with Cin % 48 == 0, Cout % 48 == 0 and unpadded
 * channel strides run in Winograd F(2x2,3x3) form (csrc/conv_wgrad_wino.hip: same
 * result to fp32 rounding -- error vs float64 4e-7 of the largest tap, the direct
 * kernel's 3e-7 -- not bit-identical; the environment switch EGN_WGRAD_WINO=0
 * keeps the direct kernel).  Either way two launches give the same bits. */
long egn_conv2d_wgrad_ws_bytes(int N, int H, int W, int Cin, int cs_in, int Cout,
                               int cs_out, int KH, int KW, int stride, int pad);
int egn_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, int N, int H,
                         int W, int Cin, int cs_in, int Cout, int cs_out, int KH,
                         int KW, int stride, int pad, void* ws, long ws_bytes,
                         void* stream);
/* Host-only introspection of the weight-gradient planner (no GPU needed, like
 * egn_conv_plan_query).  egn_conv2d_wgrad_num_variants(): rows of the dispatch
 * table = kernels egn_conv2d_wgrad_f32 can launch.  The query returns non-zero
 * exactly where egn_conv2d_wgrad_ws_bytes() returns < 0, else fills
 * out[0..15] = table row, form (0 direct, 1 Winograd 8 x 16 tiles, 2 Winograd
 *              8 x 8 tiles of image pairs), TH, TW, TNB, co_tiles, ci_tiles,
 *              ntiles, tiles_per_split, nsplit, reduce lanes (2, 8 or 32),
 *              slab order (0 dense [tap][CoP][CiP], 1 MFMA-fragment order),
 *              lds_bytes, and how often the tile-shrinking loop halved TNB,
 *              TH, TW. */
int egn_conv2d_wgrad_num_variants(void);
int egn_conv2d_wgrad_plan_query(int N, int H, int W, int Cin, int cs_in, int Cout,
                                int cs_out, int KH, int KW, int stride, int pad,
                                int* out);
/* conv weights [nchunk][1][4][CoutP][4] from a row-major matrix:
 * transpose 0: W[co][ci] = src[co*ld+ci]; 1: W[co][ci] = src[ci*ld+co].
 * A NULL src / dst, cout / cin <= 0 or ld below the row length (cin; transposed: cout): EGN_E_BADARG. */
int egn_pack_matrix_f32(const float* src, int ld, int cout, int cin,
                        int transpose, float* dst, void* stream);
/* Dense fp32 GEMM on the matrix pipe (csrc/gemm.hip) for the lifter's nn.Linear layers -- reference
 * libs/model/FCmodel.py:33-43, 92-105 (forward) and what torch autograd derives from them in
 * libs/trainer/trainer.py:191-197 (data / weight gradients); operands are read as they lie, nothing is packed:
 *   form 0 "NT"  C[M][N] = A[M][K] . B[N][K]^T (+ bias[N])     z  = a W^T + b
 *   form 1 "NN"  C[M][N] = A[M][K] . B[K][N]                   da = dz W
 *   form 2 "TN"  C[M][N] = A[K][M]^T . B[K][N]                 dW = dz^T a   (split along K, fixed-order reduction;
 *                                                              `ws` of egn_gemm_ws_bytes bytes)
 * Row-major with leading dimensions lda / ldb / ldc (floats, multiples of 4).  egn_gemm_supported() = 1 for the
 * shapes the kernels take (M, N multiples of 128, K of 32); the callers keep the conv-kernel route for the rest.
 * It answers 0 for a leading dimension smaller than the row it strides (form 0: lda >= K, ldb >= K; form 1: lda >= K,
 * ldb >= N; form 2: lda >= M, ldb >= N; always ldc >= N -- zero and negative values among them: such rows would fold
 * onto each other) and for an A or B of 0xF0000000 bytes or more (rows x leading dimension x 4: the range of the
 * kernels' 32-bit buffer offsets).  The query and the launch agree: egn_gemm_f32 / egn_gemm_ex_f32 return
 * EGN_E_BADARG exactly where the query says 0, or for a NULL A / B / C, a bias with form 2, an addend outside form 1,
 * stats outside form 0 or with too few rows, or a missing / short `ws` where egn_gemm_ws_bytes is not 0.
 * variant 0 = default tile configuration of the form (others: tools/gemm_probe.py). */
int egn_gemm_supported(int form, int M, int N, int K, int lda, int ldb, int ldc);
long egn_gemm_ws_bytes(int form, int M, int N, int K);
int egn_gemm_f32(int form, const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                 int lda, int ldb, int ldc, int variant, void* ws, long ws_bytes, void* stream);
/* The same with the epilogue fusions of the lifter's training step (FCmodel.py:33-43 under trainer.py:183-209):
 *   addend (form 1 only, [M][ldc]): C = A.B + addend -- the skip-path gradient of a residual block (FCmodel.py:49-51,
 *           `out = x + y`) joins the branch gradient without an add pass;
 *   stats  (form 0 only): partial column sums and sums of squares of the stored C, [stats_rows][2][N]
 *           doubles with stats_rows >= egn_gemm_stats_rows(M) (one row per 128-row block tile, fixed summation order)
 *           -- nn.BatchNorm1d's batch statistics without a pass over z; egn_bn_stats_finalize_f32 adds the rows. */
long egn_gemm_stats_rows(int M);
int egn_gemm_ex_f32(int form, const float* A, const float* B, float* C, const float* bias, const float* addend,
                    double* stats, long stats_rows, int M, int N, int K, int lda, int ldb, int ldc, int variant,
                    void* ws, long ws_bytes, void* stream);
/* dst[c][r] = src[r][c]; dst columns R..ld_dst-1 are zeroed */
int egn_transpose_f32(const float* src, int R, int C, int ld_src, float* dst,
                      int ld_dst, void* stream);
/* scratch bytes the column reductions below need for `cols` columns */
long egn_colreduce_ws_bytes(int cols);
int egn_colsum_f32(const float* a, int rows, int cols, int ld, float* sum,
                   void* ws, void* stream);
/* per-column batch statistics of z [rows, ld] (NHWC conv output: rows = N*H*W,
 * ld = cs): mean, 1/sqrt(biased var + eps), unbiased var; when running_mean /
 * running_var are given they are updated in place with torch's rule
 * running = (1-momentum)*running + momentum*batch (unbiased var) */
int egn_bn_stats_f32(const float* z, int rows, int cols, int ld, float eps,
                     float* mean, float* invstd, float* var_unbiased,
                     float* running_mean, float* running_var, float momentum,
                     void* ws, void* stream);
/* BatchNorm batch statistics WITHOUT a second pass over the conv output: the raw convolution
 * (scale = ones, shift = zeros, no residual / activation; `wpack` as egn_conv_config_kind(cfg) says)
 * whose epilogue also writes, per (tile, wave), the column sums and sums of squares of what it stores:
 * partials [rows][2][Cout] doubles, rows = egn_conv2d_bnstats_rows(...) (0 = this tile configuration
 * has no fused statistics: use egn_conv2d_f32 + egn_bn_stats_f32).  egn_bn_stats_finalize_f32 adds
 * the rows in a fixed order (deterministic) and produces what egn_bn_stats_f32 produces
 * (`rows` there = N*Ho*Wo, the number of samples per channel). */
long egn_conv2d_bnstats_rows(int N, int H, int W, int Cin, int cs_in, int Cout,
                             int cs_out, int KH, int KW, int stride, int pad, int cfg);
int egn_conv2d_bnstats_f32(const float* x, const float* wpack, const float* ones,
                           const float* zeros, float* y, int N, int H, int W,
                           int Cin, int cs_in, int Cout, int cs_out, int KH, int KW,
                           int stride, int pad, int cfg, double* partials,
                           long partial_rows, void* stream);
/* [round 5] The 1x1 convolutions around layer1's 256-channel tensor as ONE streaming launch (csrc/conv_pw.hip).
 * Replaces, for a Bottleneck of libs/model/heatmapModel/hrnet.py:95-133 and the first line of the next one,
 *     out = relu(bn3(conv3(h)) + residual)    (1x1, 64 -> 256)    and    hn = relu(bn1(conv1(out)))    (1x1, 256 -> 64):
 *     out[M][256] = act1(h[M][64] . w3^T + shift3 (+ res[M][256])),    hn[M][64] = relu(out . w1^T + shift1)
 * with the block's tile of `out` kept in LDS between the two products (the 256-channel tensor crosses HBM once per
 * direction).  w3 [256][64] / w1 [64][256]: the 1x1 filters as torch holds them ([Cout][Cin], row-major) with the
 * folded BatchNorm scale multiplied in per output channel; shift: the folded shift.  act1 = ReLU if relu1 else none.
 * w1 = shift1 = hn = NULL: the first product alone (the downsample conv, the last block's conv3).
 * M = N*H*W pixels, M % 32 == 0; NHWC rows without padding; res != out, h != hn. */
int egn_pw_pair_f32(const float* h, const float* res, const float* w3, const float* shift3,
                    const float* w1, const float* shift1, float* out, float* hn, int M,
                    int relu1, void* stream);
/* [round 5] egn_conv2d_f32 with the two optional side tables of the native training tape
 * (replaces the MIOpen convolutions under libs/trainer/trainer.py:191-197 for the 3x3 s1 layers of
 * libs/model/heatmapModel/hrnet.py:63-92 on the F(4x4,3x3) kernels):
 *   partials / partial_rows  BatchNorm partial statistics of the stored output, as egn_conv2d_bnstats_f32
 *                            (NULL = none; else egn_conv2d_bnstats_rows(cfg) rows are written);
 *   tickets / ticket_words   zeroed `unsigned` words for the K-split configurations (cfg 83 / 84):
 *                            egn_conv2d_ticket_words(...) of them (0 = the configuration uses none).  With
 *                            them the layer is ONE kernel launch, as inside a program, and leaves the words
 *                            zero; launches that share the words must be ordered (one stream).  NULL = the
 *                            three-launch form of egn_conv2d_f32. */
long egn_conv2d_ticket_words(int N, int H, int W, int Cin, int cs_in, int Cout,
                             int cs_out, int KH, int KW, int stride, int pad, int cfg);
int egn_conv2d_ex_f32(const float* x, const float* wpack, const float* scale,
                      const float* shift, const float* res, float* y, int N, int H,
                      int W, int Cin, int cs_in, int Cout, int cs_out, int KH, int KW,
                      int stride, int pad, int act, int cfg, double* partials,
                      long partial_rows, unsigned* tickets, long ticket_words,
                      void* stream);
int egn_bn_stats_finalize_f32(const double* partials, long nrows, int rows, int cols,
                              float eps, float* mean, float* invstd,
                              float* var_unbiased, float* running_mean,
                              float* running_var, float momentum, void* stream);
/* relu: 0 none, 1 nn.ReLU, 2 nn.LeakyReLU() (slope 0.01, FCmodel.py:19-22) -- here and in the two
 * backward entry points below.  The forward entry points also take relu | EGN_ACT_RES_AFTER (0x11, 0x12):
 * y = res + dropout(act(bn(z))) instead of act(bn(z) + res).  The backward entry points (and their _drop forms) take
 * 0, 1 and 2 only and refuse anything else with EGN_E_BADARG: the residual-after form puts no gate on res (its
 * gradient is dy itself), so its backward is the plain flag without res.
 * y = relu?(gamma*(z-mean)*invstd + beta + res?) * (mask ? mask*keep_scale : 1)
 * (BatchNorm on batch statistics + residual + ReLU + inverted dropout) */
int egn_bn_act_fwd_f32(const float* z, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, const float* mask,
                       float keep_scale, int relu, const float* res, float* y,
                       int rows, int cols, int ld, void* stream);
/* BatchNorm backward, step 1: dbeta = sum dpre, dgamma = sum dpre*xhat with
 * dpre = dy * dropout-mask * relu-gate(gamma*xhat + beta + res > 0) */
int egn_bn_bwd_sums_f32(const float* dy, const float* z, const float* mask,
                        float keep_scale, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, int relu,
                        const float* res, int rows, int cols, int ld,
                        float* dbeta, float* dgamma, void* ws, void* stream);
/* step 2: dz = gamma*invstd*(dpre - dbeta/rows - xhat*dgamma/rows); dres
 * (optional) = dpre, the gradient that flows into the residual branch */
int egn_bn_bwd_dz_f32(const float* dy, const float* z, const float* mask,
                      float keep_scale, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, int relu,
                      const float* res, const float* dbeta, const float* dgamma,
                      float* dz, float* dres, int rows, int cols, int ld,
                      void* stream);
/* The same three with the inverted-dropout keep mask DRAWN IN THE KERNEL (nn.Dropout(p) after every ReLU of the
 * lifter, libs/model/FCmodel.py:24, 38-41): Philox4x32-10 keyed by `seed`, counter = (float4 group index of the
 * element, `layer`, *step_dev); element kept <=> its 32-bit draw >= p * 2^32; kept values are scaled by 1/(1-p).
 * Forward and backward regenerate the same mask from the same (seed, layer, *step_dev): no mask tensor, no RNG
 * kernel inside a training step; *step_dev is read on the device (the optimizer's step counter: hipGraph-safe).
 * egn_dropout_mask_f32 writes the mask those kernels use (tests). */
int egn_bn_act_fwd_drop_f32(const float* z, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float p, unsigned long long seed, const int* step_dev, int layer,
                            int relu, const float* res, float* y, int rows, int cols, int ld, void* stream);
int egn_bn_bwd_sums_drop_f32(const float* dy, const float* z, float p, unsigned long long seed, const int* step_dev,
                             int layer, const float* mean, const float* invstd, const float* gamma,
                             const float* beta, int relu, const float* res, int rows, int cols, int ld,
                             float* dbeta, float* dgamma, void* ws, void* stream);
int egn_bn_bwd_dz_drop_f32(const float* dy, const float* z, float p, unsigned long long seed, const int* step_dev,
                           int layer, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           int relu, const float* res, const float* dbeta, const float* dgamma, float* dz,
                           float* dres, int rows, int cols, int ld, void* stream);
int egn_dropout_mask_f32(float* mask, long n, float p, unsigned long long seed, const int* step_dev, int layer,
                         void* stream);
/* BatchNorm in EVAL mode inside a model that trains (nn.BatchNorm2d.forward with training == False under
 * trainer.py:183-209: a frozen layer of a fine-tune normalises with running_mean / running_var and writes nothing).
 * egn_bn_fold_batch_f32: ONE launch folds every such layer of a model from a device table of `n` descriptors of
 * egn_bn_fold_desc_bytes() bytes each, in this order, naturally aligned:
 *     const float *gamma, *beta, *mean, *var, *bias;  float *scale, *shift;  double eps;  int cout, coutp;
 *   scale[c] = gamma[c] / sqrt(var[c] + eps)              (gamma NULL: 1 / sqrt(var[c] + eps), the layer's 1/sigma)
 *   shift[c] = beta[c] + (bias[c] - mean[c]) * scale[c]   (bias NULL: no conv bias; shift NULL: not written)
 * computed in double and rounded once; entries cout..coutp-1 of both vectors are written as zeros.  scale / shift are
 * what egn_conv2d_f32 / egn_conv2d_ex_f32 take: y = act(conv(x) * scale + shift (+ res)) is the layer's forward. */
int egn_bn_fold_desc_bytes(void);
int egn_bn_fold_batch_f32(const void* descs_dev, int n, void* stream);
/* ... and its backward in one pass over [rows][ld] (no reduction: the statistics are constants):
 *   dpre = dy * [y > 0] (relu = 1; relu = 0: dy, y may be NULL),  dz = dpre * scale[c],  dres (optional) = dpre
 * y is the layer's OUTPUT (relu(pre) > 0 <=> pre > 0: torch's gate), so neither the conv output nor the residual is
 * read.  Columns cols..ld-1 of dz / dres are written as zeros whatever dy holds there.  ld % 4 == 0. */
int egn_bn_frozen_bwd_f32(const float* dy, const float* y, const float* scale, int relu, float* dz, float* dres,
                          int rows, int cols, int ld, void* stream);
int egn_add_f32(const float* a, const float* b, float* y, long n, void* stream);
/* *loss += weight*mean((pred-tgt)^2) (zero it first);
 * dpred (= or, with accumulate, +=) weight*2(pred-tgt)/(rows*cols).
 * weight 0.5 over all joints = the heat-map term of JointsCompositeLoss
 * (function.py:95-111), weight 1 = MSELoss1D (function.py:204-215) */
int egn_mse_f32(const float* pred, const float* tgt, int rows, int cols,
                int ld_pred, int ld_tgt, float weight, int accumulate,
                float* dpred, double* loss, void* stream);
/* The three criteria of the reference's loss_dict (libs/loss/function.py:17-20)
 * over a [rows, cols] view with row pitches; crit 0 = nn.MSELoss, 1 = nn.L1Loss,
 * 2 = nn.SmoothL1Loss (beta 1), reduction 'mean':
 *   *loss += weight * mean(c(pred - tgt)) (zero it first);
 *   dpred (= or, with accumulate, +=) weight * c'(pred - tgt) / (rows*cols).
 * Heat-map term L_hm (function.py:95-111): weight 0.5 * w_hm over all joints;
 * coordinate term L_2d (:155-168): rows 1, cols N*K*2. */
int egn_elem_loss_f32(const float* pred, const float* tgt, int rows, int cols,
                      int ld_pred, int ld_tgt, int crit, float weight,
                      int accumulate, float* dpred, double* loss, void* stream);
/* The heat-map criterion on pixel-shuffled maps (hrnet.py:373-383, 598-600 +
 * JointsMSELoss / loss_dict, function.py:17-46) without materialising the shuffled
 * prediction: x = the pre-shuffle NHWC activations [N,H,W,cs] (channel j*up*up+a*up+b),
 * tgt = the NCHW target [N,C,H*up,W*up], tw = per-(n, j) weights [N,C] or NULL
 * (use_target_weight); crit as egn_elem_loss_f32.
 *   *loss += weight * mean(c(pred*w - tgt*w)) (zero it first);
 *   dx = weight * c'(pred*w - tgt*w) * w / (N*C*H*up*W*up) in the pre-shuffle layout
 *   (pad channels zero; dx may be NULL).  x, dx 16-byte aligned, cs % 4 == 0, else
 *   EGN_E_BADARG; tgt at any 4-byte alignment (16 bytes: the vectorised path). */
int egn_pixshuf_loss_f32(const float* x, const float* tgt, const float* tw, int N, int H,
                         int W, int C, int up, int cs, int crit, float weight, float* dx,
                         double* loss, void* stream);
/* AvgPool2d(k) (stride k, no padding, floor) over NHWC: x [N,H,W,cs] -> y [N,H/k,W/k,cs],
 * the k*k taps summed, then / (k*k) (the angle head's AvgPool2d(4), hrnet.py:384-422).
 * Both pools: a NULL or not 16-byte aligned operand, H or W < k, cs < 4 or cs % 4: EGN_E_BADARG. */
int egn_avgpool_fwd_f32(const float* x, float* y, int N, int H, int W, int cs, int k,
                        void* stream);
/* its backward: dx [N,H,W,cs] (= or, with accumulate, +=) dy[n, y/k, x/k, c] / (k*k);
 * positions outside every window get 0 */
int egn_avgpool_bwd_f32(const float* dy, float* dx, int N, int H, int W, int cs, int k,
                        int accumulate, void* stream);
/* *loss += weight*mean(|pred-tgt|); dpred = weight*sign(pred-tgt)/n
 * (nn.L1Loss, the coordinate term, function.py:155-168) */
int egn_l1_f32(const float* pred, const float* tgt, long n, float weight,
               float* dpred, double* loss, void* stream);
/* cross-ratio term L_cr (function.py:113-153 calc_cross_ratio_loss + get_cr_mask,
 * img_proc.py:709-720 appro_cr): coords [N,K,2] f32, idx [L,4] int32 device
 * array of joint indices (A,B,C,D) per line (car_instance.py:83-97 'bbox12');
 * cr = |AC|^2|BD|^2 / (|BC|^2|AD|^2) / target_cr^2; a line counts when the
 * smallest non-zero distance among its four points > thres;
 * *loss += weight * sum(crit(cr,1)) / #lines kept; dcoords (may be NULL)
 * += the gradient.  crit: 0 mse, 1 l1, 2 smooth-l1.  ws: egn_cross_ratio_ws_bytes.
 * A kept line with A == C or B == D has cr = 0 and gradient 0 for its four points (the
 * reference's autograd: d|AC|^2/dA = 0); with B == C or A == D cr is infinite, as in the
 * reference, and so are the loss and the gradient of that line's points.  No line kept:
 * *loss and dcoords keep their bits.  idx must hold joint indices in 0..K-1 (device memory:
 * the entry point cannot check them). */
long egn_cross_ratio_ws_bytes(int N, int L);
int egn_cross_ratio_f32(const float* coords, int N, int K, const int* idx,
                        int L, double target_cr, float thres, int crit,
                        float weight, float* dcoords, double* loss, float* ws,
                        void* stream);
/* Differentiable soft-arg-max of heat-maps (JointsCompositeLoss on a model that returns
 * heat-maps only, function.py:187-201; soft_arg_max, img_proc.py:678-707) on the padded NHWC
 * maps z [N,h,w,cs] f32, channels 0..K-1 live (csrc/softargmax.hip, softargmax_math.h).
 * Forward, per map: m = max z, e_p = exp(z_p - m), ex = sum e_p x_p / sum e_p (x_p, y_p the
 * integer column / row), ey alike; coords [N,K,2] = (ex / div_x, ey / div_y);
 * save [N,K,4] = (ex, ey, m, sum e) for the backward.  fp32 sums in the fixed order the header
 * documents: equal inputs give equal bits.  Logits of any finite size give finite results.
 * Backward: dz [N,h,w,cs] (= or, with accumulate, +=) s_p ((x_p - ex) gx / div_x +
 * (y_p - ey) gy / div_y) with s_p = e_p / sum e recomputed from z and save, (gx, gy) =
 * dcoords [N,K,2]; channels K..cs-1 and the images n_rows..N-1 are neither read nor written.
 * One launch each, counted by egn_launch_count().  The _host_ twins take host pointers and
 * return the same bits.  EGN_E_BADARG: a NULL operand or one not aligned (z, dz, save: 16 bytes;
 * coords, dcoords: 8), N < 1, K < 1, K > cs, cs % 4, h or w < 1, div_x or div_y not > 0,
 * n_rows outside 0..N (device: n_rows > 65535). */
int egn_softargmax_fwd_f32(const float* z, int N, int h, int w, int K, int cs, float div_x,
                           float div_y, float* coords, float* save, void* stream);
int egn_softargmax_bwd_f32(const float* z, const float* save, const float* dcoords, int N,
                           int n_rows, int h, int w, int K, int cs, float div_x, float div_y,
                           int accumulate, float* dz, void* stream);
int egn_softargmax_fwd_host_f32(const float* z, int N, int h, int w, int K, int cs, float div_x,
                                float div_y, float* coords, float* save);
int egn_softargmax_bwd_host_f32(const float* z, const float* save, const float* dcoords, int N,
                                int n_rows, int h, int w, int K, int cs, float div_x,
                                float div_y, int accumulate, float* dz);
/* dz = dy*y*(1-y): backward of the coordinate head's Sigmoid (hrnet.py:461-466) */
int egn_sigmoid_bwd_f32(const float* dy, const float* y, float* dz, long n,
                        void* stream);
/* torch conv weight [Cout][Cin][KH][KW] -> packed filter of egn_conv2d_f32, on
 * the device.  dgrad 0: the forward filter.  dgrad 1: the data-gradient
 * filter (in/out channels swapped, taps rotated by 180 degrees), so that
 *   dx = egn_conv2d_f32(dy [zero-inserted when stride 2], packed, Cin' = Cout,
 *                       Cout' = Cin, stride 1, pad K-1-pad)
 * egn_packed_weight_floats = number of floats dst must hold. */
long egn_packed_weight_floats(int Cout, int Cin, int KH, int KW, int dgrad);
int egn_pack_conv_weight_f32(const float* w, int Cout, int Cin, int KH, int KW,
                             int dgrad, float* dst, void* stream);
/* Every filter of a model packed in ONE launch (the weights only change in the
 * optimizer step; a W48 training step needs ~600 packs).  descs: DEVICE array of
 *   struct { const float* w; float* dst; int32 Cout, Cin, taps, dgrad; int64 begin; }
 * (egn_pack_desc_bytes() bytes each), `begin` = running sum of the work units of the
 * preceding descriptors: egn_packed_weight_floats()/4 (one float4 each) for the direct
 * layouts (dgrad 0 / 1), egn_wino_weight_floats()/64 for the Winograd layout
 * (dgrad | 2: taps must be 9; one unit = 4 input channels x 16 frequencies),
 * egn_wino4_pack_weight_floats()/48 for the F(4x4,3x3) layout of conv_wino4.hip
 * (dgrad | 4: taps must be 9; one unit = one (output, input) channel pair). */
int egn_pack_desc_bytes(void);
int egn_pack_conv_weights_batch_f32(const void* descs_dev, int n, long total_float4,
                                    void* stream);
/* up[n][2y][2x][:] = dy[n][y][x][:], zero elsewhere; up is [N,H,W,cs] */
int egn_zero_insert2_f32(const float* dy, float* up, int N, int Ho, int Wo,
                         int H, int W, int cs, void* stream);
/* backward of one term of egn_fuse_sum_relu_f32: g [N,H>>shift,W>>shift,cs] =
 * block sums of dy*(y>0) (y NULL: no gate) */
int egn_fuse_bwd_f32(const float* dy, const float* y, float* g, int N, int H,
                     int W, int cs, int shift, void* stream);
/* Heat-map training targets for a whole batch (img_proc.py:347-409
 * generate_target): an un-normalised Gaussian dot of half-width 3*sigma centred
 * on cell int(joint/stride + 0.5) of every visible joint, clipped to the map.
 *   joints [N,K,3] f64 (x, y, unused) in input pixels; vis [N,K] f32 or NULL
 *   target [N,K,H,W] f32 out; weight [N,K] f32 out (vis, zeroed where the dot
 *   is completely out of bounds), may be NULL
 *   stride_x = input_size[0]/heatmap_size[0], stride_y = input_size[1]/heatmap_size[1]
 * The launch is added to the launch counter. */
int egn_gaussian_targets_f32(const double* joints, const float* vis, int N, int K,
                             int H, int W, double stride_x, double stride_y,
                             double sigma, float* target, float* weight,
                             void* stream);
/* running = (1-momentum)*running + momentum*batch */
int egn_ema_f32(float* running, const float* batch, float momentum, int n,
                void* stream);
/* torch.optim.Adam (weight_decay 0, no amsgrad), step counted from 1 */
int egn_adam_step_f32(float* p, const float* g, float* m, float* v, long n,
                      float lr, float beta1, float beta2, float eps, int step,
                      void* stream);

/* the same update with the step counter (step_dev[0], incremented by the call)
 * and the learning rate (lr_dev[0]) in device memory: nothing of the iteration
 * is baked into kernel arguments, so a hipGraph captured around a whole
 * training step replays correctly */
/* [round 6] start-of-step bookkeeping in one launch: *counters[k] += 1 for the n BatchNorm num_batches_tracked words
 * (int64; `counters` = device array of their addresses) and *zero_f64 = 0 (the loss accumulator; may be NULL).
 * Replaces torch's own increment of BatchNorm.num_batches_tracked in train-mode forwards (FCmodel.py:24-43, hrnet.py:63-92). */
int egn_step_counters_i64(long long* const* counters, int n, double* zero_f64, void* stream);
int egn_adam_step_dev_f32(float* p, const float* g, float* m, float* v, long n,
                          const float* lr_dev, float beta1, float beta2,
                          float eps, int* step_dev, void* stream);
/* torch.optim.Adam(weight_decay) -- coupled L2: g += weight_decay * p before the
 * moments (libs/optimizer/optimizer.py:19-21); state as egn_adam_step_dev_f32 */
int egn_adam_l2_step_dev_f32(float* p, const float* g, float* m, float* v,
                             long n, const float* lr_dev, float beta1,
                             float beta2, float eps, float weight_decay,
                             int* step_dev, void* stream);
/* torch.optim.SGD(momentum, weight_decay), dampening 0, no Nesterov
 * (libs/optimizer/optimizer.py:23-26): g' = g + wd p; buf = g' on the first step,
 * momentum*buf + g' after; p -= lr*buf.  buf may be NULL when momentum == 0.
 * step_dev[0] is incremented first (first step <=> it becomes 1). */
int egn_sgd_step_dev_f32(float* p, const float* g, float* buf, long n,
                         const float* lr_dev, float momentum, float weight_decay,
                         int* step_dev, void* stream);

/* ------------------------------------------------------------------------
 * The optimizer step for parameter groups (csrc/optim.hip): torch.optim.Adam / AdamW / SGD with any number of
 * param_groups, AMSGrad, Nesterov, dampening, and torch.nn.utils.clip_grad_norm_ (norm_type 2) folded into the
 * update.  The three entry points above are untouched and remain the path of everything they can express.
 *
 * A group is a row of 8 words (egn_optim_group); a work item is (begin, length, group) in floats of the flat buffer
 * (egn_optim_item): begin and length are multiples of 4, 0 < length <= egn_optim_item_floats(), and the items in
 * table order cover [0, n) exactly once (item k + 1 begins where item k ends).  An item never crosses the boundary
 * between two groups' segments; a parameter's padding belongs to the parameter.  Both tables exist twice: the host
 * copy is validated before anything is launched, the device copy is what the kernel reads -- the learning rates are
 * rewritten there by the scheduler, so a captured step replays with the current ones.
 *
 * family 0 (Adam):   g' = coef g + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;
 *                    p -= lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
 * family 1 (AdamW):  p *= 1 - lr wd first, then family 0 with wd = 0
 *   EGN_OPTIM_AMSGRAD in a group's flags: vmax' = max(vmax, v') takes the place of v' in the denominator.
 * family 2 (SGD):    g' = coef g + wd p;  buf' = g' where the step counter becomes 1, else mu buf + (1 - dampening) g'
 *                    (m is buf, v is not read); p -= lr (EGN_OPTIM_NESTEROV ? g' + mu buf' : buf'); mu == 0: p -= lr g'.
 * t = step_dev[0] after its increment (a launch of its own, before the one update launch); the bias corrections are
 * computed in double from it on the device.  coef = clip[1] when clip is not NULL (egn_grad_norm_clip_f32), else 1.
 * g is only read: the caller's gradient keeps its unclipped values.  Both launches are added to egn_launch_count().
 *
 * EGN_E_BADARG, before anything is launched: a NULL or not 16-byte aligned p / g (m, v for Adam; m for SGD where a
 * group has momentum; vmax where a group has EGN_OPTIM_AMSGRAD), a NULL table or step_dev, a clip that is not 8-byte
 * aligned, n < 1 or n % 4, 1 <= ngroups <= EGN_OPTIM_MAX_GROUPS violated, an item outside the buffer, items that
 * overlap or leave a gap, a group index outside the table, beta outside [0, 1), eps <= 0, a negative or non-finite
 * lr / weight_decay / momentum, dampening outside [0, 1], Nesterov with momentum 0 or dampening != 0, a flag
 * that does not belong to the family. */
#define EGN_OPTIM_ADAM 0
#define EGN_OPTIM_ADAMW 1
#define EGN_OPTIM_SGD 2
#define EGN_OPTIM_AMSGRAD 1
#define EGN_OPTIM_NESTEROV 2
#define EGN_OPTIM_MAX_GROUPS 32
typedef struct egn_optim_group {
  float lr, weight_decay, beta1, beta2, eps, momentum, dampening;
  int flags;
} egn_optim_group;
typedef struct egn_optim_item {
  long long begin;
  int length, group;
} egn_optim_item;
int egn_optim_item_floats(void);
int egn_optim_grouped_step_f32(int family, float* p, const float* g, float* m, float* v, float* vmax, long n,
                               const egn_optim_group* groups_host, const egn_optim_group* groups_dev, int ngroups,
                               const egn_optim_item* items_host, const egn_optim_item* items_dev, long nitems,
                               const float* clip, int* step_dev, void* stream);
/* clip_grad_norm_(norm_type 2) without the pass that scales: clip[0] = total_norm = sqrt(sum g^2) and
 * clip[1] = coef = min(1, max_norm / (total_norm + 1e-6)), both on the device, for egn_optim_grouped_step_f32 to
 * multiply in as it loads g.  Two launches (added to egn_launch_count()): a fixed grid of per-block partial sums of
 * squares in double (ws: egn_grad_norm_ws_bytes() bytes), then one block that adds them in a fixed order -- equal
 * inputs give equal bits.  A non-finite norm gives what torch gives with error_if_nonfinite=False: coef NaN for a
 * NaN norm, 0 for an infinite one.  The sum runs over the whole flat buffer: padding words must be 0.
 * EGN_E_BADARG: a NULL or misaligned g (16 bytes) / ws / clip (8), n < 1 or n % 4, max_norm negative or NaN. */
long egn_grad_norm_ws_bytes(void);
int egn_grad_norm_clip_f32(const float* g, long n, float max_norm, double* ws, float* clip, void* stream);

/* ------------------------------------------------------------------------
 * Programs: a recorded sequence of the launches above with every pointer
 * expressed as (slot, byte offset).  Slots are bound to base addresses before
 * a run (slot 0 = activation arena, 1 = packed weights, 2.. = user tensors),
 * so one recording serves every forward of a model at a fixed batch shape.
 * ---------------------------------------------------------------------- */
typedef struct egn_program egn_program;
typedef struct { int32_t slot; int64_t off; } egn_ref;   /* slot < 0: NULL */

egn_program* egn_program_create(int nslots);
void egn_program_destroy(egn_program* p);
int egn_program_bind(egn_program* p, int slot, void* base);
int egn_program_num_ops(const egn_program* p);

int egn_program_add_conv2d(egn_program* p, egn_ref x, egn_ref wpack,
                           egn_ref scale, egn_ref shift, egn_ref res, egn_ref y,
                           int N, int H, int W, int Cin, int cs_in,
                           int Cout, int cs_out, int KH, int KW, int stride,
                           int pad, int act, int out_nchw, int cfg);
int egn_program_add_fuse(egn_program* p, egn_ref y, int N, int H, int W, int C,
                         int cs, int nterms, const egn_ref* terms,
                         const int* shifts, int relu);
int egn_program_add_nchw_to_nhwc(egn_program* p, egn_ref x, egn_ref y, int N,
                                 int C, int H, int W, int cs);
int egn_program_add_nhwc_to_nchw(egn_program* p, egn_ref x, egn_ref y, int N,
                                 int C, int H, int W, int cs);
int egn_program_add_pixel_shuffle(egn_program* p, egn_ref x, egn_ref y, int N,
                                  int C, int H, int W, int cs, int up);
int egn_program_add_ramps(egn_program* p, egn_ref y, int N, int H, int W,
                          int cs, int c0);
int egn_program_add_decode(egn_program* p, egn_ref hm, int N, int K, int H,
                           int W, int mode, egn_ref out_xy, egn_ref out_max,
                           egn_ref out_idx);
/* Concurrency: ops added between egn_program_fork and egn_program_join run on
 * the launch lane selected by egn_program_set_lane (0 = the caller's stream,
 * 1..3 = internal side streams that start at the fork point and are waited for
 * at the join).  Ops on different lanes of one region must be independent and
 * must not share scratch buffers.  HRNet: one lane per resolution branch
 * (hrnet.py:286-287) and per fuse output (hrnet.py:291-298). */
int egn_program_fork(egn_program* p);
int egn_program_join(egn_program* p);
int egn_program_set_lane(egn_program* p, int lane);
/* Point-to-point ordering between lanes, as attributes of the op added last (not an op of its own).  signal != 0: after
 * the op's launch an event is recorded on its lane.  waits[0..nwaits): indices (in egn_program_num_ops order) of EARLIER
 * ops that signal; the op's lane waits for their events before the launch (hipStreamWaitEvent).  Anything else -- the op
 * itself, a later index, an op that does not signal, a fork / join -- is EGN_E_BADARG, so waits cannot form a cycle.  The
 * events (timing disabled) belong to the program and are destroyed with it.  Fork / join keep their meaning: every side
 * lane is still joined at the region's end.  egn_program_run_timed is serial on one stream and ignores both fields.
 * Under egn_program_capture the dependencies are not recorded as graph edges: the first wait for a signal given since
 * the last join is lowered to a join of every lane followed by a fork, so a captured graph keeps the plain fork / join
 * shape (same results; the waits only order less than that in an eager run). */
int egn_program_set_deps(egn_program* p, int signal, const int* waits, int nwaits);
/* tag the most recently added op (shown by the profiler); copied */
int egn_program_tag(egn_program* p, const char* tag, double flops, double bytes);

/* launch every op in order on `stream` */
int egn_program_run(egn_program* p, void* stream);
/* same, bracketing every op with hipEvents; ms[i] = duration of op i.
 * Synchronises the stream before returning. */
int egn_program_run_timed(egn_program* p, void* stream, float* ms, int n_ms);
/* capture the op sequence into a hipGraph (bindings frozen) / replay it */
int egn_program_capture(egn_program* p, void* stream);
int egn_program_replay(egn_program* p, void* stream);
/* [round 6] Ticket words of the program's K-split convolution ops (conv_wino4.hip: word 0 of an op's buffer is the error
 * word a block raises when its bounded wait for its partner runs out; 1.. are the item pairs' words, zero between runs).
 * A raised error word fails the NEXT egn_program_run / _run_timed / _replay with EGN_E_STATE (the run that raised it
 * produced invalid output); all words are zeroed again by that call.  egn_program_ticket_ops: how many ops own words.
 * egn_program_poke_ticket: TEST HOOK -- stores `value` into word `word` of K-split op `op` (0-based among those ops),
 * synchronously; the reference has no counterpart (its layers are single torch calls: libs/model/heatmapModel/hrnet.py:63-92). */
int egn_program_ticket_ops(const egn_program* p);
int egn_program_poke_ticket(egn_program* p, int op, int word, unsigned value);
/* [round 5] layer1's 1x1 pair as one op (egn_pw_pair_f32 below); w1 / shift1 / hn with slot < 0: the first product alone */
int egn_program_add_pw_pair(egn_program* p, egn_ref h, egn_ref res, egn_ref w3, egn_ref shift3,
                            egn_ref w1, egn_ref shift1, egn_ref out, egn_ref hn, int M,
                            int relu1);
/* Two independent 3x3 / stride 1 / pad 1 convolutions (unpadded channel strides) as ONE launch and one op
 * (conv_wino4_pair_kernel, csrc/conv_wino4.hip): `a` on 16-divisible maps with Cout_a % 96 == 0 the way config 86 runs
 * it, `b` on 8 x 8 maps with Cout_b % 48 == 0 the way config 82 does -- both filters in the F(4x4,3x3) register-feed
 * layout (kind 3), both outputs bit-identical to the two single-convolution ops.  The two grids share the chip: the
 * coarse HRNet branches (hrnet.py:286-287: independent at every depth) have 128 + 128 such items at 64 crops.  res_a /
 * res_b may be NULL.  grid_cap: 0, or a TEST HOOK -- plan for this many compute units (makes the persistent item loops
 * iterate on small inputs).  egn_conv_pair_plan_query is host-only (no GPU needed): returns non-zero where
 * egn_program_add_conv2d_pair would refuse the shapes, else out[0..1] = the blocks of the launch that work on `a` / on
 * `b` when the chip has `cus` compute units; with_stats / with_tickets != 0: as if the caller also asked for BatchNorm
 * statistics / brought K-split ticket words (refused: the pair has neither). */
int egn_program_add_conv2d_pair(egn_program* p, egn_ref xa, egn_ref wa, egn_ref scale_a, egn_ref shift_a,
                                egn_ref res_a, egn_ref ya, int Na, int Ha, int Wa, int Cin_a, int Cout_a,
                                int act_a, egn_ref xb, egn_ref wb, egn_ref scale_b, egn_ref shift_b,
                                egn_ref res_b, egn_ref yb, int Nb, int Hb, int Wb, int Cin_b, int Cout_b,
                                int act_b, int grid_cap);
int egn_conv_pair_plan_query(int Na, int Ha, int Wa, int Cin_a, int Cout_a, int Nb, int Hb, int Wb,
                             int Cin_b, int Cout_b, int cus, int with_stats, int with_tickets, int* out);
/* The f16-OPERAND 3x3 / stride 1 / pad 1 convolution (csrc/conv_h.hip): the opt-in fast inference mode
 * (PoseHighResolutionNet.precision = 'f16').  Activations stay fp32 NHWC (x [N][H][W][Cin], y / res [N][H][W][Cout],
 * unpadded channel strides); every activation element is rounded to f16 (nearest-even, saturating at +-65504) while it
 * is staged, the filter is rounded once on the host (engine.pack_conv_weight_f16, egn_conv3x3_h_wpack_bytes bytes in the
 * MFMA B-operand layout), products run on v_mfma_f32_16x16x32_f16 with fp32 accumulators:
 *     y = act(conv(f16(x), f16(w)) * scale + shift (+ res)),    act = EGN_ACT_NONE or EGN_ACT_RELU.
 * The family lives beside the tile-config table (no config id, never a tuner answer).  egn_conv3x3_h_applies is its one
 * predicate, host-only (no GPU needed): 1 where the family takes the layer -- Cin, Cout in {48, 96, 192, 384} with
 * cs == C, N >= 1, H, W >= 2, tensors below 2 GiB, a plain epilogue -- else 0 (the Pedestrian widths 32 / 64 / 128 / 256
 * and 256 -> 48 are refused); the other entry points return EGN_E_BADARG where it says 0.  The reference has no
 * counterpart (libs/model/heatmapModel/hrnet.py:63-92 runs these layers as fp32 torch calls). */
int egn_conv3x3_h_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act);
long egn_conv3x3_h_wpack_bytes(int Cin, int Cout);
int egn_conv3x3_h_f32(const float* x, const void* wpack_f16, const float* scale, const float* shift,
                      const float* res, float* y, int N, int H, int W, int Cin, int Cout, int act,
                      void* stream);
/* the same as a program op (fork / join lanes, egn_program_run_timed, egn_program_op_info, capture / replay); res may be NULL */
int egn_program_add_conv3x3_h(egn_program* p, egn_ref x, egn_ref wpack, egn_ref scale, egn_ref shift,
                              egn_ref res, egn_ref y, int N, int H, int W, int Cin, int Cout, int act);
/* The same family at STRIDE 2 (3x3 / stride 2 / pad 1; PoseHighResolutionNet.precision = 'f16s2'): x [N][H][W][Cin],
 * y [N][Ho][Wo][Cout] with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1 -- H, W are the INPUT size everywhere.  The same
 * kernel, rounding and filter pack (engine.pack_conv_weight_f16: its layout does not depend on the stride) as above:
 *     y = act(conv_s2(f16(x), f16(w)) * scale + shift),    act = EGN_ACT_NONE or EGN_ACT_RELU;    no residual.
 * egn_conv3x3s2_h_applies is its one predicate, host-only: 1 where Cin, Cout in {48, 96, 192, 384} with cs == C, N >= 1,
 * H, W >= 2, input and output below 2 GiB, act none / ReLU -- else 0 (256 -> 96, the stem's 3 -> 64 and 64 -> 64 are
 * refused); the other entry points return EGN_E_BADARG where it says 0.  The reference runs these layers as fp32 torch
 * calls (libs/model/heatmapModel/hrnet.py, the transition and fuse layers). */
int egn_conv3x3s2_h_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int act);
int egn_conv3x3s2_h_f32(const float* x, const void* wpack_f16, const float* scale, const float* shift, float* y,
                        int N, int H, int W, int Cin, int Cout, int act, void* stream);
/* as a program op with a kind id of its own (13; egn_program_op_info: flops = 2 * 9 * N * Ho * Wo * Cout * Cin) */
int egn_program_add_conv3x3s2_h(egn_program* p, egn_ref x, egn_ref wpack, egn_ref scale, egn_ref shift, egn_ref y,
                                int N, int H, int W, int Cin, int Cout, int act);
/* The same family for the 32-MULTIPLE widths (PoseHighResolutionNet.precision = 'f16x'): the same kernel walking the input
 * channels in chunks of 32 instead of 48, stride 1 or 2 (H, W are the INPUT size; Ho = (H - 1) / stride + 1), the same
 * rounding, accumulators and epilogue:
 *     y = act(conv(f16(x), f16(w)) * scale + shift (+ res)),    act = EGN_ACT_NONE or EGN_ACT_RELU;  res at stride 1 only.
 * The filter pack is engine.pack_conv_weight_f16x: [Cout/16][Cin/32][9 taps][64 lanes][8] f16, egn_conv3x3_hx_wpack_bytes
 * = Cout * Cin * 9 * 2 bytes (0 for widths the family does not take).  egn_conv3x3_hx_applies is its one predicate,
 * host-only: 1 where Cin in {32, 64, 128, 256}, Cout in {32, 64, 128, 256, 48, 96} with cs == C, N >= 1, H, W >= 2, input
 * and output below 2 GiB, act none / ReLU, stride 1 or 2, no residual at stride 2 -- else 0 (Cin = 48 and its multiples
 * belong to the two predicates above, whose answers do not change); the other entry points return EGN_E_BADARG where it
 * says 0.  These are HRNet-W32's stage / transition / fuse layers and, in every width, layer1's 64 -> 64, the stem's
 * second convolution and transition1 (256 -> C). */
int egn_conv3x3_hx_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act,
                           int stride);
long egn_conv3x3_hx_wpack_bytes(int Cin, int Cout);
int egn_conv3x3_hx_f32(const float* x, const void* wpack_f16, const float* scale, const float* shift,
                       const float* res, float* y, int N, int H, int W, int Cin, int Cout, int act, int stride,
                       void* stream);
/* as a program op with a kind id of its own (14; egn_program_op_info: flops = 2 * 9 * N * Ho * Wo * Cout * Cin); res may be NULL */
int egn_program_add_conv3x3_hx(egn_program* p, egn_ref x, egn_ref wpack, egn_ref scale, egn_ref shift,
                               egn_ref res, egn_ref y, int N, int H, int W, int Cin, int Cout, int act, int stride);
/* f16 STORAGE between two ops of the family (PoseHighResolutionNet.activations = 'f16'): x_f16 = 1 reads x as f16
 * [N][H][W][Cin] (8 channels per 16-byte load, staged as they lie), y_f16 = 1 writes y as f16 [N][Ho][Wo][Cout] -- after
 * scale / shift and the activation every element goes through the very rounding the staging applies to an fp32 x (clamp to
 * +-65504, nearest-even), so a reader with x_f16 = 1 sees the operand bits it would have made of the fp32 tensor and every
 * fp32 output downstream keeps its bits.  ck (48 or 32) and stride (1 or 2) name the chunk size and stride the three
 * predicates above stand for; egn_conv3x3_h16_applies is theirs with the flags: it also wants x_f16, y_f16 in {0, 1} and no
 * residual beside y_f16 (the 2 GiB condition stays at fp32 sizes); host-only.  With both flags 0 the entries below compute
 * what the entries above compute. */
int egn_conv3x3_h16_applies(int N, int H, int W, int Cin, int cs_in, int Cout, int cs_out, int has_res, int act,
                            int stride, int ck, int x_f16, int y_f16);
int egn_conv3x3_h16_f32(const void* x, const void* wpack_f16, const float* scale, const float* shift, const float* res,
                        void* y, int N, int H, int W, int Cin, int Cout, int act, int stride, int ck, int x_f16, int y_f16,
                        void* stream);
/* as a program op of the kind its chunk size and stride have above (12, 13 or 14); egn_program_op_info counts an f16 tensor
 * as 2 bytes an element; res may be NULL */
int egn_program_add_conv3x3_h16(egn_program* p, egn_ref x, egn_ref wpack, egn_ref scale, egn_ref shift, egn_ref res,
                                egn_ref y, int N, int H, int W, int Cin, int Cout, int act, int stride, int ck, int x_f16,
                                int y_f16);
/* number of kernel launches issued through egn_program_run / _run_timed / _replay
 * since the library was loaded (process wide, all devices).  Test hook: a caller
 * can prove that a forward went through this library's kernels. */
long egn_launch_count(void);
/* number of convolution-class launches issued through the DIRECT entry points (egn_conv2d_f32,
 * egn_conv2d_bnstats_f32, egn_conv2d_wgrad_f32) since the library was loaded: the training tape and the
 * torch.autograd bridge (egonet_amd/autograd.py; replaces the MIOpen convolutions torch would run for
 * libs/trainer/trainer.py:191-197) do not go through programs -- this is their proof. */
long egn_direct_conv_count(void);
/* per-op metadata for reports */
int egn_program_op_info(const egn_program* p, int i, int* kind, double* flops,
                        double* bytes, char* tag, int tag_len);

/* ------------------------------------------------------------------------
 * The lifter's training pairs, built and kept on the device (csrc/lifter_pairs.hip).  Replaces the host loops of
 * libs/dataset/KITTI/car_instance.py:611-644, 730-790, 902-1010, 1051-1086 and basic_classes.py:26-44.
 * Every launch of this group is added to egn_launch_count().
 *
 * egn_lifter_pairs_f64: all samples of all labels, filtered and compacted in the reference's order.
 *   labels [A][7] f64 (l h w x y z rot_y), label_frame [A] i32 in [0, F) (the caller checks it; an index outside is
 *   clamped into the table, never read out of bounds), frames [F][14] f64 (K row major, shift, width, height),
 *   draws [A][7T+1] f64 (T x 3 rotation, T x 3 translation, T + 1 yaw draws; NULL = none, then T must be 0),
 *   coef0 / coef1 / ncoef (1 or 2): the edge interpolation coefficients, J = 9 + 12 * ncoef key points,
 *   out_root != 0: 'R3d+T' rows (3J values), else 'R3d' (3(J-1)).
 *   ws: egn_lifter_pairs_ws_bytes(A, T) bytes; afterwards its first 8 bytes hold the kept row count N (int64) and
 *   its tail the A(T+1) keep flags (uint8, at ws + ws_bytes(A, T) - A(T+1)).
 *   in2d [A(T+1)][2J] f32, out3d [A(T+1)][3(J-1)|3J] f32, roots [A(T+1)][3] f64: the first N rows are written.
 *   A(T+1) must stay below 2^31 (else EGN_E_BADARG / a negative ws size): build a larger set in parts.  Row and byte
 *   offsets are 64-bit throughout. */
long egn_lifter_pairs_ws_bytes(int A, int T);
int egn_lifter_pairs_f64(const double* labels, const int* label_frame, int A, const double* frames, int F,
                         const double* draws, int T, double coef0, double coef1, int ncoef, int out_root,
                         void* ws, long ws_bytes, float* in2d, float* out3d, double* roots, void* stream);
/* column mean and population deviation (np.std, ddof 0) of x [N][C] f32, C <= 128: float64 sums in a fixed order
 * (bit-reproducible), two passes, rounded to float32 at the end.  ws: egn_col_mean_std_ws_bytes(C) bytes. */
long egn_col_mean_std_ws_bytes(int C);
int egn_col_mean_std_f32(const float* x, long N, int C, void* ws, long ws_bytes, float* mean, float* stdv,
                         void* stream);
/* x[r][c] = (x[r][c] - mean[c]) / stdv[c] in place, float32, both operations correctly rounded (operations.py:47) */
int egn_normalize_rows_f32(float* x, long N, int C, const float* mean, const float* stdv, void* stream);
/* dst[i][:] = src[idx[i]][:], i < n; idx int64 on the device; an index outside [0, nrows) yields zeros */
int egn_gather_rows_f32(const float* src, long nrows, int C, const int64_t* idx, int n, float* dst, void* stream);

/* ------------------------------------------------------------------------
 * The 2-D pose annotations the key-point model trains on, built on the device (csrc/pose_annot.hip; the cuboid is
 * the lifter pairs' own, csrc/cuboid_math.h).  Replaces the host loops of libs/dataset/KITTI/car_instance.py:221-262
 * (_prepare_key_points_custom -> get_2d_3d_pair without augmentation) and :304-346 (_prepare_2d_pose_annot ->
 * kpts2cs method 'boundary', cs2bbox, int()).  Every launch is added to egn_launch_count().
 *
 * egn_pose2d_annot_f64: per label the J-point cuboid, posed and projected with the frame's intrinsics; a point is
 * visible when 0 < u < width and 0 < v < height.  Level 1 ("raw") keeps a label when visible / J >= inlier_share,
 * level 2 ("kept") when it also has >= min_visible visible points.  Both levels are compacted in label order.
 *   labels [A][7] f64 (l h w x y z rot_y), alpha [A] f64, label_frame [A] i32 in [0, F) (the caller checks it; an
 *   index outside is clamped into the table, never read out of bounds), frames [F][14] f64 (K row major, shift,
 *   width, height), coef0 / coef1: the edge interpolation coefficients, J = 33 (both) or 21 (coef0 only).
 *   ws: egn_pose2d_annot_ws_bytes(A) bytes of scratch.
 *   raw_kpts [A][J][3] f64 (u, v, visible): the first totals[0] rows are written;
 *   kpts [A][J][2] f64, boxes [A][4] i32, rots [A][2] f64 (alpha, rot_y), src [A] i32 (the label's index): the
 *   first totals[1] rows are written.  A box is centre -/+ half-size with centre = (min + max) / 2 and half-size =
 *   (max - min) * enlarge / 2 over all J points, each corner truncated toward zero (saturated to the int32 range).
 *   frame_raw / frame_kept [F] i32: instances of each frame at the two levels; totals [2] i64.
 *   A = 0 is allowed (the pointers sized by A may then be NULL): the counts and totals are zeroed. */
long egn_pose2d_annot_ws_bytes(int A);
int egn_pose2d_annot_f64(const double* labels, const double* alpha, const int* label_frame, int A,
                         const double* frames, int F, double coef0, double coef1, int J, double inlier_share,
                         int min_visible, double enlarge, void* ws, long ws_bytes, double* raw_kpts, double* kpts,
                         int* boxes, double* rots, int* src, int* frame_raw, int* frame_kept, int64_t* totals,
                         void* stream);

/* ------------------------------------------------------------------------
 * The lifter's 3-D validation metrics on the device (csrc/lifter_metrics.hip, per-row math in csrc/metric_math.h).
 * Replaces the host loops of libs/metric/criterions.py:223-301 (update_statistics, update_joints_3d_error style
 * 'direct', update_rotation_error style 'euler') behind RError3D / RTError3D (:390-538) and the per-batch
 * .cpu().numpy() + unnormalise of libs/trainer/trainer.py:474-481.  Every launch is added to egn_launch_count().
 *
 * layout 0 = 'R3d': rows of D = 96 float32 (32 points relative to the root); result columns [0,32) _rT point
 *   distances, [32,35) _R |Euler 'xyz' angles| in degrees of the Kabsch rotation prediction -> target: 35 columns.
 * layout 1 = 'R3d+T': D = 99, the root first; the same 35 columns, then [35] _T root distance and [36,39) _T_xyz
 *   |root difference|: 39 columns.
 * Accumulator: EGN_LIFTER_METRICS_ACC_DOUBLES float64 on the device: [0] row count, [1] layout, [8 + c] column sums,
 *   [48 + c] maxima, [88 + c] minima (c < 40; columns past the layout's keep the initial values).  The mean of a column
 *   is sum / count.  egn_lifter_metrics_reset sets count and sums to 0, maxima to -1 and minima to 1e16, the
 *   reference's initial values (criterions.py:403-411); it must run once before the first update.
 * egn_lifter_metrics_update_f32 folds n rows in: pred / gt [n][ld] float32 (ld >= D floats between rows), mean_out /
 *   std_out [D] float32 or both NULL: x * std + mean first, in float32, product and sum rounded separately
 *   (operations.py:50-52 on float32 arrays); everything after it is float64.  ws: egn_lifter_metrics_ws_bytes(n)
 *   bytes (grows with n up to 2048 rows, constant beyond), contents irrelevant between calls.  rows_out [n][35 | 39]
 *   float64 or NULL: the per-row columns.  Two launches: the block partials (plain stores, no atomics) and their fold
 *   into acc in block order, so equal inputs give equal bits.  n == 0 is a no-op; n < 0, a NULL pred / gt / ws / acc,
 *   a D other than 96 (layout 0) / 99 (layout 1), ld < D, one of mean_out / std_out alone or a short ws: EGN_E_BADARG.
 *   A row whose predicted (or target) points coincide has rotation error 0 like the reference; see metric_math.h for
 *   rank-1 rows.  Non-finite inputs reach the sums like they reach the reference's distances, never max / min. */
#define EGN_LIFTER_METRICS_ACC_DOUBLES 128
long egn_lifter_metrics_ws_bytes(long n);
int egn_lifter_metrics_reset(double* acc, int layout, void* stream);
int egn_lifter_metrics_update_f32(const float* pred, const float* gt, long n, int D, int ld, const float* mean_out,
                                  const float* std_out, int layout, void* ws, long ws_bytes, double* acc,
                                  double* rows_out, void* stream);

/* ------------------------------------------------------------------------
 * The key-point model's source-image metric on the device (csrc/kpt_metrics.hip, per-instance math in
 * csrc/kpt_metric_math.h).  Replaces the host loop of libs/metric/criterions.py:68-143 (get_distance_src: rescale,
 * inverse crop affine, get_distance :17-37, get_PCK :57-66) behind JointDistance2DSIP (:173-224) and the metric_func of
 * the training loop (libs/trainer/trainer.py:200-205).  Every launch is added to the launch counter.
 *
 * Accumulator: EGN_KPT_METRICS_ACC_DOUBLES float64 on the device: [0] joints counted, [1] sum of their distances,
 *   [2..4] joints closer than 0.1 / 0.2 / 0.3 of the instance's PCK denominator, the rest zero.  The mean distance is
 *   [1] / [0].  The reset zeroes it; it must run once before the first update.
 * The update folds one batch in.  Prediction, exactly one of
 *   hm      [N][K][H][W] float32 heat-maps, decoded like the decode entry point above does with the same `mode`
 *           (0 hard, 1 soft, 2 soft-np; bit-identical, one decoder) and multiplied by float32(img_w / W);
 *   coords  [N][K][2] float32 in [0, 1] (the coordinate head), multiplied by float32 (img_w, img_h).
 *   Labels of the first n <= N predictions, float64: center [n][2], scale [n][2] (x 200 px), rotation [n] in degrees
 *   (NULL = zeros), original_joints [n][K][3] (x, y, visibility; a joint counts when visibility != 0).  The crop window
 *   is img_w x img_h.  Per labelled instance the inverse crop affine is built in float64 from the reference's three
 *   point pairs held in float32 (img_proc.py:26-64, inv=1); the PCK denominator is (max y - min y) / 3 over ALL K
 *   annotated joints.
 *   ws: the ws_bytes query's size for (N, K), contents irrelevant between calls.  Optional outputs, each may be NULL:
 *   src_coord [n][K][2] float64 (predictions in the source image), joints_pred [N][K][2] float32 (rescaled
 *   predictions), max_vals [N][K] float32 (raw maxima; heat-maps only, untouched with coords).
 *   Two launches: one wavefront per map writes block partials (plain stores, no atomics), a single block folds them
 *   into acc in block order, so equal inputs give equal bits.  N == 0 is a no-op.  Both or neither of hm / coords,
 *   n > N, N * K or H * W past 2^31 - 1, a mode outside 0..2, a NULL label array with n > 0, a NULL ws / acc, a
 *   non-positive window or a short ws: EGN_E_BADARG. */
#define EGN_KPT_METRICS_ACC_DOUBLES 8
long egn_kpt_metrics_ws_bytes(int N, int K);
int egn_kpt_metrics_reset(double* acc, void* stream);
int egn_kpt_metrics_update_f32(const float* hm, const float* coords, int N, int K, int H, int W, int mode,
                               const double* center, const double* scale, const double* rotation,
                               const double* original_joints, int n, double img_w, double img_h, void* ws,
                               long ws_bytes, double* acc, double* src_coord, float* joints_pred, float* max_vals,
                               void* stream);

/* ------------------------------------------------------------------------
 * The angle-regression baselines' metric on the device (csrc/angle_metrics.hip).  Replaces the per-batch
 * .cpu().numpy() of libs/metric/criterions.py:40-55 (get_angle_error) behind AngleError (:145-171) and the metric_func
 * of the training loop (libs/trainer/trainer.py:200-205).  Every launch is added to the launch counter.
 *
 * Accumulator: EGN_ANGLE_METRICS_ACC_DOUBLES float64 on the device: [0] rows counted, [1] sum of their errors in
 *   degrees; the mean error is [1] / [0].  The reset zeroes it; it must run once before the first update.
 * The update folds one batch in: row i of pred (float32, row pitch ld >= 2 floats, only columns 0 and 1 are read:
 *   [cos, sin]) against angles_gt[i] (float64, radians): d = |gt - atan2(sin, cos)| * 180 / pi with the atan2 in
 *   float64, and 360 - d where d > 180.
 *   ws: the ws_bytes query's size for N, contents irrelevant between calls.
 *   Two launches: one thread per row, one {count, sum} partial per block (plain stores, no atomics); a single wave
 *   folds the partials into acc in a fixed order, so equal inputs give equal bits.  N == 0 is a no-op (no launch).
 *   N < 0 or past 2^31 - 1, ld < 2, a NULL acc, and with N > 0 a NULL pred / angles_gt / ws or a short ws:
 *   EGN_E_BADARG. */
#define EGN_ANGLE_METRICS_ACC_DOUBLES 2
long egn_angle_metrics_ws_bytes(long N);
int egn_angle_metrics_reset(double* acc, void* stream);
int egn_angle_metrics_update_f32(const float* pred, long N, int ld, const double* angles_gt, void* ws, long ws_bytes,
                                 double* acc, void* stream);

/* ------------------------------------------------------------------------
 * Reprojection refinement of lifted cuboids against their own 2-D key points (csrc/pnp_refine.hip, math in
 * csrc/pnp_math.h): the reference's pnp_refine (libs/common/transformation.py:143-157) with the flow of
 * tools/inference_legacy.py:518-547, for a batch in one launch.  Per instance a rigid pose (R, T) minimises
 *     sum_i w_i | pi(R X_i + T) - k_i |^2,   X_0 = 0 (the root), X_i = shape[i-1],
 * pi the pinhole projection with (fx, fy, cx, cy); no distortion, no scale.  Levenberg-Marquardt from R = I and
 * T = root0 (or, root0 == NULL, the weak-perspective start z0 = sqrt(sum w (Sx^2 + Sy^2) / sum w |(k_i - k_0)/fx|^2),
 * T = z0 K^-1 (k_0, 1)); left-multiplicative rotation update, analytic Jacobian, 6x6 normal equations with
 * Marquardt's diagonal scaling, Cholesky; a step is taken only if the cost does not increase (decided down to the resolution of the cost's own
 * evaluation, EGN_PNP_COST_RES); ends on a step below
 * EGN_PNP_STEP_TOL or after EGN_PNP_MAX_ITERS trial steps (pnp_math.h).  It is pinned on the optimum of this
 * objective, not on cv2.solvePnP: it starts from the prediction rather than from a DLT, so on an instance with
 * several minima the two can end in different ones.
 *   shape   [n, J-1, 3] f64   lifted shape relative to the root
 *   kpts2d  [n, J, 2]   f64   screen key points, key point 0 = the root's projection
 *   intr    [n, 4]      f64   fx fy cx cy
 *   weights [n, J]      f64 or NULL (ones); a weight that is not > 0 drops the correspondence
 *   root0   [n, 3]      f64 or NULL
 *   max_shift                 >= 0 or +inf; applies only with root0
 *   refined [n, J, 3]   f64   absolute camera coordinates, root first
 *   rt      [n, 12]     f64   R row-major, then T, of the returned placement
 *   cost    [n, 2]      f64   weighted squared pixel error at the start / of the returned placement
 *   iters   [n] i32           trial steps taken
 *   status  [n] i32           1 refined;  0 converged but |T - root0| > max_shift;  -1 not usable (a used point with
 *                             z <= 0 at the start, a non-finite start, a singular system, or the cap reached).
 *                             For 0 and -1 the output is the unrefined placement [T_start; T_start + shape],
 *                             rt = (I, T_start) and cost[1] = cost[0]; every output is finite for finite inputs.
 *   dims    [n, 3]      f64   (l, h, w): mean edge lengths of the returned cuboid, corners = points 1..8, by the
 *                             rule of the pose solve (zeros when J < 9)
 * 2 <= J <= 64; n == 0 is a no-op (no launch); n < 0, a J outside the range, a negative or NaN max_shift, or with
 * n > 0 a NULL required pointer: EGN_E_BADARG.  One launch, one wave per instance, added to the launch counter;
 * fixed-order sums, so equal inputs give equal bits.  The _host_ entry runs the same header as a plain loop over
 * HOST pointers (numpy inputs / a CPU model) and is never used for device tensors.
 * ---------------------------------------------------------------------- */
int egn_pnp_refine_f64(const double* shape, const double* kpts2d, const double* intr, const double* weights,
                       const double* root0, int n, int J, double max_shift, double* refined, double* rt,
                       double* cost, int* iters, int* status, double* dims, void* stream);
int egn_pnp_refine_host_f64(const double* shape, const double* kpts2d, const double* intr, const double* weights,
                            const double* root0, int n, int J, double max_shift, double* refined, double* rt,
                            double* cost, int* iters, int* status, double* dims);

/* ------------------------------------------------------------------------
 * Overlay rasteriser (csrc/overlay.hip, definition in csrc/overlay_math.h): draws predictions into uint8 frames.
 * One primitive, the capsule: a segment (x0,y0)-(x1,y1) of radius r in an RGB8 colour at opacity a (clamped to
 * [0, 1]); a zero-length segment is a disc.  Primitives are drawn in list order; one with a non-finite field or
 * r < 0 is dropped.  Pixel (x, y) has its centre at the integer coordinates.  Per pixel and primitive, in float64
 * without contraction:
 *     t = clamp(((p - p0) . (p1 - p0)) / |p1 - p0|^2, 0, 1), 0 for a zero length;   d = |p - p0 - t (p1 - p0)|
 *     c = antialias ? clamp(r + 0.5 - d, 0, 1) : (d <= r);   w = c a
 *     if w > 0, per channel:  v = floor(v + (col - v) w + 0.5), stored as uint8 before the next primitive
 * so the device and the host entry give the same bytes, and a pixel no primitive reaches keeps its byte.
 *   base              frames are addressed relative to it
 *   frames [n_frames][6] i64  byte offset from base (>= 0), H, W, row stride in bytes (>= 3 W, any alignment),
 *                             first primitive, one past the last; frames are uint8 HWC, RGB interleaved, and may
 *                             differ in size
 *   max_h, max_w              the largest H and W of the table: the grid is (tiles x, tiles y, frame) of 32 x 32
 *                             pixel tiles, and blocks outside a smaller frame exit
 *   prims  [n_prims][6] f32   x0 y0 x1 y1 r a
 *   colors [n_prims]    u32   R | G << 8 | B << 16
 *   cull                      1: every tile walks the primitives in chunks of egn_overlay_tile_capacity(), keeps those
 *                             whose grown bounding box meets the tile, in index order, in an LDS list, and draws from
 *                             it; 0: every primitive goes to every tile (kept for the measurement of what the
 *                             binning buys).  Both give the same bytes.
 * n_frames == 0 or n_prims == 0 is a successful no-op.  EGN_E_BADARG: a negative count or size, more than 65535
 * frames, a NULL required pointer; the host entry also refuses a table row with a negative size or offset, a stride
 * below 3 W or a primitive range outside [0, n_prims].  The device entry cannot read its table without a
 * synchronisation: there a block that finds such a row draws nothing into that frame (callers check the table while
 * it is still on the host, as egonet_amd.visualization.OverlayRenderer does).  One launch on `stream`, added to the
 * launch counter; no synchronisation, no allocation.  The _host_ entry takes HOST pointers and is never used for
 * device frames.
 * ---------------------------------------------------------------------- */
int egn_overlay_tile_capacity(void);
int egn_overlay_draw_u8(void* base, const int64_t* frames_dev, int n_frames, int max_h, int max_w,
                        const float* prims_dev, const uint32_t* colors_dev, int n_prims, int antialias, int cull,
                        void* stream);
int egn_overlay_draw_host_u8(void* base, const int64_t* frames, int n_frames, const float* prims,
                             const uint32_t* colors, int n_prims, int antialias);

/* ------------------------------------------------------------------------
 * Training debug pictures (csrc/debug_pictures.hip, definition in csrc/debug_pictures_math.h): the grid of crops and
 * the heat-map mosaic of libs/visualization/debug.py:51-149, composed into caller-allocated uint8 RGB pictures.  The
 * pictures are pinned on the header's definition (no cv2 / torchvision pixel parity); markers are drawn afterwards
 * with the overlay rasteriser above.
 *
 * Range: lohi[0] / lohi[1] = minimum / maximum of x [n][c][hw] f32 over the first c_used channels, NaNs ignored, -0
 *   stored as +0, 0 0 when every value is a NaN.  Two launches (block partials with plain stores, one block folds
 *   them); min / max are exact, so equal inputs give equal bits.  ws: the ws_bytes query's bytes (-1: bad sizes).
 *   n * c_used * hw == 0 is a no-op that leaves lohi alone.
 * Crop value -> grey level: q = trunc(min(255, max(0, 255 (x - lo) / (hi - lo + 1e-5)))) in float64, 0 for a NaN.
 * Grid (make_grid(img[:, :3], nrow, pad, normalize=True)): out [ymaps (H + pad) + pad][xmaps (W + pad) + pad][3] with
 *   xmaps = min(nrow, N), ymaps = ceil(N / xmaps); crop k at row (k / xmaps)(H + pad) + pad, column
 *   (k % xmaps)(W + pad) + pad; padding and empty cells are zeros.  img [N][C][H][W] f32, C >= 3.
 * Mosaic: out [n h][(J + 1) w][3]; row block i is crop i; tile 0 is the crop's thumbnail (the quantised crop resized
 *   to w x h, bilinear on the uint8 values with half-pixel centres, rounded half up), tile j + 1 is
 *   (7 lut[q(maps[i][j])] + 3 thumbnail) / 10 in integers with q(m) = trunc(min(255, max(0, 255 m))), 0 for a NaN.
 *   maps [n][J][h][w] f32, img holds at least n crops, lut [256][3] u8 (egonet_amd.visualization.debug.jet_lut()).
 * out rows are `stride` bytes apart; bytes past 3 * width of a row are not touched.  lohi is read on the device.
 * A zero N / n, crop or map size is a successful no-op; a negative size, C < 3, nrow < 1, a NULL required pointer, a
 * stride below 3 * width or a picture size past 2^31 - 1: EGN_E_BADARG.  One launch each, added to the launch
 * counter; no allocation, no synchronisation.  The _host_ entries run the same header as plain loops over HOST
 * pointers and give the same bytes; they are never used for device tensors.
 * ---------------------------------------------------------------------- */
long egn_debug_range_ws_bytes(int n, int c_used, int hw);
int egn_debug_range_f32(const float* x, int n, int c, int c_used, int hw, void* ws, long ws_bytes, float* lohi,
                        void* stream);
int egn_debug_range_host_f32(const float* x, int n, int c, int c_used, int hw, float* lohi);
int egn_debug_grid_u8(const float* img, int N, int C, int H, int W, int nrow, int pad, const float* lohi,
                      uint8_t* out, long stride, void* stream);
int egn_debug_grid_host_u8(const float* img, int N, int C, int H, int W, int nrow, int pad, const float* lohi,
                           uint8_t* out, long stride);
int egn_debug_mosaic_u8(const float* img, int C, int H, int W, const float* maps, int n, int J, int h, int w,
                        const float* lohi, const uint8_t* lut, uint8_t* out, long stride, void* stream);
int egn_debug_mosaic_host_u8(const float* img, int C, int H, int W, const float* maps, int n, int J, int h, int w,
                             const float* lohi, const uint8_t* lut, uint8_t* out, long stride);

/* ------------------------------------------------------------------------
 * Inference plans (.egnplan): the planned, tuned and packed network of EgoNet.infer_crops(refine=None), written once
 * by egonet_amd.plan.export_plan and run from here with nothing but this library -- no Python, no model, no filter
 * packing, no autotune.  A file holds, per exported batch size, one HRNet and one lifter launch program as the list of
 * egn_program_* calls the engine made, the packed weights as pieces stored once, and the constants of the chain
 * (csrc/plan_format.h).  The reference has no counterpart (it builds its torch modules at every start).
 *
 * egn_plan_open / egn_plan_parse (a file in memory; the bytes are copied) are HOST-ONLY (csrc/plan.cpp, no HIP call).
 * Before they return 0 they have checked: magic, format version, egn_version and egn_conv_table_fingerprint of the
 * writer against this library's, the CRC-32 of every section; every count against the bytes that remain, before
 * anything is allocated; every op kind, argument count and dimension; every slot index; every wait (an earlier op
 * that signals); and for every pointer reference its offset and -- where the op's shape gives one -- its extent
 * against the size of the slot it points into.  A file that fails is never loaded:
 *   EGN_E_PLAN_IO           the file cannot be read
 *   EGN_E_PLAN_TRUNCATED    the file ends inside or before a section (the END section closes a file)
 *   EGN_E_PLAN_MAGIC / _VERSION (format or library) / _FINGERPRINT (the tile-config ids mean something else) / _CRC
 *   EGN_E_PLAN_COUNT        a count or length larger than the bytes that remain in its section (or than its cap)
 *   EGN_E_PLAN_OP           an unknown op kind
 *   EGN_E_PLAN_SLOT         a slot index outside the program's slots (or NULL where a pointer is required)
 *   EGN_E_PLAN_REF          an offset, or offset + extent, past its slot; an offset that is not 16-byte aligned
 *   EGN_E_PLAN_WAIT         a wait on a later op, on itself or on an op that does not signal
 *   EGN_E_PLAN_FORMAT       anything else inconsistent (section order, roles, dimensions, missing programs)
 * egn_plan_get_info / _get_text (what = 0 arch, 1 the EGONET_AMD_* switches of the recording) / _get_stats (which =
 * 0..3: mean_in, std_in, mean_out, std_out; n must be the vector's length) / _program_info (per program: type 0 HRNet /
 * 1 lifter, its batch size, arena and weight bytes, op count, ops with waits, the op kinds -- kinds may be NULL) /
 * _op_record (the canonical little-endian record of one op: u32 kind, lane, signal, nwaits, waits[], nints, i32 ints[],
 * u32 nrefs, {i32 slot, i64 off}[], f64 flops, f64 bytes, u32 tag length, tag; buf NULL: only *used) read a parsed plan.
 *
 * egn_plan_load (device >= 0: hipSetDevice first; < 0: the current device) uploads every piece once, assembles each
 * program's weights slot on the device, replays the calls into egn_programs (the filter extent of every convolution
 * is checked against its tile config's layout first) and allocates ONE arena and one set of temporaries for the
 * largest exported size.  Everything is freed by egn_plan_close.
 * egn_plan_infer runs infer_crops' chain on `stream`: all pointers are DEVICE pointers; crops [n,C,H,W] fp32,
 * centers / scales [n,2] f64; outputs local [n,J,2] fp32, kpts_2d [n,2J] f64, kpts_3d [n,D] f64 and, for the 96-output
 * lifter, euler [n,3] f64 and alpha [n] f64 (alpha_mode 0 'proj' needs has_K with fx, cx; without K it is 'trans', as
 * in infer_crops).  It allocates nothing and never waits for the device.  An n that is not an exported size runs as
 * chunks of exported sizes, greedy from the largest; an n that cannot be composed is EGN_E_BADARG before anything is
 * launched.  Eager runs only (no capture / replay); one plan runs one call at a time (a call on another stream is
 * ordered behind the previous one).  Out of scope: refine = 'pnp', kpts_x_for_alpha, the second in-flight copy
 * (slot = 1), training.
 * egn_plan_native_program: the egn_program of program index `program` of a LOADED plan (NULL otherwise), owned by the
 * plan -- for egn_program_num_ops / _op_info / _ticket_ops / _run_timed.
 *
 * egn_conv_table_fingerprint (host only): CRC-32 over every tile-config id's kind, tile sizes and kernel symbol.
 * egn_box_to_crop_f64 (host only, HOST pointers): boxes [n,4] (left, top, right, bottom) -> modify_bbox's center [n,2]
 * and scale [n,2] (enlarge about the centre, then grow to target_ar = height / width of the crop) and, unless M is
 * NULL, the forward affines M [n,6] image -> crop that egn_crop_frames_warp_normalize_u8 takes: the float64 bits of
 * common/img_proc.py::modify_bbox and common/crop_gpu.py::forward_affines (egonet.py:105-155, img_proc.py:26-64).
 * ---------------------------------------------------------------------- */
#define EGN_E_PLAN_IO          (-10)
#define EGN_E_PLAN_TRUNCATED   (-11)
#define EGN_E_PLAN_MAGIC       (-12)
#define EGN_E_PLAN_VERSION     (-13)
#define EGN_E_PLAN_FINGERPRINT (-14)
#define EGN_E_PLAN_CRC         (-15)
#define EGN_E_PLAN_COUNT       (-16)
#define EGN_E_PLAN_OP          (-17)
#define EGN_E_PLAN_SLOT        (-18)
#define EGN_E_PLAN_REF         (-19)
#define EGN_E_PLAN_WAIT        (-20)
#define EGN_E_PLAN_FORMAT      (-21)

typedef struct egn_plan egn_plan;
typedef struct egn_plan_info {
  int format_version, lib_version;
  unsigned fingerprint;
  char arch[32];
  int precision;              /* 0 f32, 1 f16, 2 f16s2, 3 f16x */
  int head_type;              /* 0 coordinates, 1 heatmap */
  int decode;                 /* 0 hard, 1 soft, 2 coords */
  int J, C, H, W, map_h, map_w;
  double mul_x, mul_y;
  int lifter_in, lifter_out, ld_in;
  int n_sizes, sizes[64];
  int n_pieces, n_programs, loaded;
} egn_plan_info;
typedef struct egn_plan_outputs {
  float* local;
  double* kpts_2d;
  double* kpts_3d;
  double* euler;
  double* alpha;
} egn_plan_outputs;

unsigned egn_conv_table_fingerprint(void);
int egn_plan_open(const char* path, egn_plan** plan);
int egn_plan_parse(const void* bytes, size_t n, egn_plan** plan);
void egn_plan_close(egn_plan* plan);
int egn_plan_get_info(const egn_plan* plan, egn_plan_info* info);
int egn_plan_get_text(const egn_plan* plan, int what, char* buf, int len);
int egn_plan_get_stats(const egn_plan* plan, int which, double* out, int n);
int egn_plan_program_info(const egn_plan* plan, int program, int* type, int* n, long long* arena_bytes,
                          long long* weight_bytes, int* n_ops, int* ops_with_waits, int* kinds, int kinds_len);
int egn_plan_op_record(const egn_plan* plan, int program, int op, void* buf, int len, int* used);
int egn_plan_load(egn_plan* plan, int device);
egn_program* egn_plan_native_program(const egn_plan* plan, int program);
int egn_plan_infer(egn_plan* plan, const float* crops, int n, const double* centers, const double* scales, int has_K,
                   double fx, double cx, int alpha_mode, const egn_plan_outputs* outputs, void* stream);
int egn_box_to_crop_f64(const double* boxes, int n, double target_ar, double enlarge, int out_w, int out_h,
                        double* center, double* scale, double* M);

#ifdef __cplusplus
}
#endif
#endif /* EGONET_HIP_H */
