// plan_run.hip -- load a validated plan file (plan.cpp) onto the current device and run EgoNet.infer_crops' chain from it:
// HRNet program -> egn_keypoints_to_screen_f64 -> lifter program -> egn_unnormalize_f64 -> egn_pose_solve_f64, the entry
// points the Python engine calls, in its order.  The programs are replayed from the file's call lists through the public
// egn_program_* entries, so a plan launches what the engine that wrote it launches.
#include <string.h>

#include <algorithm>
#include <vector>

#include "egn_internal.h"
#include "plan_format.h"

namespace {

struct LoadedProgram {
  egn_program* prog = nullptr;
  void* weights = nullptr;
  const PlanProgram* desc = nullptr;
};

struct Runtime {
  int device = 0;
  void* arena = nullptr;                 // one arena for all programs: a plan never runs two of them at once
  std::vector<LoadedProgram> programs;
  std::vector<uint32_t> sizes;           // distinct exported sizes, largest first
  std::vector<int> hrnet_of, lifter_of;  // per entry of `sizes`: index into `programs`
  void* role_tmp[16] = {};               // temporaries by user-slot role, sized for the largest exported size
  double* ls[4] = {};                    // mean_in, std_in, mean_out, std_out
  double* kx = nullptr;
  hipEvent_t ev_done = nullptr;          // the arena and the temporaries are shared: a call on another stream waits
  hipStream_t last_stream = nullptr;
  bool ran = false;
};

void free_runtime(void* p) {
  Runtime* rt = static_cast<Runtime*>(p);
  if (!rt) return;
  if (rt->ev_done && rt->ran) hipEventSynchronize(rt->ev_done);
  for (LoadedProgram& g : rt->programs) {
    if (g.prog) egn_program_destroy(g.prog);
    if (g.weights) hipFree(g.weights);
  }
  if (rt->arena) hipFree(rt->arena);
  for (void* t : rt->role_tmp)
    if (t) hipFree(t);
  for (double* t : rt->ls)
    if (t) hipFree(t);
  if (rt->kx) hipFree(rt->kx);
  if (rt->ev_done) hipEventDestroy(rt->ev_done);
  delete rt;
}

// bytes of the filter layout the op's kernel reads (egn_conv_config_kind, include/egonet_hip.h): the parser knows only
// the least of them
uint64_t conv_filter_bytes(const PlanOp& op) {
  const uint64_t Cin = op.ints[3], Cout = op.ints[5], KH = op.ints[7], KW = op.ints[8];
  const int cfg = op.ints[13];
  const int kind = cfg > 0 ? egn_conv_config_kind(cfg) : 0;
  if (kind < 0) return UINT64_MAX;
  if (kind == 0) return ((Cin + 15) / 16 * 16) * KH * KW * ((Cout + 15) / 16 * 16) * 4;
  const uint64_t per = kind == 1 ? 16 : (kind == 2 ? 36 : 48);
  return Cout * Cin * per * 4;
}

egn_ref ref_of(const PlanRef& r) { return egn_ref{r.slot, r.off}; }

int replay_op(egn_program* p, const PlanProgram& g, const PlanOp& op) {
  if (op.kind == EGN_PLAN_OP_FORK) return egn_program_fork(p);
  if (op.kind == EGN_PLAN_OP_JOIN) return egn_program_join(p);
  int rc = egn_program_set_lane(p, (int)op.lane);
  if (rc) return rc;
  const int32_t* i = op.ints.data();
  egn_ref r[16];
  for (size_t k = 0; k < op.refs.size() && k < 16; ++k) r[k] = ref_of(op.refs[k]);
  switch (op.kind) {
    case EGN_PLAN_OP_CONV: {
      const uint64_t wsize = g.weight_bytes < 256 ? 256 : g.weight_bytes, need = conv_filter_bytes(op);
      if (op.refs[1].slot != 1 || (uint64_t)op.refs[1].off > wsize || need > wsize - (uint64_t)op.refs[1].off)
        return EGN_E_PLAN_REF;
      rc = egn_program_add_conv2d(p, r[0], r[1], r[2], r[3], r[4], r[5], i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], i[8],
                                  i[9], i[10], i[11], i[12], i[13]);
      break;
    }
    case EGN_PLAN_OP_CONVPAIR:
      rc = egn_program_add_conv2d_pair(p, r[0], r[1], r[2], r[3], r[4], r[5], i[0], i[1], i[2], i[3], i[4], i[5], r[6], r[7],
                                       r[8], r[9], r[10], r[11], i[6], i[7], i[8], i[9], i[10], i[11], i[12]);
      break;
    case EGN_PLAN_OP_CONVH:
      rc = egn_program_add_conv3x3_h(p, r[0], r[1], r[2], r[3], r[4], r[5], i[0], i[1], i[2], i[3], i[4], i[5]);
      break;
    case EGN_PLAN_OP_CONVH2:
      rc = egn_program_add_conv3x3s2_h(p, r[0], r[1], r[2], r[3], r[4], i[0], i[1], i[2], i[3], i[4], i[5]);
      break;
    case EGN_PLAN_OP_CONVHX:
      rc = egn_program_add_conv3x3_hx(p, r[0], r[1], r[2], r[3], r[4], r[5], i[0], i[1], i[2], i[3], i[4], i[5], i[6]);
      break;
    case EGN_PLAN_OP_FUSE:
      rc = egn_program_add_fuse(p, r[0], i[0], i[1], i[2], i[3], i[4], i[5], r + 1, i + 6, i[6 + i[5]]);
      break;
    case EGN_PLAN_OP_NCHW2NHWC:
      rc = egn_program_add_nchw_to_nhwc(p, r[0], r[1], i[0], i[1], i[2], i[3], i[4]);
      break;
    case EGN_PLAN_OP_NHWC2NCHW:
      rc = egn_program_add_nhwc_to_nchw(p, r[0], r[1], i[0], i[1], i[2], i[3], i[4]);
      break;
    case EGN_PLAN_OP_PIXSHUF:
      rc = egn_program_add_pixel_shuffle(p, r[0], r[1], i[0], i[1], i[2], i[3], i[4], i[5]);
      break;
    case EGN_PLAN_OP_RAMPS:
      rc = egn_program_add_ramps(p, r[0], i[0], i[1], i[2], i[3], i[4]);
      break;
    case EGN_PLAN_OP_DECODE:
      rc = egn_program_add_decode(p, r[0], i[0], i[1], i[2], i[3], i[4], r[1], r[2], r[3]);
      break;
    case EGN_PLAN_OP_PWPAIR:
      rc = egn_program_add_pw_pair(p, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], i[0], i[1]);
      break;
    default:
      return EGN_E_PLAN_OP;
  }
  if (rc) return rc;
  rc = egn_program_tag(p, op.tag.c_str(), op.flops, op.bytes);
  if (rc) return rc;
  if (op.signal || !op.waits.empty()) {
    std::vector<int> waits(op.waits.begin(), op.waits.end());
    rc = egn_program_set_deps(p, (int)op.signal, waits.data(), (int)waits.size());
  }
  return rc;
}

int load(egn_plan* plan, Runtime* rt) {
  const PlanInfo& h = plan->info;
  // the pieces: one upload each, then copied on the device to every place a program's weights slot has them
  std::vector<uint64_t> piece_off(plan->pieces.size());
  uint64_t total = 0;
  for (size_t k = 0; k < plan->pieces.size(); ++k) {
    piece_off[k] = total;
    total += (plan->pieces[k].nbytes + 255) / 256 * 256;
  }
  char* staged = nullptr;
  if (total) EGN_CHECK_HIP(hipMalloc(&staged, total));
  struct Guard { char* p; ~Guard() { if (p) hipFree(p); } } guard{staged};
  for (size_t k = 0; k < plan->pieces.size(); ++k)
    EGN_CHECK_HIP(hipMemcpy(staged + piece_off[k], plan->file.data() + plan->pieces[k].file_off, plan->pieces[k].nbytes,
                            hipMemcpyHostToDevice));
  uint64_t arena = 256, role_bytes[16] = {};
  for (const PlanProgram& g : plan->programs) {
    arena = std::max<uint64_t>(arena, g.arena_bytes);
    for (const PlanSlot& u : g.user) role_bytes[u.role] = std::max(role_bytes[u.role], u.nbytes);
  }
  EGN_CHECK_HIP(hipMalloc(&rt->arena, arena));
  EGN_CHECK_HIP(hipMemset(rt->arena, 0, arena));
  // the caller brings the crops and receives `local`; every other slot is a temporary
  const int local = h.decode == 2 ? EGN_PLAN_ROLE_COORDS : EGN_PLAN_ROLE_XY;
  for (int role = 1; role < 16; ++role) {
    if (!role_bytes[role] || role == EGN_PLAN_ROLE_CROPS || role == local) continue;
    EGN_CHECK_HIP(hipMalloc(&rt->role_tmp[role], role_bytes[role]));
    EGN_CHECK_HIP(hipMemset(rt->role_tmp[role], 0, role_bytes[role]));     // (the lifter input's padding columns stay 0)
  }
  for (int k = 0; k < 4; ++k) {
    EGN_CHECK_HIP(hipMalloc(&rt->ls[k], h.ls[k].size() * sizeof(double)));
    EGN_CHECK_HIP(hipMemcpy(rt->ls[k], h.ls[k].data(), h.ls[k].size() * sizeof(double), hipMemcpyHostToDevice));
  }
  rt->programs.reserve(plan->programs.size());
  for (const PlanProgram& g : plan->programs) {
    rt->programs.emplace_back();
    LoadedProgram& lp = rt->programs.back();
    lp.desc = &g;
    const uint64_t wsize = g.weight_bytes < 256 ? 256 : g.weight_bytes;
    EGN_CHECK_HIP(hipMalloc(&lp.weights, wsize));
    EGN_CHECK_HIP(hipMemset(lp.weights, 0, wsize));
    for (const PlanPlace& pl : g.places)
      EGN_CHECK_HIP(hipMemcpy((char*)lp.weights + pl.off, staged + piece_off[pl.piece], plan->pieces[pl.piece].nbytes,
                              hipMemcpyDeviceToDevice));
    lp.prog = egn_program_create(2 + (int)g.user.size());
    if (!lp.prog) return EGN_E_BADARG;
    int rc = egn_program_bind(lp.prog, 0, rt->arena);
    if (!rc) rc = egn_program_bind(lp.prog, 1, lp.weights);
    for (size_t k = 0; k < g.ops.size() && !rc; ++k) rc = replay_op(lp.prog, g, g.ops[k]);
    if (rc) return rc;
  }
  EGN_CHECK_HIP(hipDeviceSynchronize());
  rt->sizes = h.sizes;
  std::sort(rt->sizes.begin(), rt->sizes.end(), [](uint32_t a, uint32_t b) { return a > b; });
  rt->sizes.erase(std::unique(rt->sizes.begin(), rt->sizes.end()), rt->sizes.end());
  for (uint32_t s : rt->sizes)
    for (int type = 0; type < 2; ++type) {
      int found = -1;
      for (size_t k = 0; k < rt->programs.size() && found < 0; ++k)
        if (rt->programs[k].desc->type == (uint32_t)type && rt->programs[k].desc->n == s) found = (int)k;
      if (found < 0) return EGN_E_PLAN_FORMAT;
      (type ? rt->lifter_of : rt->hrnet_of).push_back(found);
    }
  EGN_CHECK_HIP(hipMalloc(&rt->kx, (size_t)rt->sizes[0] * sizeof(double)));
  EGN_CHECK_HIP(hipEventCreateWithFlags(&rt->ev_done, hipEventDisableTiming));
  return 0;
}

// kx[i] = screen[i][0]: the screen x of key point 0 (what `screen[:, 0].contiguous()` copies)
__global__ void plan_first_column_kernel(const double* __restrict__ screen, int n, int ld, double* __restrict__ kx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) kx[i] = screen[(size_t)i * ld];
}

}  // namespace

extern "C" int egn_plan_load(egn_plan* plan, int device) {
  if (!plan || plan->runtime) return plan ? EGN_E_STATE : EGN_E_BADARG;
  if (plan->file.empty()) return EGN_E_STATE;
  if (device >= 0) EGN_CHECK_HIP(hipSetDevice(device));
  Runtime* rt = new Runtime();
  EGN_CHECK_HIP(hipGetDevice(&rt->device));
  const int rc = load(plan, rt);
  if (rc) { free_runtime(rt); return rc; }
  plan->runtime = rt;
  plan->runtime_free = free_runtime;
  // the pieces are on the device: the file's bytes are not needed again (the parsed ops stay)
  std::vector<uint8_t>().swap(plan->file);
  return 0;
}

// native program `which` (egn_plan_program_info's index) of a loaded plan: for egn_program_num_ops / _ticket_ops / _op_info
extern "C" egn_program* egn_plan_native_program(const egn_plan* plan, int program) {
  if (!plan || !plan->runtime) return nullptr;
  const Runtime* rt = static_cast<const Runtime*>(plan->runtime);
  return program >= 0 && program < (int)rt->programs.size() ? rt->programs[program].prog : nullptr;
}

extern "C" int egn_plan_infer(egn_plan* plan, const float* crops, int n, const double* centers, const double* scales,
                              int has_K, double fx, double cx, int alpha_mode, const egn_plan_outputs* out, void* stream) {
  if (!plan || !out) return EGN_E_BADARG;
  if (!plan->runtime) return EGN_E_STATE;
  Runtime* rt = static_cast<Runtime*>(plan->runtime);
  const PlanInfo& h = plan->info;
  const bool pose = h.lifter_out == 96;
  if (n < 1 || !crops || !centers || !scales || !out->local || !out->kpts_2d || !out->kpts_3d || alpha_mode < 0 ||
      alpha_mode > 1 || (pose && (!out->euler || !out->alpha)))
    return EGN_E_BADARG;
  // n as chunks of exported sizes, greedy from the largest; refused before anything is launched
  std::vector<int> chunks;
  uint32_t left = (uint32_t)n;
  for (size_t k = 0; k < rt->sizes.size(); ++k)
    while (left >= rt->sizes[k]) { chunks.push_back((int)k); left -= rt->sizes[k]; }
  if (left) return EGN_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (rt->ran && rt->last_stream != s) EGN_CHECK_HIP(hipStreamWaitEvent(s, rt->ev_done, 0));
  const int local_role = h.decode == 2 ? EGN_PLAN_ROLE_COORDS : EGN_PLAN_ROLE_XY;
  const int J = (int)h.J, D = (int)h.lifter_out;
  float* lin = static_cast<float*>(rt->role_tmp[EGN_PLAN_ROLE_LIFT_IN]);
  float* y = static_cast<float*>(rt->role_tmp[EGN_PLAN_ROLE_LIFT_OUT]);
  size_t at = 0;
  for (int k : chunks) {
    const int c = (int)rt->sizes[k];
    LoadedProgram& hp = rt->programs[rt->hrnet_of[k]];
    LoadedProgram& lp = rt->programs[rt->lifter_of[k]];
    float* local = out->local + at * J * 2;
    for (size_t u = 0; u < hp.desc->user.size(); ++u) {
      const int role = (int)hp.desc->user[u].role;
      void* base = role == EGN_PLAN_ROLE_CROPS ? (void*)(crops + at * h.C * h.H * h.W)
                                               : (role == local_role ? (void*)local : rt->role_tmp[role]);
      int rc = egn_program_bind(hp.prog, 2 + (int)u, base);
      if (rc) return rc;
    }
    int rc = egn_program_run(hp.prog, stream);
    if (rc) return rc;
    double* screen = out->kpts_2d + at * 2 * J;
    rc = egn_keypoints_to_screen_f64(local, c, J, h.mul_x, h.mul_y, centers + at * 2, scales + at * 2, (int)h.W, (int)h.H,
                                     screen, rt->ls[0], rt->ls[1], lin, (int)h.ld_in, stream);
    if (rc) return rc;
    rc = egn_program_bind(lp.prog, 2, lin);
    if (!rc) rc = egn_program_bind(lp.prog, 3, y);
    if (!rc) rc = egn_program_run(lp.prog, stream);
    if (rc) return rc;
    double* pred3d = out->kpts_3d + at * D;
    rc = egn_unnormalize_f64(y, c, D, D, rt->ls[2], rt->ls[3], pred3d, stream);
    if (rc) return rc;
    if (pose) {
      hipLaunchKernelGGL(plan_first_column_kernel, dim3((c + 63) / 64), dim3(64), 0, s, screen, c, 2 * J, rt->kx);
      EGN_CHECK_HIP(hipGetLastError());
      const int amode = (alpha_mode == 0 && has_K) ? 0 : 1;
      rc = egn_pose_solve_f64(pred3d, c, rt->kx, has_K ? fx : 1.0, has_K ? cx : 0.0, amode, out->euler + at * 3,
                              out->alpha + at, stream);
      if (rc) return rc;
    }
    at += (size_t)c;
  }
  EGN_CHECK_HIP(hipEventRecord(rt->ev_done, s));
  rt->last_stream = s;
  rt->ran = true;
  return 0;
}
