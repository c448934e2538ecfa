// plan.cpp -- host-only parser and validator of inference plan files (.egnplan, plan_format.h), and
// egn_box_to_crop_f64.  No HIP: this file also compiles alone with a plain host compiler (tests/plan_fuzz_main.cpp
// parses mutated files under AddressSanitizer / UBSan).
//
// egn_plan_open returns success only for a file every later step can trust: the loader (plan_run.hip) replays its ops
// into egn_programs and launches them, so every index, count, offset and extent is checked HERE, against the bytes that
// remain before anything is allocated and against the slot it points into before anything can be launched.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/egonet_hip.h"
#include "plan_format.h"

#pragma STDC FP_CONTRACT OFF

namespace {

struct Reader {
  const uint8_t* p;
  size_t n, at = 0;
  bool short_read = false;
  Reader(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
  size_t left() const { return n - at; }
  bool take(void* dst, size_t k) {
    if (short_read || k > left()) { short_read = true; memset(dst, 0, k); return false; }
    memcpy(dst, p + at, k);
    at += k;
    return true;
  }
  // (the build targets are little-endian: the file's integers are read as they lie)
  uint32_t u32() { uint32_t v; take(&v, 4); return v; }
  int32_t i32() { int32_t v; take(&v, 4); return v; }
  uint64_t u64() { uint64_t v; take(&v, 8); return v; }
  double f64() { double v; take(&v, 8); return v; }
  // a count of elements of at least `each` bytes: refused unless the bytes are there
  bool count(uint32_t* out, size_t each, uint32_t cap) {
    const uint32_t c = u32();
    if (short_read || c > cap || (uint64_t)c * each > left()) return false;
    *out = c;
    return true;
  }
  bool str(std::string* s, uint32_t cap) {
    uint32_t len;
    if (!count(&len, 1, cap)) return false;
    s->assign(reinterpret_cast<const char*>(p + at), len);
    at += len;
    return true;
  }
};

const uint64_t kMaxBytes = (uint64_t)1 << 40;     // no slot of a plan is larger
const uint64_t F32 = 4;

inline uint64_t mul(uint64_t a, uint64_t b) { return egn_plan_mul(a, b); }
inline uint64_t mul(uint64_t a, uint64_t b, uint64_t c) { return mul(mul(a, b), c); }
inline uint64_t mul(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return mul(mul(a, b), mul(c, d)); }
inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

int parse_head(Reader& r, PlanInfo& h) {
  h.lib_version = r.u32();
  h.fingerprint = r.u32();
  if (!r.str(&h.arch, 64)) return EGN_E_PLAN_COUNT;
  h.precision = r.u32(); h.head_type = r.u32(); h.decode = r.u32();
  h.J = r.u32(); h.C = r.u32(); h.H = r.u32(); h.W = r.u32(); h.map_h = r.u32(); h.map_w = r.u32();
  h.mul_x = r.f64(); h.mul_y = r.f64();
  h.lifter_in = r.u32(); h.lifter_out = r.u32(); h.ld_in = r.u32();
  for (int k = 0; k < 4; ++k) {
    uint32_t c;
    if (!r.count(&c, 8, 1u << 20)) return EGN_E_PLAN_COUNT;
    h.ls[k].resize(c);
    r.take(h.ls[k].data(), (size_t)c * 8);
  }
  uint32_t ns;
  if (!r.count(&ns, 4, 64)) return EGN_E_PLAN_COUNT;
  h.sizes.resize(ns);
  for (uint32_t k = 0; k < ns; ++k) h.sizes[k] = r.u32();
  if (!r.str(&h.switches, 1u << 16)) return EGN_E_PLAN_COUNT;
  if (r.short_read) return EGN_E_PLAN_COUNT;
  if (r.left()) return EGN_E_PLAN_FORMAT;
  if (h.lib_version != (uint32_t)egn_version()) return EGN_E_PLAN_VERSION;
  if (h.fingerprint != egn_conv_table_fingerprint()) return EGN_E_PLAN_FINGERPRINT;
  const auto in = [](uint32_t v, uint32_t lo, uint32_t hi) { return v >= lo && v <= hi; };
  if (h.precision > 3 || h.head_type > 1 || h.decode > 2 || !in(h.J, 1, 4096) || !in(h.C, 1, 4096) || !in(h.H, 1, 65536) ||
      !in(h.W, 1, 65536) || !in(h.map_h, 1, 65536) || !in(h.map_w, 1, 65536) || !(h.mul_x > 0) || !(h.mul_y > 0) ||
      !isfinite(h.mul_x) || !isfinite(h.mul_y) || h.lifter_in != 2 * h.J || !in(h.lifter_out, 1, 1u << 20) ||
      h.ld_in < h.lifter_in || h.ld_in % 4 || h.ld_in > h.lifter_in + 3 || ns < 1)
    return EGN_E_PLAN_FORMAT;
  if (h.ls[0].size() != h.lifter_in || h.ls[1].size() != h.lifter_in || h.ls[2].size() != h.lifter_out ||
      h.ls[3].size() != h.lifter_out)
    return EGN_E_PLAN_FORMAT;
  for (uint32_t s : h.sizes)
    if (!in(s, 1, 65535)) return EGN_E_PLAN_FORMAT;
  return 0;
}

int parse_pieces(Reader& r, size_t payload_off, std::vector<PlanPiece>& pieces) {
  uint32_t c;
  if (!r.count(&c, 8, 1u << 24)) return EGN_E_PLAN_COUNT;
  pieces.resize(c);
  for (uint32_t k = 0; k < c; ++k) {
    const uint64_t nb = r.u64();
    if (r.short_read || nb > r.left()) return EGN_E_PLAN_COUNT;
    if (nb == 0 || nb % 4) return EGN_E_PLAN_FORMAT;
    pieces[k].nbytes = nb;
    pieces[k].file_off = payload_off + r.at;
    r.at += (size_t)nb;
  }
  return r.left() ? EGN_E_PLAN_FORMAT : 0;
}

// ---- the ops -----------------------------------------------------------------------------------------------------------
struct Check {
  const std::vector<uint64_t>& slot_bytes;
  int rc = 0;
  explicit Check(const std::vector<uint64_t>& s) : slot_bytes(s) {}
  void fail(int code) { if (!rc) rc = code; }
  // a dimension: 1 .. 2^24
  uint64_t dim(int32_t v, int32_t lo = 1, int32_t hi = 1 << 24) {
    if (v < lo || v > hi) { fail(EGN_E_PLAN_FORMAT); return 1; }
    return (uint64_t)v;
  }
  // `extent` bytes from the ref lie inside its slot
  void ref(const PlanRef& r, uint64_t extent, bool nullable = false) {
    if (r.slot < 0) {
      if (!nullable || r.slot != -1) fail(EGN_E_PLAN_SLOT);
      return;
    }
    if ((size_t)r.slot >= slot_bytes.size()) { fail(EGN_E_PLAN_SLOT); return; }
    const uint64_t size = slot_bytes[r.slot];
    if (r.off < 0 || r.off % 16 || (uint64_t)r.off > size || extent > size - (uint64_t)r.off) fail(EGN_E_PLAN_REF);
  }
};

// numbers of (refs, ints) an op kind carries; -1: by the op (fuse)
bool arity(uint32_t kind, int* nrefs, int* nints) {
  switch (kind) {
    case EGN_PLAN_OP_CONV: *nrefs = 6; *nints = 14; return true;
    case EGN_PLAN_OP_FUSE: *nrefs = -1; *nints = -1; return true;
    case EGN_PLAN_OP_NCHW2NHWC: case EGN_PLAN_OP_NHWC2NCHW: *nrefs = 2; *nints = 5; return true;
    case EGN_PLAN_OP_RAMPS: *nrefs = 1; *nints = 5; return true;
    case EGN_PLAN_OP_DECODE: *nrefs = 4; *nints = 5; return true;
    case EGN_PLAN_OP_FORK: case EGN_PLAN_OP_JOIN: *nrefs = 0; *nints = 0; return true;
    case EGN_PLAN_OP_PIXSHUF: *nrefs = 2; *nints = 6; return true;
    case EGN_PLAN_OP_PWPAIR: *nrefs = 8; *nints = 2; return true;
    case EGN_PLAN_OP_CONVPAIR: *nrefs = 12; *nints = 13; return true;
    case EGN_PLAN_OP_CONVH: *nrefs = 6; *nints = 6; return true;
    case EGN_PLAN_OP_CONVH2: *nrefs = 5; *nints = 6; return true;
    case EGN_PLAN_OP_CONVHX: *nrefs = 6; *nints = 7; return true;
  }
  return false;
}

// x, w, scale, shift, res, y of a 3x3 / pad 1 convolution with unpadded channel strides; `wbytes`: its filter
void check_conv3x3(Check& c, const PlanRef* r, bool has_res_ref, const int32_t* i, int stride, uint64_t wbytes) {
  const uint64_t N = c.dim(i[0]), H = c.dim(i[1]), W = c.dim(i[2]), Cin = c.dim(i[3]), Cout = c.dim(i[4]);
  const uint64_t Ho = stride == 2 ? (H - 1) / 2 + 1 : H, Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
  const uint64_t ybytes = mul(N, Ho, Wo, Cout * F32);
  int k = 0;
  c.ref(r[k++], mul(N, H, W, Cin * F32));
  c.ref(r[k++], wbytes);
  c.ref(r[k++], round_up(Cout, 16) * F32);
  c.ref(r[k++], round_up(Cout, 16) * F32);
  if (has_res_ref) c.ref(r[k++], ybytes, true);
  c.ref(r[k++], ybytes);
}

int check_op(const PlanOp& op, const std::vector<uint64_t>& slot_bytes) {
  Check c(slot_bytes);
  const int32_t* i = op.ints.data();
  const PlanRef* r = op.refs.data();
  switch (op.kind) {
    case EGN_PLAN_OP_CONV: {
      const uint64_t N = c.dim(i[0]), H = c.dim(i[1]), W = c.dim(i[2]), Cin = c.dim(i[3]), cs_in = c.dim(i[4]),
                     Cout = c.dim(i[5]), cs_out = c.dim(i[6]), KH = c.dim(i[7], 1, 64), KW = c.dim(i[8], 1, 64),
                     stride = c.dim(i[9], 1, 8), pad = c.dim(i[10], 0, 32);
      c.dim(i[12], 0, 1);
      c.dim(i[13], 0, 1 << 16);
      if (c.rc) return c.rc;
      if (cs_in < Cin || H + 2 * pad < KH || W + 2 * pad < KW || (!i[12] && cs_out < Cout)) return EGN_E_PLAN_FORMAT;
      const uint64_t Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
      const uint64_t ybytes = i[12] ? mul(N, Cout, Ho, Wo * F32) : mul(N, Ho, Wo, cs_out * F32);
      c.ref(r[0], mul(N, H, W, cs_in * F32));
      c.ref(r[1], mul(Cout, Cin, KH, KW * F32));        // (the least of the layouts; the loader knows cfg's own)
      c.ref(r[2], round_up(Cout, 16) * F32);
      c.ref(r[3], round_up(Cout, 16) * F32);
      c.ref(r[4], mul(N, Ho, Wo, cs_out * F32), true);
      c.ref(r[5], ybytes);
      break;
    }
    case EGN_PLAN_OP_CONVPAIR:
      for (int h = 0; h < 2; ++h) {
        const int32_t* q = i + 6 * h;
        check_conv3x3(c, r + 6 * h, true, q, 1, mul(c.dim(q[3]), c.dim(q[4]), 48 * F32));
      }
      break;
    case EGN_PLAN_OP_CONVH:
    case EGN_PLAN_OP_CONVH2: {
      const uint64_t Cin = c.dim(i[3]), Cout = c.dim(i[4]);
      check_conv3x3(c, r, op.kind == EGN_PLAN_OP_CONVH, i, op.kind == EGN_PLAN_OP_CONVH ? 1 : 2,
                    mul((Cout + 15) / 16, (Cin + 47) / 48, 14 * 32 * 16 * 2));
      break;
    }
    case EGN_PLAN_OP_CONVHX: {
      const uint64_t stride = c.dim(i[6], 1, 2);
      check_conv3x3(c, r, true, i, (int)stride, mul(c.dim(i[3]), c.dim(i[4]), 9 * 2));
      break;
    }
    case EGN_PLAN_OP_FUSE: {
      if (op.ints.size() < 8) return EGN_E_PLAN_FORMAT;
      const uint64_t N = c.dim(i[0]), H = c.dim(i[1]), W = c.dim(i[2]), C = c.dim(i[3]), cs = c.dim(i[4]), nt = c.dim(i[5], 1, 4);
      if (c.rc) return c.rc;
      if (op.ints.size() != 7 + nt || op.refs.size() != 1 + nt || cs < C) return EGN_E_PLAN_FORMAT;
      c.ref(r[0], mul(N, H, W, cs * F32));
      for (uint64_t k = 0; k < nt; ++k) {
        const uint64_t s = c.dim(i[6 + k], 0, 16);
        if (!(H >> s) || !(W >> s)) return EGN_E_PLAN_FORMAT;
        c.ref(r[1 + k], mul(N, H >> s, W >> s, cs * F32));
      }
      break;
    }
    case EGN_PLAN_OP_NCHW2NHWC:
    case EGN_PLAN_OP_NHWC2NCHW: {
      const uint64_t N = c.dim(i[0]), C = c.dim(i[1]), H = c.dim(i[2]), W = c.dim(i[3]), cs = c.dim(i[4]);
      if (cs < C) return EGN_E_PLAN_FORMAT;
      const bool to_nhwc = op.kind == EGN_PLAN_OP_NCHW2NHWC;
      c.ref(r[to_nhwc ? 0 : 1], mul(N, C, H, W * F32));
      c.ref(r[to_nhwc ? 1 : 0], mul(N, H, W, cs * F32));
      break;
    }
    case EGN_PLAN_OP_PIXSHUF: {
      const uint64_t N = c.dim(i[0]), C = c.dim(i[1]), H = c.dim(i[2]), W = c.dim(i[3]), cs = c.dim(i[4]), up = c.dim(i[5], 1, 16);
      if (cs < C * up * up) return EGN_E_PLAN_FORMAT;
      c.ref(r[0], mul(N, H, W, cs * F32));
      c.ref(r[1], mul(mul(N, C), mul(H, up), mul(W, up), F32));
      break;
    }
    case EGN_PLAN_OP_RAMPS: {
      const uint64_t N = c.dim(i[0]), H = c.dim(i[1]), W = c.dim(i[2]), cs = c.dim(i[3]), c0 = c.dim(i[4], 0);
      if (c0 + 2 > cs) return EGN_E_PLAN_FORMAT;
      c.ref(r[0], mul(N, H, W, cs * F32));
      break;
    }
    case EGN_PLAN_OP_DECODE: {
      const uint64_t N = c.dim(i[0]), K = c.dim(i[1]), H = c.dim(i[2]), W = c.dim(i[3]);
      c.dim(i[4], 0, 2);
      c.ref(r[0], mul(N, K, H, W * F32));
      c.ref(r[1], mul(N, K, 2 * F32));
      c.ref(r[2], mul(N, K, F32));
      c.ref(r[3], mul(N, K, F32), true);
      break;
    }
    case EGN_PLAN_OP_PWPAIR: {
      const uint64_t M = c.dim(i[0]);
      c.dim(i[1], 0, 1);
      c.ref(r[0], mul(M, 64 * F32));
      c.ref(r[1], mul(M, 256 * F32), true);
      c.ref(r[2], 256 * 64 * F32);
      c.ref(r[3], 256 * F32);
      c.ref(r[4], 64 * 256 * F32, true);
      c.ref(r[5], 64 * F32, true);
      c.ref(r[6], mul(M, 256 * F32));
      c.ref(r[7], mul(M, 64 * F32), true);
      break;
    }
    case EGN_PLAN_OP_FORK:
    case EGN_PLAN_OP_JOIN:
      break;
    default:
      return EGN_E_PLAN_OP;
  }
  return c.rc;
}

int parse_program(Reader& r, const PlanInfo& h, PlanProgram& g) {
  g.type = r.u32();
  g.n = r.u32();
  g.arena_bytes = r.u64();
  g.weight_bytes = r.u64();
  if (r.short_read) return EGN_E_PLAN_COUNT;
  if (g.type > 1 || g.n < 1 || g.n > 65535 || g.arena_bytes > kMaxBytes || g.weight_bytes > kMaxBytes) return EGN_E_PLAN_FORMAT;
  const uint64_t wsize = g.weight_bytes < 256 ? 256 : g.weight_bytes;
  uint32_t np;
  if (!r.count(&np, 12, 1u << 24)) return EGN_E_PLAN_COUNT;
  g.places.resize(np);
  for (auto& pl : g.places) {
    pl.piece = r.u32();
    pl.off = r.u64();
    if (pl.off % 16 || pl.off > wsize) return EGN_E_PLAN_REF;      // (the piece's length: check_places, behind PIEC)
  }
  uint32_t nu;
  if (!r.count(&nu, 12, 62)) return EGN_E_PLAN_COUNT;
  g.user.resize(nu);
  std::vector<uint64_t> slot_bytes = {g.arena_bytes < 256 ? 256 : g.arena_bytes, wsize};
  uint32_t seen = 0;
  const uint64_t n = g.n, J = h.J;
  for (auto& u : g.user) {
    u.role = r.u32();
    u.nbytes = r.u64();
    uint64_t want = 0;
    switch (u.role) {
      case EGN_PLAN_ROLE_CROPS: want = mul(mul(n, h.C), mul(h.H, h.W), F32); break;
      case EGN_PLAN_ROLE_MAPS: want = u.nbytes; break;
      case EGN_PLAN_ROLE_COORDS: case EGN_PLAN_ROLE_XY: want = n * J * 2 * F32; break;
      case EGN_PLAN_ROLE_MAX: case EGN_PLAN_ROLE_IDX: want = n * J * F32; break;
      case EGN_PLAN_ROLE_LIFT_IN: want = n * h.ld_in * F32; break;
      case EGN_PLAN_ROLE_LIFT_OUT: want = n * h.lifter_out * F32; break;
      default: return EGN_E_PLAN_FORMAT;
    }
    if (u.nbytes != want || u.nbytes == 0 || u.nbytes > kMaxBytes || (seen >> u.role) & 1) return EGN_E_PLAN_FORMAT;
    seen |= 1u << u.role;
    slot_bytes.push_back(u.nbytes);
  }
  if (r.short_read) return EGN_E_PLAN_COUNT;
  const auto has = [&](int role) { return (seen >> role) & 1; };
  if (g.type == 0) {
    const int local = h.decode == 2 ? EGN_PLAN_ROLE_COORDS : EGN_PLAN_ROLE_XY;
    if (nu < 2 || g.user[0].role != EGN_PLAN_ROLE_CROPS || !has(local) || has(EGN_PLAN_ROLE_LIFT_IN) ||
        has(EGN_PLAN_ROLE_LIFT_OUT))
      return EGN_E_PLAN_FORMAT;
  } else if (nu != 2 || g.user[0].role != EGN_PLAN_ROLE_LIFT_IN || g.user[1].role != EGN_PLAN_ROLE_LIFT_OUT) {
    return EGN_E_PLAN_FORMAT;
  }
  uint32_t nops;
  if (!r.count(&nops, 44, 1u << 24)) return EGN_E_PLAN_COUNT;
  g.ops.resize(nops);
  for (uint32_t k = 0; k < nops; ++k) {
    PlanOp& op = g.ops[k];
    op.kind = r.u32(); op.lane = r.u32(); op.signal = r.u32();
    uint32_t c;
    if (!r.count(&c, 4, 64)) return EGN_E_PLAN_COUNT;
    op.waits.resize(c);
    for (auto& w : op.waits) w = r.u32();
    if (!r.count(&c, 4, 32)) return EGN_E_PLAN_COUNT;
    op.ints.resize(c);
    for (auto& v : op.ints) v = r.i32();
    if (!r.count(&c, 12, 16)) return EGN_E_PLAN_COUNT;
    op.refs.resize(c);
    for (auto& q : op.refs) { q.slot = r.i32(); q.off = (int64_t)r.u64(); }
    op.flops = r.f64();
    op.bytes = r.f64();
    if (!r.str(&op.tag, 4096)) return EGN_E_PLAN_COUNT;
    if (r.short_read) return EGN_E_PLAN_COUNT;
    int nrefs, nints;
    if (!arity(op.kind, &nrefs, &nints)) return EGN_E_PLAN_OP;
    if ((nrefs >= 0 && (int)op.refs.size() != nrefs) || (nints >= 0 && (int)op.ints.size() != nints)) return EGN_E_PLAN_FORMAT;
    const bool barrier = op.kind == EGN_PLAN_OP_FORK || op.kind == EGN_PLAN_OP_JOIN;
    if (op.lane > 3 || op.signal > 1 || (barrier && (op.lane || op.signal || !op.waits.empty()))) return EGN_E_PLAN_FORMAT;
    for (uint32_t w : op.waits)
      if (w >= k || !g.ops[w].signal) return EGN_E_PLAN_WAIT;
    const int rc = check_op(op, slot_bytes);
    if (rc) return rc;
  }
  return r.left() ? EGN_E_PLAN_FORMAT : 0;
}

// the pieces section lies behind the programs: where each program puts which piece is checked once their sizes are known
int check_places(const egn_plan& plan) {
  for (const PlanProgram& g : plan.programs) {
    const uint64_t wsize = g.weight_bytes < 256 ? 256 : g.weight_bytes;
    for (const PlanPlace& pl : g.places) {
      if (pl.piece >= plan.pieces.size()) return EGN_E_PLAN_FORMAT;
      if (plan.pieces[pl.piece].nbytes > wsize - pl.off) return EGN_E_PLAN_REF;
    }
  }
  return 0;
}

struct Bytes {
  const uint8_t* p;
  size_t n;
  const uint8_t* data() const { return p; }
  size_t size() const { return n; }
};

int parse_file(egn_plan& plan, const Bytes& f) {
  static const char magic[8] = {'E', 'G', 'N', 'P', 'L', 'A', 'N', 0};
  if (f.size() < 12) return EGN_E_PLAN_TRUNCATED;
  if (memcmp(f.data(), magic, 8)) return EGN_E_PLAN_MAGIC;
  memcpy(&plan.info.format_version, f.data() + 8, 4);
  if (plan.info.format_version != EGN_PLAN_FORMAT_VERSION) return EGN_E_PLAN_VERSION;
  size_t at = 12;
  int stage = 0;          // sections seen: 0 none, 1 HEAD (then any number of PROG), 2 PIEC, 3 END
  while (stage < 3) {
    if (f.size() - at < 12) return EGN_E_PLAN_TRUNCATED;
    uint32_t tag;
    uint64_t len;
    memcpy(&tag, f.data() + at, 4);
    memcpy(&len, f.data() + at + 4, 8);
    at += 12;
    if (len > f.size() - at || f.size() - at - len < 4) return EGN_E_PLAN_TRUNCATED;
    uint32_t crc;
    memcpy(&crc, f.data() + at + len, 4);
    if (crc != egn_plan_crc32(f.data() + at, (size_t)len)) return EGN_E_PLAN_CRC;
    Reader r(f.data() + at, (size_t)len);
    int rc = EGN_E_PLAN_FORMAT;
    if (tag == EGN_PLAN_SEC_HEAD && stage == 0) {
      rc = parse_head(r, plan.info);
      stage = 1;
    } else if (tag == EGN_PLAN_SEC_PROG && stage == 1) {
      if (plan.programs.size() >= 256) return EGN_E_PLAN_FORMAT;
      plan.programs.emplace_back();
      rc = parse_program(r, plan.info, plan.programs.back());
    } else if (tag == EGN_PLAN_SEC_PIEC && stage == 1) {
      rc = parse_pieces(r, at, plan.pieces);
      if (!rc) rc = check_places(plan);
      stage = 2;
    } else if (tag == EGN_PLAN_SEC_END && stage == 2) {
      rc = len ? EGN_E_PLAN_FORMAT : 0;
      stage = 3;
    }
    if (rc) return rc;
    at += (size_t)len + 4;
  }
  if (at != f.size()) return EGN_E_PLAN_FORMAT;
  // every exported size has its HRNet and its lifter program
  for (uint32_t s : plan.info.sizes)
    for (uint32_t type = 0; type < 2; ++type) {
      bool found = false;
      for (const PlanProgram& g : plan.programs) found = found || (g.type == type && g.n == s);
      if (!found) return EGN_E_PLAN_FORMAT;
    }
  return 0;
}

void put(std::vector<uint8_t>& out, const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  out.insert(out.end(), b, b + n);
}
void put32(std::vector<uint8_t>& out, uint32_t v) { put(out, &v, 4); }

}  // namespace

// Parse an in-memory file (the plan takes the bytes over).  What egn_plan_open does after reading, and what the fuzz
// program calls directly.
extern "C" int egn_plan_parse(const void* bytes, size_t n, egn_plan** out) {
  if (!out || (!bytes && n)) return EGN_E_BADARG;
  *out = nullptr;
  egn_plan* plan = new egn_plan();
  const uint8_t* b = static_cast<const uint8_t*>(bytes);
  const int rc = parse_file(*plan, Bytes{b, n});
  if (rc) { delete plan; return rc; }
  plan->file.assign(b, b + n);        // (the pieces are offsets into it)
  *out = plan;
  return 0;
}

extern "C" int egn_plan_open(const char* path, egn_plan** out) {
  if (!out || !path) return EGN_E_BADARG;
  *out = nullptr;
  FILE* fp = fopen(path, "rb");
  if (!fp) return EGN_E_PLAN_IO;
  egn_plan* plan = new egn_plan();
  int rc = 0;
  if (fseek(fp, 0, SEEK_END) != 0) rc = EGN_E_PLAN_IO;
  const long size = rc ? 0 : ftell(fp);
  if (!rc && (size < 0 || fseek(fp, 0, SEEK_SET) != 0)) rc = EGN_E_PLAN_IO;
  if (!rc) {
    plan->file.resize((size_t)size);
    if (size && fread(plan->file.data(), 1, (size_t)size, fp) != (size_t)size) rc = EGN_E_PLAN_IO;
  }
  fclose(fp);
  if (!rc) rc = parse_file(*plan, Bytes{plan->file.data(), plan->file.size()});
  if (rc) { delete plan; return rc; }
  *out = plan;
  return 0;
}

extern "C" void egn_plan_close(egn_plan* plan) {
  if (!plan) return;
  if (plan->runtime && plan->runtime_free) plan->runtime_free(plan->runtime);
  delete plan;
}

extern "C" int egn_plan_get_info(const egn_plan* plan, egn_plan_info* info) {
  if (!plan || !info) return EGN_E_BADARG;
  const PlanInfo& h = plan->info;
  memset(info, 0, sizeof(*info));
  info->format_version = (int)h.format_version; info->lib_version = (int)h.lib_version;
  info->fingerprint = h.fingerprint;
  snprintf(info->arch, sizeof(info->arch), "%s", h.arch.c_str());
  info->precision = (int)h.precision; info->head_type = (int)h.head_type; info->decode = (int)h.decode;
  info->J = (int)h.J; info->C = (int)h.C; info->H = (int)h.H; info->W = (int)h.W;
  info->map_h = (int)h.map_h; info->map_w = (int)h.map_w;
  info->mul_x = h.mul_x; info->mul_y = h.mul_y;
  info->lifter_in = (int)h.lifter_in; info->lifter_out = (int)h.lifter_out; info->ld_in = (int)h.ld_in;
  info->n_sizes = (int)h.sizes.size();
  for (size_t k = 0; k < h.sizes.size() && k < 64; ++k) info->sizes[k] = (int)h.sizes[k];
  info->n_pieces = (int)plan->pieces.size();
  info->n_programs = (int)plan->programs.size();
  info->loaded = plan->runtime != nullptr;
  return 0;
}

extern "C" int egn_plan_get_text(const egn_plan* plan, int what, char* buf, int len) {
  if (!plan || !buf || len < 1 || what < 0 || what > 1) return EGN_E_BADARG;
  snprintf(buf, (size_t)len, "%s", (what == 0 ? plan->info.arch : plan->info.switches).c_str());
  return 0;
}

extern "C" int egn_plan_get_stats(const egn_plan* plan, int which, double* out, int n) {
  if (!plan || !out || which < 0 || which > 3 || n != (int)plan->info.ls[which].size()) return EGN_E_BADARG;
  memcpy(out, plan->info.ls[which].data(), (size_t)n * 8);
  return 0;
}

extern "C" int egn_plan_program_info(const egn_plan* plan, int program, int* type, int* n, long long* arena_bytes,
                                     long long* weight_bytes, int* n_ops, int* ops_with_waits, int* kinds, int kinds_len) {
  if (!plan || program < 0 || program >= (int)plan->programs.size()) return EGN_E_BADARG;
  const PlanProgram& g = plan->programs[program];
  if (type) *type = (int)g.type;
  if (n) *n = (int)g.n;
  if (arena_bytes) *arena_bytes = (long long)g.arena_bytes;
  if (weight_bytes) *weight_bytes = (long long)g.weight_bytes;
  if (n_ops) *n_ops = (int)g.ops.size();
  int nw = 0;
  for (const PlanOp& op : g.ops) nw += !op.waits.empty();
  if (ops_with_waits) *ops_with_waits = nw;
  if (kinds) {
    if (kinds_len < (int)g.ops.size()) return EGN_E_BADARG;
    for (size_t k = 0; k < g.ops.size(); ++k) kinds[k] = (int)g.ops[k].kind;
  }
  return 0;
}

// The canonical record of an op, serialised again from the parsed form (the bytes egonet_amd.plan.encode_op gives for
// the logged call): kind, lane, signal, waits, ints, refs, flops, bytes, tag.
extern "C" int egn_plan_op_record(const egn_plan* plan, int program, int op_index, void* buf, int len, int* used) {
  if (!plan || program < 0 || program >= (int)plan->programs.size() || !used) return EGN_E_BADARG;
  const PlanProgram& g = plan->programs[program];
  if (op_index < 0 || op_index >= (int)g.ops.size()) return EGN_E_BADARG;
  const PlanOp& op = g.ops[op_index];
  std::vector<uint8_t> out;
  put32(out, op.kind); put32(out, op.lane); put32(out, op.signal);
  put32(out, (uint32_t)op.waits.size());
  for (uint32_t w : op.waits) put32(out, w);
  put32(out, (uint32_t)op.ints.size());
  for (int32_t v : op.ints) put(out, &v, 4);
  put32(out, (uint32_t)op.refs.size());
  for (const PlanRef& q : op.refs) { put(out, &q.slot, 4); put(out, &q.off, 8); }
  put(out, &op.flops, 8);
  put(out, &op.bytes, 8);
  put32(out, (uint32_t)op.tag.size());
  put(out, op.tag.data(), op.tag.size());
  *used = (int)out.size();
  if (!buf || len < (int)out.size()) return buf ? EGN_E_BADARG : 0;
  memcpy(buf, out.data(), out.size());
  return 0;
}

// modify_bbox (enlarge about the centre, then grow one side to the target aspect ratio) and the forward affine of the
// crop front end, in the reference's order of operations: the float64 bits of common/img_proc.py::modify_bbox and
// common/crop_gpu.py::forward_affines.
extern "C" int egn_box_to_crop_f64(const double* boxes, int n, double target_ar, double enlarge, int out_w, int out_h,
                                   double* center, double* scale, double* M) {
  if (n < 0 || (n && (!boxes || !center || !scale)) || out_w < 1 || out_h < 1) return EGN_E_BADARG;
  for (int k = 0; k < n; ++k) {
    const double l0 = boxes[4 * k], t0 = boxes[4 * k + 1], r0 = boxes[4 * k + 2], b0 = boxes[4 * k + 3];
    const double ecx = (l0 + r0) / 2, ecy = (t0 + b0) / 2;
    const double hw = 0.5 * (r0 - l0) * enlarge, hh = 0.5 * (b0 - t0) * enlarge;
    double left = ecx - hw, top = ecy - hh, right = ecx + hw, bottom = ecy + hh;
    const double width = right - left, height = bottom - top;
    const double cx = (left + right) / 2, cy = (top + bottom) / 2;
    if (height / width > target_ar) {
      const double half = 0.5 * height * (1 / target_ar);
      left = cx - half; right = cx + half;
    } else {
      const double half = 0.5 * width * target_ar;
      top = cy - half; bottom = cy + half;
    }
    center[2 * k] = cx; center[2 * k + 1] = cy;
    const double s0 = (right - left) / 200.0, s1 = (bottom - top) / 200.0;
    scale[2 * k] = s0; scale[2 * k + 1] = s1;
    if (M) {
      const double w = (double)out_w, h = (double)out_h;
      const double kk = w / (s0 * 200.0);
      double* m = M + 6 * k;
      m[0] = kk; m[1] = 0.0; m[2] = w * 0.5 - kk * cx;
      m[3] = 0.0; m[4] = kk; m[5] = h * 0.5 - kk * cy;
    }
  }
  return 0;
}
