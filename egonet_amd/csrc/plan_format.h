// plan_format.h -- the parsed form of an inference plan file (.egnplan) shared by its host-only parser / validator
// (plan.cpp) and its loader / runner (plan_run.hip).  DESIGN 3.23 has the byte layout; egonet_amd/plan.py writes it.
//
//   file     := "EGNPLAN\0"  u32 format_version  section*                       (all integers little-endian)
//   section  := u32 tag  u64 length  payload[length]  u32 crc32(payload)        tags: 1 HEAD, 2 PIEC, 3 PROG, 4 END
//   order    := HEAD  PROG*  PIEC  END     (everything that is validated field by field lies before the bulk)
//
// Nothing here includes HIP: plan.cpp compiles with a plain host compiler (tests/plan_fuzz_main.cpp links it alone).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#define EGN_PLAN_FORMAT_VERSION 1u
enum { EGN_PLAN_SEC_HEAD = 1, EGN_PLAN_SEC_PIEC = 2, EGN_PLAN_SEC_PROG = 3, EGN_PLAN_SEC_END = 4 };
// roles of a program's user slots (slot 2 + index)
enum { EGN_PLAN_ROLE_CROPS = 1, EGN_PLAN_ROLE_MAPS = 2, EGN_PLAN_ROLE_COORDS = 3, EGN_PLAN_ROLE_XY = 4, EGN_PLAN_ROLE_MAX = 5,
       EGN_PLAN_ROLE_IDX = 6, EGN_PLAN_ROLE_LIFT_IN = 7, EGN_PLAN_ROLE_LIFT_OUT = 8 };
// op kinds: the values of OpKind in program.hip
enum { EGN_PLAN_OP_CONV = 1, EGN_PLAN_OP_FUSE = 2, EGN_PLAN_OP_NCHW2NHWC = 3, EGN_PLAN_OP_NHWC2NCHW = 4, EGN_PLAN_OP_RAMPS = 5,
       EGN_PLAN_OP_DECODE = 6, EGN_PLAN_OP_FORK = 7, EGN_PLAN_OP_JOIN = 8, EGN_PLAN_OP_PIXSHUF = 9, EGN_PLAN_OP_PWPAIR = 10,
       EGN_PLAN_OP_CONVPAIR = 11, EGN_PLAN_OP_CONVH = 12, EGN_PLAN_OP_CONVH2 = 13, EGN_PLAN_OP_CONVHX = 14 };

struct PlanRef { int32_t slot; int64_t off; };

struct PlanOp {
  uint32_t kind = 0, lane = 0, signal = 0;
  std::vector<uint32_t> waits;      // indices of earlier, signalling ops of the same program
  std::vector<int32_t> ints;        // the integer arguments of the egn_program_add_* call, in its order
  std::vector<PlanRef> refs;        // its egn_ref arguments, in its order (a fuse op: y, then the terms)
  double flops = 0, bytes = 0;
  std::string tag;
};

struct PlanPiece { uint64_t nbytes = 0; size_t file_off = 0; };    // the bytes lie at file[file_off]
struct PlanPlace { uint32_t piece = 0; uint64_t off = 0; };        // piece -> byte offset in the weights slot
struct PlanSlot { uint32_t role = 0; uint64_t nbytes = 0; };

struct PlanProgram {
  uint32_t type = 0;                // 0 HRNet, 1 lifter
  uint32_t n = 0;                   // crops per run
  uint64_t arena_bytes = 0, weight_bytes = 0;
  std::vector<PlanPlace> places;
  std::vector<PlanSlot> user;
  std::vector<PlanOp> ops;
};

struct PlanInfo {
  uint32_t format_version = 0, lib_version = 0, fingerprint = 0;
  std::string arch, switches;
  uint32_t precision = 0;           // 0 f32, 1 f16, 2 f16s2, 3 f16x
  uint32_t head_type = 0;           // 0 coordinates, 1 heatmap
  uint32_t decode = 0;              // 0 hard, 1 soft, 2 coords
  uint32_t J = 0, C = 0, H = 0, W = 0, map_h = 0, map_w = 0;
  double mul_x = 0, mul_y = 0;
  uint32_t lifter_in = 0, lifter_out = 0, ld_in = 0;
  std::vector<double> ls[4];        // mean_in, std_in [lifter_in]; mean_out, std_out [lifter_out]
  std::vector<uint32_t> sizes;      // the exported batch sizes, as given
};

struct egn_plan {
  PlanInfo info;
  std::vector<uint8_t> file;        // the whole file (the pieces are read from it; released by egn_plan_load)
  std::vector<PlanPiece> pieces;
  std::vector<PlanProgram> programs;
  // the loaded form belongs to plan_run.hip; egn_plan_close calls `runtime_free` (this file's owner links no HIP)
  void* runtime = nullptr;
  void (*runtime_free)(void*) = nullptr;
};

// CRC-32 (IEEE 802.3, zlib's), slicing by 8
static inline uint32_t egn_plan_crc32(const void* data, size_t n, uint32_t crc = 0) {
  struct Tables {
    uint32_t T[8][256];
    Tables() {
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        T[0][i] = c;
      }
      for (uint32_t i = 0; i < 256; ++i)
        for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xff];
    }
  };
  static const Tables tables;
  const uint32_t (*T)[256] = tables.T;
  const uint8_t* p = static_cast<const uint8_t*>(data);
  crc = ~crc;
  while (n >= 8) {
    uint32_t w[2];            // (little-endian hosts, like the file)
    memcpy(w, p, 8);
    const uint32_t lo = crc ^ w[0], hi = w[1];
    crc = T[7][lo & 0xff] ^ T[6][(lo >> 8) & 0xff] ^ T[5][(lo >> 16) & 0xff] ^ T[4][lo >> 24] ^ T[3][hi & 0xff] ^
          T[2][(hi >> 8) & 0xff] ^ T[1][(hi >> 16) & 0xff] ^ T[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) crc = T[0][(crc ^ *p++) & 0xff] ^ (crc >> 8);
  return ~crc;
}

// a * b, saturating at UINT64_MAX (extents of tensors a hostile file describes)
static inline uint64_t egn_plan_mul(uint64_t a, uint64_t b) {
  uint64_t r;
  return __builtin_mul_overflow(a, b, &r) ? UINT64_MAX : r;
}
