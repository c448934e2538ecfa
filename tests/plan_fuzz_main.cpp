// plan_fuzz_main.cpp -- a stand-alone program (its own main) around the plan parser of egonet_amd/csrc/plan.cpp, built by
// tests/test_plan_cpu.py with -fsanitize=address,undefined and nothing else of the library:
//
//   plan_fuzz <valid plan file> <mutations> <seed>
//
// applies seeded single-byte and 4-byte mutations to the file, one at a time, repairs the CRC of the section a mutation
// fell into for two mutants out of three (so the fields behind the CRC check are reached), parses every mutant with
// egn_plan_parse and closes the ones that are accepted.  Exit 0 if nothing crashed; the sanitizers abort otherwise.  The
// two library functions the parser compares the header with are defined here: they answer what the valid file holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../egonet_amd/csrc/plan_format.h"
#include "../include/egonet_hip.h"

static uint32_t g_version = 0, g_fingerprint = 0;
extern "C" int egn_version(void) { return (int)g_version; }
extern "C" unsigned egn_conv_table_fingerprint(void) { return g_fingerprint; }

struct Section { size_t payload, length; };

static uint64_t g_state;
static uint32_t rnd() {      // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: plan_fuzz <plan> <mutations> <seed>\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "plan_fuzz: cannot read %s\n", argv[1]); return 2; }
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) file.insert(file.end(), buf, buf + k);
  fclose(fp);
  const long count = atol(argv[2]);
  g_state = strtoull(argv[3], nullptr, 10);
  if (file.size() < 32) { fprintf(stderr, "plan_fuzz: %s is too short\n", argv[1]); return 2; }
  memcpy(&g_version, file.data() + 24, 4);          // HEAD payload: u32 egn_version, u32 fingerprint
  memcpy(&g_fingerprint, file.data() + 28, 4);
  egn_plan* plan = nullptr;
  int rc = egn_plan_parse(file.data(), file.size(), &plan);
  if (rc) { fprintf(stderr, "plan_fuzz: the unmutated file is refused (code %d)\n", rc); return 3; }
  egn_plan_close(plan);
  std::vector<Section> sections;
  std::vector<size_t> meta;        // every byte outside the pieces' payload: where most mutations go
  for (size_t k = 0; k < 12; ++k) meta.push_back(k);
  for (size_t at = 12; at + 12 <= file.size();) {
    uint32_t tag;
    uint64_t len;
    memcpy(&tag, file.data() + at, 4);
    memcpy(&len, file.data() + at + 4, 8);
    sections.push_back({at + 12, (size_t)len});
    const size_t end = at + 12 + (size_t)len + 4;
    for (size_t k = at; k < end; ++k)
      if (tag != EGN_PLAN_SEC_PIEC || k < at + 12 + 64 || k >= end - 4) meta.push_back(k);
    at = end;
  }
  static const uint32_t words[] = {0u, 1u, 0xffffffffu, 0x80000000u, 0x7fffffffu, 99u, 0x10000u, 0xfffffff0u};
  long accepted = 0, codes[32] = {0};
  for (long it = 0; it < count; ++it) {
    const bool anywhere = rnd() % 16 == 0;
    const size_t pos = anywhere ? rnd() % file.size() : meta[rnd() % meta.size()];
    uint8_t saved[4 + 4] = {0};
    const size_t width = (rnd() & 1) && pos + 4 <= file.size() ? 4 : 1;
    memcpy(saved, file.data() + pos, width);
    if (width == 1) {
      file[pos] = (uint8_t)((rnd() & 3) == 0 ? file[pos] ^ (1u << (rnd() % 8)) : rnd());
    } else {
      const uint32_t pick = rnd() % 12;
      const uint32_t w = pick < 8 ? words[pick] : rnd();
      memcpy(file.data() + pos, &w, 4);
    }
    // the section whose payload was hit gets its CRC repaired, two times out of three
    size_t crc_at = 0;
    if (rnd() % 3)
      for (const Section& s : sections)
        if (pos + width > s.payload && pos < s.payload + s.length && s.payload + s.length + 4 <= file.size()) {
          crc_at = s.payload + s.length;
          memcpy(saved + 4, file.data() + crc_at, 4);
          const uint32_t crc = egn_plan_crc32(file.data() + s.payload, s.length);
          memcpy(file.data() + crc_at, &crc, 4);
          break;
        }
    plan = nullptr;
    rc = egn_plan_parse(file.data(), file.size(), &plan);
    if (rc == 0) {
      ++accepted;
      egn_plan_info info;
      egn_plan_get_info(plan, &info);
      for (int g = 0; g < info.n_programs; ++g) {        // read back what was accepted
        int n_ops = 0, used = 0;
        egn_plan_program_info(plan, g, nullptr, nullptr, nullptr, nullptr, &n_ops, nullptr, nullptr, 0);
        for (int k = 0; k < n_ops; ++k) egn_plan_op_record(plan, g, k, nullptr, 0, &used);
      }
      egn_plan_close(plan);
    } else if (rc < 0 && rc > -32) {
      ++codes[-rc];
    }
    if (crc_at) memcpy(file.data() + crc_at, saved + 4, 4);
    memcpy(file.data() + pos, saved, width);
  }
  printf("plan_fuzz: %ld mutants, %ld accepted; refused by code:", count, accepted);
  for (int k = 1; k < 32; ++k)
    if (codes[k]) printf(" %d:%ld", -k, codes[k]);
  printf("\n");
  return 0;
}
