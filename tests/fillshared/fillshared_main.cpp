// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for the K12 sub-table
// fill from shared multiples (babble_amd/csrc/verify_core.h BV_FILL_SHARED),
// compiled from the device's own source with plain clang
// (tests/test_fill_shared.py).  The kernels' bodies are replayed lane by lane
// on the host — k_table_fill<6, 22> (the per-entry double-and-add),
// k_fill_multiples + k_table_fill_shared, and k_table_pair<12, 6, 11> on
// either's sub-tables — with a plain field inversion where the kernels share
// one per block.  Reads keys from the file given as argv[1], one per line:
//     <x 64 hex> <y 64 hex> <status>
// (status != 0: a key the kernels skip), builds each key's K12 table both
// ways into buffers pre-filled with the same pattern, and prints
//     SUB <live sub-table entries compared> <differing>
//     DEAD <dead sub-table words the new fill left untouched> <of>
//     TABLE <table words compared> <differing>
//     E <key> <slot> <x> <y>      for the slots named in argv[2..]
// Exit status 1 if anything differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/verify_core.h"

namespace {

constexpr int W = BV_K12W, L = BV_K12L, NSUB = BV_K12NSUB, NWIN = BV_K12NWIN;
constexpr uint32_t ENT = BV_K12ENT, NS = 1u << L, ODD = BV_FS_ODD_LIVE(W, L);
constexpr uint32_t LIVE = fs_live<L, NSUB, ODD>();
constexpr uint64_t SUB_U32 = BV_K12SUB_U32, HALF_U32 = BV_K12HALF_U32, TABLE_U32 = BV_K12TABLE_U32;
constexpr uint32_t FILL = 0xA5A5A5A5u;

fe fe_hex(const std::string &s) {
  fe a;
  if (s.size() != 64) {
    fprintf(stderr, "bad field element '%s'\n", s.c_str());
    exit(2);
  }
  for (int i = 0; i < 8; i++) a.v[7 - i] = (uint32_t)strtoul(s.substr(8 * i, 8).c_str(), nullptr, 16);
  return a;
}

std::string hex_words(const uint32_t *w) {
  char buf[65];
  for (int i = 0; i < 8; i++) snprintf(buf + 8 * i, 9, "%08x", w[7 - i]);
  return buf;
}

// k_table_fill<6, 22, false, 64, false>, block (j, b)
void fill_old(uint32_t b, const uint32_t *bases_jac, const uint8_t *bstatus, uint32_t *sub) {
  if (bstatus[b] != KS_OK) return;
  for (uint32_t j = 0; j < (uint32_t)NSUB; j++)
    for (uint32_t d = 0; d < NS; d++) {
      const uint32_t *bj = bases_jac + ((uint64_t)b * NSUB + j) * 24;
      fe bx, by, bz, Z, zi;
      fe_load(bx, bj);
      fe_load(by, bj + 8);
      fe_load(bz, bj + 16);
      gej R;
      bool inf;
      table_point<false>(R, inf, Z, bx, by, d, L);
      if (!inf) fe_mul(Z, Z, bz);
      fe_inv(zi, Z);
      table_store(sub + (uint64_t)b * SUB_U32 + (((uint64_t)j << L) + d) * BV_ENTRY_U32, nullptr, d, R, inf, zi);
    }
}

// k_fill_multiples<22> and k_table_fill_shared<12, 6, 22>, every lane of their grids
void fill_new(uint32_t b, const uint32_t *bases_jac, const uint8_t *bstatus, uint32_t *mult, uint32_t *sub) {
  if (bstatus[b] != KS_OK) return;
  const uint32_t mblocks = (BV_FS_MULTS * NSUB + 63) / 64, fblocks = (LIVE + 63) / 64;
  for (uint32_t u = 0; u < 64 * mblocks; u++)
    if (u < (uint32_t)BV_FS_MULTS * NSUB) fill_multiple_one<NSUB>(b, u, bases_jac, mult);
  for (uint32_t f = 0; f < 64 * fblocks; f++) {
    if (f >= LIVE) continue;
    uint32_t k, x;
    fill_shared_slot<L, NSUB, ODD>(f, k, x);
    gej R;
    bool inf;
    fe Z, zi;
    fill_shared_point<NSUB>(R, inf, Z, b, k, x, mult);
    if (!inf) {
      fe bz;
      fe_load(bz, bases_jac + ((uint64_t)b * NSUB + k) * 24 + 16);
      fe_mul(Z, Z, bz);
    }
    fe_inv(zi, Z);
    table_store(sub + (uint64_t)b * SUB_U32 + (((uint64_t)k << L) + x) * BV_ENTRY_U32, nullptr, x, R, inf, zi);
  }
}

// k_table_pair<12, 6, 11>, block (j, b)
void pair(uint32_t b, const uint32_t *sub, const uint8_t *bstatus, uint32_t *table) {
  if (bstatus[b] != KS_OK) return;
  constexpr uint32_t E = ENT / 256u;
  for (uint32_t j = 0; j < (uint32_t)NWIN; j++) {
    const int live_bits = 128 - W * (int)j;
    const uint32_t e_live = live_bits >= W - 1 ? E : ((1u << live_bits) + 1u + 255u) / 256u;
    const uint32_t *s_lo = sub + ((uint64_t)b * 2 * NWIN + 2 * j) * NS * BV_ENTRY_U32, *s_hi = s_lo + NS * BV_ENTRY_U32;
    uint32_t *base = table + (uint64_t)b * 2 * HALF_U32 + (uint64_t)j * ENT * BV_ENTRY_U32;
    for (uint32_t s = 0; s < 256 * e_live; s++) {
      const uint32_t d = k12_digit(s, ENT), lo = d & (NS - 1), hi = d >> L;
      const int kind = pair_kind(lo, hi);
      fe x1, y1, x2, y2, H, Hinv;
      pair_load(s_lo, s_hi, lo, hi, x1, y1, x2, y2);
      pair_denominator(H, kind, x1, x2);
      fe_inv(Hinv, H);
      uint32_t *entry = base + (uint64_t)d * BV_ENTRY_U32;
      pair_store(entry, entry + HALF_U32, kind, x1, y1, x2, y2, Hinv);
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s keys.txt [slot ...]\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  std::vector<uint32_t> bxy;
  std::vector<uint8_t> bstatus;
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string x, y;
    int st;
    in >> x >> y >> st;
    fe fx = fe_hex(x), fy = fe_hex(y);
    bxy.insert(bxy.end(), fx.v, fx.v + 8);
    bxy.insert(bxy.end(), fy.v, fy.v + 8);
    bstatus.push_back((uint8_t)st);
  }
  const uint32_t nb = (uint32_t)bstatus.size();
  std::vector<uint32_t> bases((size_t)nb * NSUB * 24, FILL), mult((size_t)nb * fs_mult_u32<NSUB>(), FILL);
  std::vector<uint32_t> sub_a((size_t)nb * SUB_U32, FILL), sub_b(sub_a), tab_a((size_t)nb * TABLE_U32, FILL), tab_b(tab_a);
  for (uint32_t b = 0; b < nb; b++) {
    if (bstatus[b] == KS_OK) table_bases_one<false>(b, bxy.data(), bases.data(), L, NSUB);
    fill_old(b, bases.data(), bstatus.data(), sub_a.data());
    fill_new(b, bases.data(), bstatus.data(), mult.data(), sub_b.data());
    pair(b, sub_a.data(), bstatus.data(), tab_a.data());
    pair(b, sub_b.data(), bstatus.data(), tab_b.data());
  }
  uint64_t live = 0, live_bad = 0, dead = 0, dead_kept = 0, tab_bad = 0;
  for (uint32_t b = 0; b < nb; b++)
    for (uint32_t k = 0; k < (uint32_t)NSUB; k++)
      for (uint32_t x = 0; x < NS; x++) {
        const size_t o = (size_t)b * SUB_U32 + (((size_t)k << L) + x) * BV_ENTRY_U32;
        if (bstatus[b] == KS_OK && ((k & 1u) == 0 || x < ODD)) {
          live++;
          live_bad += memcmp(&sub_a[o], &sub_b[o], 64) != 0;
        } else {
          for (int i = 0; i < BV_ENTRY_U32; i++) {
            dead++;
            dead_kept += sub_b[o + i] == FILL;
          }
        }
      }
  for (size_t i = 0; i < tab_a.size(); i++) tab_bad += tab_a[i] != tab_b[i];
  printf("SUB %llu %llu\n", (unsigned long long)live, (unsigned long long)live_bad);
  printf("DEAD %llu %llu\n", (unsigned long long)dead_kept, (unsigned long long)dead);
  printf("TABLE %llu %llu\n", (unsigned long long)tab_a.size(), (unsigned long long)tab_bad);
  for (int a = 2; a < argc; a++) {
    const uint64_t slot = strtoull(argv[a], nullptr, 10);
    for (uint32_t b = 0; b < nb; b++) {
      const uint32_t *e = &tab_b[(size_t)b * TABLE_U32 + slot * BV_ENTRY_U32];
      printf("E %u %llu %s %s %s\n", b, (unsigned long long)slot, hex_words(e).c_str(), hex_words(e + 8).c_str(),
             hex_words(e + HALF_U32).c_str());
    }
  }
  return live_bad || tab_bad || dead_kept != dead ? 1 : 0;
}
