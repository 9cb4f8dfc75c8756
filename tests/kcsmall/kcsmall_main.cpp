// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for the table leaves of
// k_small's warm tree, compiled from the device's own source with plain clang
// (tests/test_kc_small.py).  Nothing is loaded into Python.
//
// k_small's lanes 10 .. 10 + 2 KNWIN - 1 of wave 0 each load one key-cache
// table entry through small_table_leaf<KW, KNWIN> (verify_core.h): the lane ->
// (GLV half, window) mapping and the signed recoding that addresses the
// table.  This program runs THAT function for every table lane of one item,
// for the KC18 geometry <18, 8> and for KC <22, 6>, against a table buffer of
// exactly the geometry's size (BV_KC18TABLE_U32 / BV_KCTABLE_U32 words)
// pre-filled with a pattern, between guard words, in which only the slots the
// caller names hold points.  Per vector:
//   * the device glv_split of u2 gives k1, k2 and the signs;
//   * each lane's slot is first predicted with next_digit (the bulk lookups'
//     recoding) and the leaf is run only when that slot is inside the table;
//   * the leaf's own slot must equal the prediction, a non-zero leaf must have
//     read a stored slot, and the top window's slot must not pass the digits a
//     half below 2^128 can have (KC18: 7 ENT + 4);
//   * the leaves are summed as the kernel's lanes do (gexz_sum_ge_lat for the
//     affine pairs 2i, 2i + 1, gexz_add_lat above them) and the affine sum is
//     printed: it is u2 Q when the stored slots held |d| 2^(W j) Q.
//
//   argv[1]: vectors, one per line
//            <18|22> <u2, 64 hex> <n> then n times: <slot> <x 64 hex> <y 64 hex>
// Output:
//   LEAF <vector> <lane> <slot> <zero> <stored>
//   SUM <vector> <inf> <x> <y>
//   GUARD <geometry> <guard words changed> <table words not holding the pattern after the run>
// Exit status 1 when a read would have left the table, a leaf's slot was not
// the predicted one, a non-zero leaf read a slot that was not stored, the top
// window's bound was passed or a guard word changed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/verify_core.h"

namespace {

constexpr uint32_t FILL = 0xA5A5A5A5u;
constexpr size_t GUARD = 4096;  // words before and after the table

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

struct Stored {
  uint64_t slot;
  fe x, y;
};
struct Vec {
  int geom;
  uint32_t index;
  std::string u2;
  std::vector<Stored> stored;
};

template <int KW, int KNWIN>
int run(const std::vector<Vec> &vecs) {
  constexpr uint32_t ENT = 1u << (KW - 1);
  constexpr uint64_t SLOTS = (uint64_t)KNWIN * ENT + 1, TABLE_U32 = SLOTS * BV_ENTRY_U32;
  static_assert(TABLE_U32 == (KW == BV_KC18W ? BV_KC18TABLE_U32 : BV_KCTABLE_U32), "exactly the table's size");
  // the largest digit of the top window: the live bits of a 128-bit half there, plus the carry
  constexpr uint64_t TOP_MAX = (uint64_t)(KNWIN - 1) * ENT + (1ull << (128 - KW * (KNWIN - 1)));
  static_assert(KW != BV_KC18W || TOP_MAX == 7ull * BV_KC18ENT + 4, "KC18: the top window's digit is at most 4");
  bool any = false;
  for (const Vec &v : vecs) any |= v.geom == KW;
  if (!any) return 0;
  std::vector<uint32_t> buf(GUARD + TABLE_U32 + GUARD, FILL);
  uint32_t *table = buf.data() + GUARD;
  int bad = 0;
  for (const Vec &v : vecs) {
    if (v.geom != KW) continue;
    std::set<uint64_t> stored;
    for (const Stored &s : v.stored) {
      if (s.slot >= SLOTS) {
        fprintf(stderr, "vector %u: slot %llu is not in the table\n", v.index, (unsigned long long)s.slot);
        return 2;
      }
      memcpy(table + s.slot * BV_ENTRY_U32, s.x.v, 32);
      memcpy(table + s.slot * BV_ENTRY_U32 + 8, s.y.v, 32);
      stored.insert(s.slot);
    }
    sc u2;
    const fe u = fe_hex(v.u2);
    for (int k = 0; k < 8; k++) u2.v[k] = u.v[k];
    uint32_t k12[8], signs;
    glv_split(k12, k12 + 4, signs, u2);
    // the slots the bulk lookups' recoding gives, per half and window
    uint64_t want[2 * KNWIN];
    bool inside = true;
    for (int h = 0; h < 2; h++) {
      uint32_t kk[4] = {k12[4 * h], k12[4 * h + 1], k12[4 * h + 2], k12[4 * h + 3]}, carry = 0;
      for (int j = 0; j < KNWIN; j++) {
        bool dneg;
        const uint32_t d = next_digit<KW, 4, true>(kk, carry, dneg);
        want[h * KNWIN + j] = (uint64_t)j * ENT + d;
        inside &= want[h * KNWIN + j] < SLOTS;
      }
      if (carry) inside = false;  // a carry out of the top window would be a lost digit
    }
    if (!inside) {
      fprintf(stderr, "vector %u: a leaf would read outside the table (not run)\n", v.index);
      bad = 1;
    } else {
      fe x[2 * KNWIN], y[2 * KNWIN];
      bool zero[2 * KNWIN];
      for (uint32_t q = 0; q < 2u * KNWIN; q++) {
        const uint64_t slot = small_table_leaf<KW, KNWIN>(x[q], y[q], zero[q], table, k12, signs, q);
        const bool is_stored = stored.count(slot) != 0;
        printf("LEAF %u %u %llu %d %d\n", v.index, BV_GNWIN + q, (unsigned long long)slot, zero[q] ? 1 : 0,
               is_stored ? 1 : 0);
        bad |= slot != want[q] || (!zero[q] && !is_stored);
        if (q % KNWIN == KNWIN - 1) bad |= slot > TOP_MAX;
      }
      // the sum tree's per-lane point functions: affine pairs, then XYZZ sums
      gexz R;
      bool inf = true;
      fe_set(R.X, 0);
      fe_set(R.Y, 0);
      fe_set(R.ZZ, 0);
      fe_set(R.ZZZ, 0);
      for (uint32_t q = 0; q < 2u * KNWIN; q += 2) {
        gexz nd;
        bool ninf;
        gexz_sum_ge_lat(nd, ninf, x[q], y[q], zero[q], x[q + 1], y[q + 1], zero[q + 1]);
        gexz_add_lat(R, inf, nd, ninf);
      }
      fe ax, ay, zi;
      fe_set(ax, 0);
      fe_set(ay, 0);
      if (!inf) {
        fe_inv(zi, R.ZZ);
        fe_mul(ax, R.X, zi);
        fe_inv(zi, R.ZZZ);
        fe_mul(ay, R.Y, zi);
        fe_canon(ax);
        fe_canon(ay);
      }
      printf("SUM %u %d %s %s\n", v.index, inf ? 1 : 0, hex_words(ax.v).c_str(), hex_words(ay.v).c_str());
    }
    for (const Stored &s : v.stored)  // the pattern again, for the next vector
      for (int k = 0; k < BV_ENTRY_U32; k++) table[s.slot * BV_ENTRY_U32 + k] = FILL;
  }
  uint64_t guard_changed = 0, touched = 0;
  for (size_t i = 0; i < GUARD; i++) guard_changed += (buf[i] != FILL) + (buf[GUARD + TABLE_U32 + i] != FILL);
  for (uint64_t i = 0; i < TABLE_U32; i++) touched += table[i] != FILL;
  printf("GUARD %d %llu %llu\n", KW, (unsigned long long)guard_changed, (unsigned long long)touched);
  return bad | (guard_changed != 0) | (touched != 0);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s vectors.txt\n", argv[0]);
    return 2;
  }
  std::ifstream fv(argv[1]);
  std::vector<Vec> vecs;
  std::string line;
  while (std::getline(fv, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Vec v;
    size_t n = 0;
    in >> v.geom >> v.u2 >> n;
    v.index = (uint32_t)vecs.size();
    for (size_t i = 0; i < n; i++) {
      Stored s;
      std::string x, y;
      in >> s.slot >> x >> y;
      s.x = fe_hex(x);
      s.y = fe_hex(y);
      v.stored.push_back(s);
    }
    if (!in || (v.geom != BV_KC18W && v.geom != BV_KCW) || v.u2.size() != 64) {
      fprintf(stderr, "bad vector '%s'\n", line.substr(0, 100).c_str());
      return 2;
    }
    vecs.push_back(v);
  }
  const int a = run<BV_KC18W, BV_KC18NWIN>(vecs);
  const int b = run<BV_KCW, BV_KCNWIN>(vecs);
  fflush(stdout);
  return a > b ? a : b;
}
