// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for the compact
// key-cache geometry KC18 (babble_amd/csrc/geometry.h: 18-bit signed windows
// x 8 from 9-bit sub-tables), compiled from the device's own source with
// plain clang (tests/test_kc_compact.py).  Nothing is loaded into Python.
//
// Per key, one at a time (a table is 67 MB), the table build is replayed lane
// by lane as bvk::build_kc launches it for kw = 18:
//   k_table_bases (L = 9, NSUB = 16), k_table_fill<9, 16, false> (blocks of
//   256 entries, one inversion per block), k_table_pair_kc<18, 9, 8> (blocks
//   of 4096 slots, 16 per thread, prefix products per thread and one inversion
//   per block, the early return of the blocks past the top window's live
//   digits)
// into a buffer pre-filled with a pattern, with guard words on both sides.
// Then every vector of the key runs its key part through
// verify_item_qfirst<18, 8, LAT> for LAT = false (the pipelined lookups: the
// look-ahead request) and LAT = true (the load-then-add loop), with r, s and
// w = s^-1 R exactly as the device pipeline hands them over, against an
// allocation of exactly the table's size.
//
//   argv[1]: keys, one per line      <x 64 hex> <y 64 hex> <status>
//   argv[2]: vectors, one per line   <key index> <r 64 hex> <s 64 hex>
//   argv[3..]: table slots to print
// Output:
//   E <key> <slot> <x> <y>                  the named slots
//   STORES <key> <stores> <max slot> <off-table stores>
//   GUARD <key> <guard words changed> <table words still holding the pattern> <table words>
//   LOOKUP <key> <vector> <max slot any window of either half addresses> <slots in the table>
//   RQ <key> <vector> <LAT> <inf> <x> <y>   R_Q = k1 T + k2 phi(T), affine
// Exit status 1 when a store or lookup left the table or a guard word changed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/verify_core.h"

namespace {

constexpr int W = BV_KC18W, L = BV_KC18L, NSUB = BV_KC18NSUB, NWIN = BV_KC18NWIN;
constexpr uint32_t ENT = BV_KC18ENT, NS = 1u << L;
constexpr uint64_t SUB_U32 = BV_KC18SUB_U32, TABLE_U32 = BV_KC18TABLE_U32, SLOTS = (uint64_t)NWIN * ENT + 1;
constexpr uint32_t FILL = 0xA5A5A5A5u;
constexpr size_t GUARD = 4096;  // words before and after the table
static_assert(W * NWIN >= 129 && 2 * L == W && NSUB == 2 * NWIN, "KC18 geometry");
static_assert(TABLE_U32 * 4 == 67108928ull, "67.1 MB per key");
static_assert(BV_W_IS_CACHED(BV_KC18W) && BV_W_IS_CACHED(BV_KCW) && !BV_W_IS_CACHED(BV_K12W), "cached geometries");

fe fe_hex(const std::string &s) {
  fe a;
  if (s.size() != 64) {
    fprintf(stderr, "bad field element '%s'\n", s.c_str());
    exit(2);
  }
  for (int i = 0; i < 8; i++) a.v[7 - i] = (uint32_t)strtoul(s.substr(8 * i, 8).c_str(), nullptr, 16);
  return a;
}

// 64 hex digits -> 8 dwords holding the 32 big-endian bytes (the r_be / s_be layout)
void be_words_hex(uint32_t *w, const std::string &s) {
  uint8_t b[32];
  for (int i = 0; i < 32; i++) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  memcpy(w, b, 32);
}

std::string hex_words(const uint32_t *w) {
  char buf[65];
  for (int i = 0; i < 8; i++) snprintf(buf + 8 * i, 9, "%08x", w[7 - i]);
  return buf;
}

// v[i] <- v[i]^-1 for n non-zero values with one field inversion (what
// block_inverse does for a block's threads)
void batch_inverse(fe *v, uint32_t n) {
  std::vector<fe> pre(n);
  fe acc;
  fe_set(acc, 1);
  for (uint32_t i = 0; i < n; i++) {
    pre[i] = acc;
    fe_mul(acc, acc, v[i]);
  }
  fe inv;
  fe_inv(inv, acc);
  for (int i = (int)n - 1; i >= 0; i--) {
    fe r;
    fe_mul(r, inv, pre[i]);
    fe_mul(inv, inv, v[i]);
    v[i] = r;
  }
}

// k_table_fill<9, 16, false>, grid (NSUB * 2^L / 256, 1): key 0 of `bases_jac` into `sub`
void fill(const uint32_t *bases_jac, uint32_t *sub) {
  constexpr uint32_t BLOCK = 256, BLOCKS = NSUB * (NS / BLOCK);
  static_assert(((NSUB << L) % BLOCK) == 0, "blocks cover whole keys");
  for (uint32_t c = 0; c < BLOCKS; c++) {
    gej R[BLOCK];
    bool inf[BLOCK];
    fe zi[BLOCK];
    for (uint32_t t = 0; t < BLOCK; t++) {
      const uint32_t f = c * BLOCK + t, j = f >> L, d = f & (NS - 1);
      const uint32_t *bj = bases_jac + (uint64_t)j * 24;
      fe bx, by, bz, Z;
      fe_load(bx, bj);
      fe_load(by, bj + 8);
      fe_load(bz, bj + 16);
      table_point<true>(R[t], inf[t], Z, bx, by, d, L);
      if (!inf[t]) fe_mul(Z, Z, bz);
      zi[t] = Z;
    }
    batch_inverse(zi, BLOCK);
    for (uint32_t t = 0; t < BLOCK; t++) {
      const uint32_t f = c * BLOCK + t, j = f >> L, d = f & (NS - 1);
      table_store(sub + (((uint64_t)j << L) + d) * BV_ENTRY_U32, nullptr, d, R[t], inf[t], zi[t]);
    }
  }
}

struct StoreLog {
  uint64_t stores = 0, max_slot = 0, off_table = 0;
};

// k_table_pair_kc<18, 9, 8>, grid (NWIN * ENT / BV_KCPAIR_ENT, 1), 256 threads
// a block; `table` is what tabs[b] points at
void pair_kc(const uint32_t *sub, uint32_t *table, StoreLog &log) {
  constexpr uint32_t E = BV_KCPAIR_ENT / 256u, CH = ENT / BV_KCPAIR_ENT;
  static_assert(ENT % BV_KCPAIR_ENT == 0, "whole blocks per window");
  std::vector<fe> ps((size_t)E * 256);  // the block's prefix products (pscr)
  for (uint32_t bx = 0; bx < (uint32_t)NWIN * CH; bx++) {
    const uint32_t j = bx / CH, c = bx % CH;
    const int live_bits = 128 - W * (int)j;
    if (live_bits < W - 1 && (uint64_t)BV_KCPAIR_ENT * c > (1ull << live_bits) + 1) continue;
    const uint32_t *s_lo = sub + (uint64_t)(2 * j) * NS * BV_ENTRY_U32, *s_hi = s_lo + (uint64_t)NS * BV_ENTRY_U32;
    fe q[256];
    for (uint32_t t = 0; t < 256; t++) {
      fe acc;
      fe_set(acc, 1);
      for (uint32_t e = 0; e < E; e++) {
        const uint32_t d = k12_digit(BV_KCPAIR_ENT * c + 256u * e + t, ENT), lo = d & (NS - 1), hi = d >> L;
        fe x1, y1, x2, y2, H;
        pair_load(s_lo, s_hi, lo, hi, x1, y1, x2, y2);
        pair_denominator(H, pair_kind(lo, hi), x1, x2);
        ps[(size_t)e * 256 + t] = acc;
        fe_mul(acc, acc, H);
      }
      q[t] = acc;
    }
    batch_inverse(q, 256);
    for (uint32_t t = 0; t < 256; t++) {
      fe qq = q[t];
      for (int e = (int)E - 1; e >= 0; e--) {
        const uint32_t d = k12_digit(BV_KCPAIR_ENT * c + 256u * e + t, ENT), lo = d & (NS - 1), hi = d >> L;
        const int kind = pair_kind(lo, hi);
        fe x1, y1, x2, y2, H, Hinv;
        pair_load(s_lo, s_hi, lo, hi, x1, y1, x2, y2);
        pair_denominator(H, kind, x1, x2);
        fe_mul(Hinv, qq, ps[(size_t)e * 256 + t]);
        fe_mul(qq, qq, H);
        const uint64_t slot = (uint64_t)j * ENT + d;
        log.stores++;
        if (slot > log.max_slot) log.max_slot = slot;
        if (slot >= SLOTS) {  // never written: counted, and the run fails
          log.off_table++;
          continue;
        }
        pair_store(table + slot * BV_ENTRY_U32, nullptr, kind, x1, y1, x2, y2, Hinv);
      }
    }
  }
}

// the largest slot the windows of one half address (the digits next_digit
// hands key_table_add, look-ahead request included)
uint64_t max_lookup_slot(const uint32_t k[4]) {
  uint32_t kk[4] = {k[0], k[1], k[2], k[3]}, carry = 0;
  uint64_t m = 0;
  for (int j = 0; j < NWIN; j++) {
    bool dneg;
    const uint32_t d = next_digit<W, 4, true>(kk, carry, dneg);
    const uint64_t slot = (uint64_t)j * ENT + d;
    if (slot > m) m = slot;
  }
  if (carry) m = ~0ull;  // a carry out of the top window would be a lost digit
  return m;
}

struct Vec {
  uint32_t key;
  std::string r, s;
};

template <bool LAT>
void key_part(uint32_t b, uint32_t vi, const Vec &v, const uint32_t *table) {
  alignas(16) uint32_t r_be[8], s_be[8], w[8], rq[RG_WORDS];
  be_words_hex(r_be, v.r);
  be_words_hex(s_be, v.s);
  sinv_thread(0, 1, 1, 1, s_be, nullptr, w);  // k_sinv for a one-item batch
  const uint32_t item_key[1] = {0};
  const uint8_t kstatus[1] = {KS_OK};
  const uint64_t key_tabs[1] = {(uint64_t)(uintptr_t)table};
  for (int i = 0; i < RG_WORDS; i++) rq[i] = FILL;
  verify_item_qfirst<W, NWIN, LAT>(0, 1, item_key, r_be, s_be, nullptr, kstatus, w, nullptr, key_tabs, rq);
  gexz R;
  bool inf;
  rg_load(rq, 1, 0, R, inf);
  fe x, y, zi;
  fe_set(x, 0);
  fe_set(y, 0);
  if (!inf) {
    fe_inv(zi, R.ZZ);
    fe_mul(x, R.X, zi);
    fe_inv(zi, R.ZZZ);
    fe_mul(y, R.Y, zi);
    fe_canon(x);
    fe_canon(y);
  }
  printf("RQ %u %u %d %u %s %s\n", b, vi, LAT ? 1 : 0, rq[32], hex_words(x.v).c_str(), hex_words(y.v).c_str());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s keys.txt vectors.txt [slot ...]\n", argv[0]);
    return 2;
  }
  std::ifstream fk(argv[1]), fv(argv[2]);
  std::vector<uint32_t> bxy;
  std::vector<uint8_t> bstatus;
  std::string line;
  while (std::getline(fk, line)) {
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
  std::vector<Vec> vecs;
  while (std::getline(fv, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    Vec v;
    in >> v.key >> v.r >> v.s;
    if (v.r.size() != 64 || v.s.size() != 64) {
      fprintf(stderr, "bad vector '%s'\n", line.c_str());
      return 2;
    }
    vecs.push_back(v);
  }
  const uint32_t nb = (uint32_t)bstatus.size();
  int bad = 0;
  std::vector<uint32_t> bases((size_t)NSUB * 24), sub((size_t)SUB_U32);
  for (uint32_t b = 0; b < nb; b++) {
    std::vector<uint32_t> buf(GUARD + TABLE_U32 + GUARD, FILL);
    uint32_t *table = buf.data() + GUARD;
    StoreLog log;
    if (bstatus[b] == KS_OK) {  // every build kernel returns at once for another status
      std::fill(bases.begin(), bases.end(), FILL);
      std::fill(sub.begin(), sub.end(), FILL);
      table_bases_one<true>(0, bxy.data() + 16 * (size_t)b, bases.data(), L, NSUB);
      fill(bases.data(), sub.data());
      pair_kc(sub.data(), table, log);
    }
    uint64_t guard_changed = 0, pattern = 0;
    for (size_t i = 0; i < GUARD; i++) guard_changed += (buf[i] != FILL) + (buf[GUARD + TABLE_U32 + i] != FILL);
    for (uint64_t i = 0; i < TABLE_U32; i++) pattern += table[i] == FILL;
    printf("STORES %u %llu %llu %llu\n", b, (unsigned long long)log.stores, (unsigned long long)log.max_slot,
           (unsigned long long)log.off_table);
    printf("GUARD %u %llu %llu %llu\n", b, (unsigned long long)guard_changed, (unsigned long long)pattern,
           (unsigned long long)TABLE_U32);
    bad |= guard_changed != 0 || log.off_table != 0;
    for (int a = 3; a < argc; a++) {
      const uint64_t slot = strtoull(argv[a], nullptr, 10);
      if (slot >= SLOTS) {
        fprintf(stderr, "slot %llu is not in the table\n", (unsigned long long)slot);
        return 2;
      }
      const uint32_t *e = table + slot * BV_ENTRY_U32;
      printf("E %u %llu %s %s\n", b, (unsigned long long)slot, hex_words(e).c_str(), hex_words(e + 8).c_str());
    }
    if (bstatus[b] != KS_OK) continue;
    // the lookups read an allocation of exactly the table's size
    std::vector<uint32_t> exact(table, table + TABLE_U32);
    for (uint32_t vi = 0; vi < (uint32_t)vecs.size(); vi++) {
      if (vecs[vi].key != b) continue;
      {  // the halves as verify_item_qfirst forms them, for the addresses alone
        alignas(16) uint32_t r_be[8], s_be[8], w[8];
        be_words_hex(r_be, vecs[vi].r);
        be_words_hex(s_be, vecs[vi].s);
        sinv_thread(0, 1, 1, 1, s_be, nullptr, w);
        sc ws, rs, u2;
        for (int k = 0; k < 8; k++) ws.v[k] = w[k];
        sc_load_be_words(rs, r_be);
        sc_mont(u2, rs, ws);
        uint32_t k1[4], k2[4], signs;
        glv_split(k1, k2, signs, u2);
        const uint64_t m1 = max_lookup_slot(k1), m2 = max_lookup_slot(k2), m = m1 > m2 ? m1 : m2;
        printf("LOOKUP %u %u %llu %llu\n", b, vi, (unsigned long long)m, (unsigned long long)SLOTS);
        if (m >= SLOTS) {
          bad = 1;
          continue;  // the lookups would leave the table: not run
        }
      }
      key_part<false>(b, vi, vecs[vi], exact.data());
      key_part<true>(b, vi, vecs[vi], exact.data());
    }
    fflush(stdout);
  }
  return bad;
}
