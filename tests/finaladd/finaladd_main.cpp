// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for two rewrites in the
// throughput verify loops, compiled from the device's own source
// (babble_amd/csrc/point.h, verify_core.h) with plain clang, optionally under
// AddressSanitizer + UBSan (tests/test_point_final_add.py):
//   * gexz_add_ge(..., xz_only): the last addition before final_check without
//     Y3 / ZZZ3, against the full addition;
//   * key_table_add with the GLV half's sign folded into each entry's sign
//     (and the lookups one window ahead when BV_LOOKUP_PIPE), against the
//     earlier form kept below as key_table_add_ref: negate the accumulator,
//     add, negate back; load, then add.
// Reads cases from the file given as argv[1], prints one result line per
// case; the test compares the two forms and checks both against Python
// integers.  Key-table geometry here: 4-bit signed windows x 33 (132 bits).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/verify_core.h"

namespace {

constexpr int TW = 4, TN = 33;
constexpr uint32_t TENT = 1u << (TW - 1);
constexpr uint64_t THALF_U32 = ((uint64_t)TN * TENT + 1) * BV_ENTRY_U32;

fe fe_hex(const std::string &s) {  // 64 hex digits, big-endian
  fe a;
  if (s.size() != 64) {
    fprintf(stderr, "bad field element '%s'\n", s.c_str());
    exit(2);
  }
  for (int i = 0; i < 8; i++) a.v[7 - i] = (uint32_t)strtoul(s.substr(8 * i, 8).c_str(), nullptr, 16);
  return a;
}

std::string hex_fe(fe a) {  // canonical
  fe_canon(a);
  char buf[65];
  for (int i = 0; i < 8; i++) snprintf(buf + 8 * i, 9, "%08x", a.v[7 - i]);
  return buf;
}

struct Acc {
  gexz R;
  bool inf;
};

Acc read_acc(std::istringstream &in) {
  std::string x, y, zz, zzz;
  int inf;
  in >> x >> y >> zz >> zzz >> inf;
  Acc a;
  a.R.X = fe_hex(x);
  a.R.Y = fe_hex(y);
  a.R.ZZ = fe_hex(zz);
  a.R.ZZZ = fe_hex(zzz);
  a.inf = inf != 0;
  return a;
}

void print_xz(const Acc &a, const fe &r) {
  std::cout << hex_fe(a.R.X) << ' ' << hex_fe(a.R.ZZ) << ' ' << (a.inf ? 1 : 0) << ' '
            << (final_check(a.R, a.inf, r) ? 1 : 0);
}

void print_yzzz(const Acc &a) { std::cout << ' ' << hex_fe(a.R.Y) << ' ' << hex_fe(a.R.ZZZ); }

// key_table_add as it was before the sign fold and the lookup pipeline
template <int W, int NWIN>
void key_table_add_ref(gexz &R, bool &inf, const uint32_t *tab, uint32_t k[4], bool neg, bool phi, bool from_inf) {
  constexpr uint32_t ENT = 1u << (W - 1);
  if (neg) fe_neg(R.Y, R.Y);
  uint32_t carry = 0;
  for (int j = 0; j < NWIN; j++) {
    uint32_t d = (k[0] & ((1u << W) - 1u)) + carry;
    k[0] = (k[0] >> W) | (k[1] << (32 - W));
    k[1] = (k[1] >> W) | (k[2] << (32 - W));
    k[2] = (k[2] >> W) | (k[3] << (32 - W));
    k[3] >>= W;
    bool dneg = false;
    carry = d > ENT ? 1u : 0u;
    if (carry) {
      d = (1u << W) - d;
      dneg = true;
    }
    const uint32_t *e = tab + ((uint64_t)j * ENT + d) * BV_ENTRY_U32;
    fe x, y;
    fe_load(x, e);
    fe_load(y, e + 8);
    if (phi) {
      fe beta;
      fe_load(beta, FE_BETA);
      fe_mul(x, x, beta);
    }
    fe_cneg_canon(y, dneg);
    if (from_inf && j == 1 && !inf) {
      if (d != 0) gexz_add_ge_aff<false>(R, inf, x, y);
      continue;
    }
    if (d != 0) gexz_add_ge(R, inf, x, y);
  }
  if (neg) fe_neg(R.Y, R.Y);
}

void limbs4(uint32_t k[4], const fe &a) {
  for (int c = 0; c < 4; c++) k[c] = a.v[c];
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  // exactly sized: an address off the table is a sanitizer report
  std::vector<uint32_t> table;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "T") {  // next table entry: x y
      std::string x, y;
      in >> x >> y;
      const fe a = fe_hex(x), b = fe_hex(y);
      for (int i = 0; i < 8; i++) table.push_back(a.v[i]);
      for (int i = 0; i < 8; i++) table.push_back(b.v[i]);
    } else if (cmd == "add") {  // acc x2 y2 r: one addition, full and trimmed
      Acc full = read_acc(in);
      std::string x2, y2, r;
      in >> x2 >> y2 >> r;
      Acc trim = full;
      const fe x = fe_hex(x2), y = fe_hex(y2), rr = fe_hex(r);
      gexz_add_ge(full.R, full.inf, x, y);
      gexz_add_ge(trim.R, trim.inf, x, y, true);
      print_xz(trim, rr);
      std::cout << ' ';
      print_xz(full, rr);
      print_yzzz(full);
      std::cout << '\n';
    } else if (cmd == "half") {  // acc k neg phi from_inf last r: one GLV half over half-table 0
      Acc a = read_acc(in);
      std::string ks, r;
      int neg, phi, from_inf, last;
      in >> ks >> neg >> phi >> from_inf >> last >> r;
      if (table.size() != 2 * THALF_U32) return 3;
      Acc b = a;
      uint32_t k[4], kr[4];
      limbs4(k, fe_hex(ks));
      limbs4(kr, fe_hex(ks));
      const fe rr = fe_hex(r);
      key_table_add<TW, TN, true>(a.R, a.inf, table.data(), k, neg != 0, phi != 0, from_inf != 0, last != 0);
      key_table_add_ref<TW, TN>(b.R, b.inf, table.data(), kr, neg != 0, phi != 0, from_inf != 0);
      print_xz(a, rr);
      std::cout << ' ';
      print_xz(b, rr);
      print_yzzz(b);
      if (!last) print_yzzz(a);  // a whole sum: Y and ZZZ as well
      std::cout << '\n';
    } else if (cmd == "item") {  // acc k1 k2 signs kc r: verify_item_q's two halves and decision
      Acc a = read_acc(in);
      std::string k1s, k2s, r;
      int signs, kc;
      in >> k1s >> k2s >> signs >> kc >> r;
      if (table.size() != 2 * THALF_U32) return 3;
      Acc b = a;
      const fe rr = fe_hex(r);
      for (int h = 0; h < 2; h++) {
        uint32_t k[4], kr[4];
        limbs4(k, fe_hex(h ? k2s : k1s));
        limbs4(kr, fe_hex(h ? k2s : k1s));
        const uint32_t *tab = table.data() + (h && !kc ? THALF_U32 : 0);
        key_table_add<TW, TN, true>(a.R, a.inf, tab, k, (signs >> h) & 1, kc && h, false, h == 1);
        key_table_add_ref<TW, TN>(b.R, b.inf, tab, kr, (signs >> h) & 1, kc && h, false);
      }
      print_xz(a, rr);
      std::cout << ' ';
      print_xz(b, rr);
      print_yzzz(b);
      std::cout << '\n';
    } else if (!cmd.empty()) {
      return 2;
    }
  }
  return 0;
}
