// Stand-alone host program (TEST INFRASTRUCTURE ONLY, tests/test_table_audit.py):
// the self-test of the audit relations of audit.h.  It builds one K8 and one
// K12 table for the keys of argv[1] (one "<x 64 hex> <y 64 hex>" per line) on
// the host by plain per-entry double-and-add (table_point / table_store: the
// build code is allowed here, this program tests the audit, not the builder),
// runs the relations serially over them, then over copies with one named
// corruption each, and prints one line per case:
//     CASE <table> <name> <audited> <failures> [<relation>:<key>:<window>:<digit> ...]
//     FORM <name> <0|1>            tc_form_ok of a synthetic entry
// Corruptions go to key 0; key 1 stays untouched.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/verify_core.h"
#include "audit.h"

namespace {

constexpr uint32_t FILL = 0xA5A5A5A5u;
using Fail = std::array<uint32_t, 4>;

fe fe_hex(const std::string &s) {
  fe a;
  if (s.size() != 64) {
    fprintf(stderr, "bad field element '%s'\n", s.c_str());
    exit(2);
  }
  for (int i = 0; i < 8; i++) a.v[7 - i] = (uint32_t)strtoul(s.substr(8 * i, 8).c_str(), nullptr, 16);
  return a;
}

// every required entry of key b's table: T[j][d] = d 2^(W j) Q by double-and-add
// from the window's base, one inversion per window (prefix products)
void build(const tc_geom &g, uint32_t b, const uint32_t *kxy, uint32_t *table) {
  std::vector<uint32_t> bases((size_t)g.nwin * 24);
  table_bases_one<false>(0, kxy + 16 * b, bases.data(), (int)g.w, (int)g.nwin);
  uint32_t *tab = table + b * tc_table_u32(g);
  const uint64_t half = tc_half_u32(g);
  for (uint32_t j = 0; j < g.nwin; j++) {
    fe bx, by, bz;
    fe_load(bx, &bases[24 * j]);
    fe_load(by, &bases[24 * j + 8]);
    fe_load(bz, &bases[24 * j + 16]);
    const uint64_t n = tc_required(g, j);
    std::vector<gej> R(n + 1);
    std::vector<fe> Z(n + 1), pre(n + 2);
    fe_set(pre[1], 1);
    for (uint64_t d = 1; d <= n; d++) {
      bool inf;
      table_point<false>(R[d], inf, Z[d], bx, by, (uint32_t)d, (int)g.w);
      fe_mul(Z[d], Z[d], bz);
      fe_mul(pre[d + 1], pre[d], Z[d]);
    }
    fe inv;
    fe_inv(inv, pre[n + 1]);
    for (uint64_t d = n; d >= 1; d--) {
      fe zi;
      fe_mul(zi, inv, pre[d]);
      fe_mul(inv, inv, Z[d]);
      uint32_t *e = tab + tc_slot(g, j, d) * TC_ENTRY_U32;
      table_store(e, g.phi ? e + half : nullptr, (uint32_t)d, R[d], false, zi);
    }
    if (!g.is_signed) {  // K8 slot 0: the identity, zeros in both halves
      uint32_t *e = tab + tc_slot(g, j, 0) * TC_ENTRY_U32;
      for (int i = 0; i < TC_ENTRY_U32; i++) e[i] = e[half + i] = 0;
    }
  }
}

// the relations over every required slot of every key, serially
void run(const char *table_name, const char *name, const tc_geom &g, uint32_t n_keys, const uint32_t *kxy,
         const std::vector<uint32_t> &table) {
  std::vector<Fail> fails;
  uint64_t audited = 0;
  for (uint32_t b = 0; b < n_keys; b++)
    for (uint32_t j = 0; j < g.nwin; j++)
      for (uint64_t d = g.is_signed ? 1 : 0; d <= tc_required(g, j); d++) {
        const uint32_t *tab = table.data() + b * tc_table_u32(g);
        uint32_t bad = g.is_signed ? tc_audit_signed(g, tab, kxy + 16 * b, j, d) : tc_audit_unsigned(g, tab, kxy + 16 * b, j, d);
        audited += d != 0 ? (g.phi ? 2 : 1) : 0;
        for (uint32_t r = 0; bad; r++, bad >>= 1)
          if (bad & 1u) fails.push_back({r, b, j, (uint32_t)d});
      }
  std::sort(fails.begin(), fails.end());
  printf("CASE %s %s %llu %zu", table_name, name, (unsigned long long)audited, fails.size());
  for (size_t i = 0; i < fails.size(); i++) printf(" %u:%u:%u:%u", fails[i][0], fails[i][1], fails[i][2], fails[i][3]);
  printf("\n");
}

void sub_from_p(uint32_t *y) {  // y <- p - y
  const uint32_t p[8] = {P0, P1, PX, PX, PX, PX, PX, PX};
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)p[i] - y[i] - br;
    y[i] = (uint32_t)t;
    br = (t >> 32) & 1;
  }
}

void add_p(uint32_t *x) {  // x <- x + p (the caller keeps it below 2^256)
  const uint32_t p[8] = {P0, P1, PX, PX, PX, PX, PX, PX};
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)x[i] + p[i] + c;
    x[i] = (uint32_t)t;
    c = t >> 32;
  }
}

void cases(const char *tn, const tc_geom &g, uint32_t n_keys, const uint32_t *kxy, const std::vector<uint32_t> &clean,
           uint32_t j, uint32_t d) {
  const uint64_t half = tc_half_u32(g);
  auto at = [&](std::vector<uint32_t> &t, uint32_t jj, uint64_t dd) { return t.data() + tc_slot(g, jj, dd) * TC_ENTRY_U32; };
  auto swap_entries = [&](uint32_t *a, uint32_t *b) {
    for (int h = 0; h < (g.phi ? 2 : 1); h++)
      for (int i = 0; i < TC_ENTRY_U32; i++) std::swap(a[h * half + i], b[h * half + i]);
  };
  run(tn, "clean", g, n_keys, kxy, clean);
  std::vector<uint32_t> t = clean;
  at(t, j, d)[0] ^= 1u;
  run(tn, "flipx", g, n_keys, kxy, t);
  t = clean;
  sub_from_p(at(t, j, d) + 8);
  run(tn, "negy", g, n_keys, kxy, t);
  t = clean;
  swap_entries(at(t, j, d), at(t, j, d + 1));
  run(tn, "swap", g, n_keys, kxy, t);
  t = clean;
  for (int h = 0; h < (g.phi ? 2 : 1); h++)
    for (int i = 0; i < TC_ENTRY_U32; i++) at(t, j, d)[h * half + i] = at(t, j + 1, d)[h * half + i];
  run(tn, "nextwin", g, n_keys, kxy, t);
  t = clean;
  for (int i = 0; i < 8; i++) at(t, j, d)[half + i] = at(t, j, d)[i];
  run(tn, "phix", g, n_keys, kxy, t);
  t = clean;
  for (int i = 0; i < TC_ENTRY_U32; i++) at(t, j, d)[i] = 0;
  run(tn, "zeroed", g, n_keys, kxy, t);
  t = clean;  // a non-canonical coordinate: x = 5 + p, below 2^256
  for (int i = 0; i < 8; i++) at(t, j, d)[i] = i == 0 ? 5u : 0u;
  add_p(at(t, j, d));
  run(tn, "noncanon", g, n_keys, kxy, t);
  if (g.is_signed) {  // the window's top digit, in slot 0 of the next window
    t = clean;
    at(t, j, tc_ent(g))[0] ^= 1u;
    run(tn, "flipx_top", g, n_keys, kxy, t);
  }
  if (!g.is_signed) {  // K8 slot 0 must stay the identity in both halves
    t = clean;
    at(t, j, 0)[half + 3] = 1u;
    run(tn, "slot0", g, n_keys, kxy, t);
  }
  t = clean;  // the anchor
  at(t, 0, 1)[8] ^= 1u;
  run(tn, "anchor", g, n_keys, kxy, t);
}

void form(const char *name, uint32_t x0, bool x_plus_p, uint32_t y0, bool y_plus_p) {
  uint32_t e[16] = {};
  e[0] = x0;
  e[8] = y0;
  if (x_plus_p) add_p(e);
  if (y_plus_p) add_p(e + 8);
  printf("FORM %s %d\n", name, tc_form_ok(e) ? 1 : 0);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s keys.txt\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  std::vector<uint32_t> kxy;
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string x, y;
    in >> x >> y;
    const fe fx = fe_hex(x), fy = fe_hex(y);
    kxy.insert(kxy.end(), fx.v, fx.v + 8);
    kxy.insert(kxy.end(), fy.v, fy.v + 8);
  }
  const uint32_t n_keys = (uint32_t)(kxy.size() / 16);
  if (n_keys != 2) {
    fprintf(stderr, "two keys expected\n");
    return 2;
  }
  const tc_geom k8 = {BV_KW, BV_KNWIN, 128, 0, 1}, k12 = {BV_K12W, BV_K12NWIN, 128, 1, 1};
  if (tc_table_u32(k8) != BV_KTABLE_U32 || tc_table_u32(k12) != BV_K12TABLE_U32) {
    fprintf(stderr, "geometry mismatch\n");
    return 2;
  }
  std::vector<uint32_t> t8(n_keys * tc_table_u32(k8), FILL), t12(n_keys * tc_table_u32(k12), FILL);
  for (uint32_t b = 0; b < n_keys; b++) {
    build(k8, b, kxy.data(), t8.data());
    build(k12, b, kxy.data(), t12.data());
  }
  cases("K8", k8, n_keys, kxy.data(), t8, 7, 100);
  cases("K12", k12, n_keys, kxy.data(), t12, 5, 1000);
  form("small", 5, false, 7, false);
  form("x_plus_p", 5, true, 7, false);
  form("y_plus_p", 5, false, 7, true);
  form("zero", 0, false, 0, false);
  form("x_is_p", 0, true, 7, false);
  return 0;
}
