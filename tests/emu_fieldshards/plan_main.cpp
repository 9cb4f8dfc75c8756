// Driver for bv_plan_event_fields_shards (babble_amd/csrc/hostplan.cpp) under
// AddressSanitizer + UBSan (test infrastructure only; host code, no device).
// One case per input line:
//   P <n_shards> <n_events> <n_parent_hashes> <kinds> <refs> <itx_start> <bsig_start>
//     kinds: 2 * n_events digits (or '-'); refs: 2 * n_events decimal values
//     separated by ',' (or '-'); itx_start / bsig_start: n_events + 1 values
//     (itx_start '-': NULL, a batch without ITX fields).  Every array is copied
//     into an exactly-sized heap buffer, so a read past its end aborts the run.
//   -> P <rc> <event bounds,...> <itx bounds,...> <bsig bounds,...> <hash_lo,...> <hash_hi,...>
//      (rc < 0: "P <rc>")
//   N   the NULL-pointer and n_shards <= 0 cases -> N <rc> x 8
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/babbleverify.h"

template <class T>
static T *exact(const std::vector<T> &v) {  // exactly v.size() elements on the heap (never NULL)
  T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

static std::vector<uint64_t> numbers(const std::string &s) {
  std::vector<uint64_t> out;
  if (s == "-") return out;
  std::istringstream r(s);
  std::string tok;
  while (std::getline(r, tok, ',')) out.push_back(strtoull(tok.c_str(), nullptr, 10));
  return out;
}

static void join(const uint64_t *v, int n) {
  printf(" ");
  for (int i = 0; i < n; i++) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "N") {
      bv_event_fields_batch f = {};
      uint64_t x[3] = {0, 0, 0};
      printf("N %d %d %d %d %d %d %d %d\n", bv_plan_event_fields_shards(nullptr, 2, x, x, x, x, x),
             bv_plan_event_fields_shards(&f, 2, nullptr, x, x, x, x),
             bv_plan_event_fields_shards(&f, 2, x, nullptr, x, x, x),
             bv_plan_event_fields_shards(&f, 2, x, x, nullptr, x, x),
             bv_plan_event_fields_shards(&f, 2, x, x, x, nullptr, x),
             bv_plan_event_fields_shards(&f, 2, x, x, x, x, nullptr), bv_plan_event_fields_shards(&f, 0, x, x, x, x, x),
             bv_plan_event_fields_shards(&f, -1, x, x, x, x, x));
      continue;
    }
    int D = 0;
    uint64_t n = 0, nh = 0;
    std::string ks, rs, is, bs;
    in >> D >> n >> nh >> ks >> rs >> is >> bs;
    std::vector<uint8_t> kinds;
    if (ks != "-")
      for (char c : ks) kinds.push_back((uint8_t)(c - '0'));
    const std::vector<uint64_t> refs = numbers(rs), istart = numbers(is), bstart = numbers(bs);
    if (kinds.size() != 2 * n || refs.size() != 2 * n || D <= 0 || (is != "-" && istart.size() != n + 1) ||
        bstart.size() != n + 1) {
      printf("P bad-input\n");
      continue;
    }
    uint8_t *k = exact(kinds);
    uint64_t *r = exact(refs), *i0 = is == "-" ? nullptr : exact(istart), *b0 = exact(bstart);
    bv_event_fields_batch f = {};
    f.ev.events.n_events = n;
    f.ev.events.parent_kind = k;
    f.ev.events.parent_ref = r;
    f.ev.events.n_parent_hashes = nh;
    f.ev.itx_start = i0;
    f.bsig_start = b0;
    const std::vector<uint64_t> zb(D + 1, 0), zd(D, 0);
    uint64_t *eb = exact(zb), *ib = exact(zb), *bb = exact(zb), *lo = exact(zd), *hi = exact(zd);
    const int rc = bv_plan_event_fields_shards(&f, D, eb, ib, bb, lo, hi);
    printf("P %d", rc);
    if (rc >= 0) join(eb, D + 1), join(ib, D + 1), join(bb, D + 1), join(lo, D), join(hi, D);
    printf("\n");
    free(k), free(r), free(i0), free(b0), free(eb), free(ib), free(bb), free(lo), free(hi);
  }
  return 0;
}
