// Driver for bv_plan_event_shards (babble_amd/csrc/hostplan.cpp) under
// AddressSanitizer + UBSan (test infrastructure only; host code, no device).
// One case per input line:
//   P <n_shards> <n_events> <n_parent_hashes> <kinds> <refs>
//     kinds: 2 * n_events digits (or '-'), refs: 2 * n_events decimal values
//     separated by ',' (or '-').  Every array is copied into an exactly-sized
//     heap buffer, so a read past its end aborts the run.
//   -> P <rc> <bounds,...> <hash_lo,...> <hash_hi,...>   (rc < 0: "P <rc>")
//   N   the NULL-pointer and n_shards <= 0 cases -> N <rc> <rc> <rc> <rc> <rc>
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

static void join(const uint64_t *v, int n) {
  for (int i = 0; i < n; i++) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "N") {
      bv_event_batch b = {};
      uint64_t x[3] = {0, 0, 0};
      printf("N %d %d %d %d %d\n", bv_plan_event_shards(nullptr, 2, x, x, x), bv_plan_event_shards(&b, 2, nullptr, x, x),
             bv_plan_event_shards(&b, 2, x, nullptr, x), bv_plan_event_shards(&b, 2, x, x, nullptr),
             bv_plan_event_shards(&b, 0, x, x, x));
      continue;
    }
    int D = 0;
    uint64_t n = 0, nh = 0;
    std::string ks, rs;
    in >> D >> n >> nh >> ks >> rs;
    std::vector<uint8_t> kinds;
    std::vector<uint64_t> refs;
    if (ks != "-")
      for (char c : ks) kinds.push_back((uint8_t)(c - '0'));
    if (rs != "-") {
      std::istringstream r(rs);
      std::string tok;
      while (std::getline(r, tok, ',')) refs.push_back(strtoull(tok.c_str(), nullptr, 10));
    }
    if (kinds.size() != 2 * n || refs.size() != 2 * n || D <= 0) {
      printf("P bad-input\n");
      continue;
    }
    uint8_t *k = exact(kinds);
    uint64_t *r = exact(refs);
    bv_event_batch b = {};
    b.n_events = n;
    b.parent_kind = k;
    b.parent_ref = r;
    b.n_parent_hashes = nh;
    uint64_t *bounds = exact(std::vector<uint64_t>(D + 1, 0)), *lo = exact(std::vector<uint64_t>(D, 0)),
             *hi = exact(std::vector<uint64_t>(D, 0));
    const int rc = bv_plan_event_shards(&b, D, bounds, lo, hi);
    printf("P %d", rc);
    if (rc >= 0) {
      printf(" ");
      join(bounds, D + 1);
      printf(" ");
      join(lo, D);
      printf(" ");
      join(hi, D);
    }
    printf("\n");
    free(k), free(r), free(bounds), free(lo), free(hi);
  }
  return 0;
}
