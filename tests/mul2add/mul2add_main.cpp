// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for the host form of
// fe_mul2add (babble_amd/csrc/field.h), compiled with plain clang under
// AddressSanitizer + UBSan by tests/test_field_mul2add.py.  Reads lines of
// four field elements "a b x y" (64 hex digits each, big-endian) from the
// file given as argv[1] and prints a b + x y mod p as the raw (weakly
// reduced) limbs, one line per input line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../babble_amd/csrc/field.h"

static fe fe_hex(const std::string &s) {
  fe a;
  if (s.size() != 64) {
    fprintf(stderr, "bad field element '%s'\n", s.c_str());
    exit(2);
  }
  for (int i = 0; i < 8; i++) a.v[7 - i] = (uint32_t)strtoul(s.substr(8 * i, 8).c_str(), nullptr, 16);
  return a;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string a, b, x, y;
    in >> a >> b >> x >> y;
    fe r;
    fe_mul2add(r, fe_hex(a), fe_hex(b), fe_hex(x), fe_hex(y));
    char buf[65];
    for (int i = 0; i < 8; i++) snprintf(buf + 8 * i, 9, "%08x", r.v[7 - i]);
    std::cout << buf << '\n';
  }
  return 0;
}
