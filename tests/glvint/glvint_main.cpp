// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for the GLV split in
// plain integers (babble_amd/csrc/field.h glv_split_int, BV_GLV_INT), compiled
// from the device's own source with plain clang, optionally under
// AddressSanitizer + UBSan (tests/test_glv_int.py).  Reads one scalar k < N
// per line (64 hex digits, big-endian) from the file given as argv[1], runs
// glv_split_mont (three Montgomery products, the earlier form), glv_split_int
// and glv_split (the form the build selects) on it and prints
//     <|k1| 32 hex> <|k2| 32 hex> <signs>
// of the integer form per scalar.  Exit status 1, with the scalar on stderr,
// where the three do not agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "../../babble_amd/csrc/field.h"

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s scalars.txt\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::string line, out;
  int bad = 0;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    if (line.size() != 64) {
      fprintf(stderr, "bad scalar '%s'\n", line.c_str());
      return 2;
    }
    sc k;
    for (int i = 0; i < 8; i++) k.v[7 - i] = (uint32_t)strtoul(line.substr(8 * i, 8).c_str(), nullptr, 16);
    uint32_t a1[4], a2[4], as, b1[4], b2[4], bs, c1[4], c2[4], cs;
    glv_split_mont(a1, a2, as, k);
    glv_split_int(b1, b2, bs, k);
    glv_split(c1, c2, cs, k);
    const bool same = !memcmp(a1, b1, 16) && !memcmp(a2, b2, 16) && as == bs;
    const bool sel = BV_GLV_INT ? (!memcmp(c1, b1, 16) && !memcmp(c2, b2, 16) && cs == bs)
                                : (!memcmp(c1, a1, 16) && !memcmp(c2, a2, 16) && cs == as);
    if (!same || !sel) {
      if (bad++ < 10)
        fprintf(stderr, "MISMATCH k=%s mont %08x%08x%08x%08x %08x%08x%08x%08x %u int %08x%08x%08x%08x %08x%08x%08x%08x %u\n",
                line.c_str(), a1[3], a1[2], a1[1], a1[0], a2[3], a2[2], a2[1], a2[0], as, b1[3], b1[2], b1[1], b1[0],
                b2[3], b2[2], b2[1], b2[0], bs);
    }
    char buf[80];
    snprintf(buf, sizeof buf, "%08x%08x%08x%08x %08x%08x%08x%08x %u\n", b1[3], b1[2], b1[1], b1[0], b2[3], b2[2], b2[1],
             b2[0], bs);
    out += buf;
  }
  fputs(out.c_str(), stdout);
  return bad ? 1 : 0;
}
