// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for the block-level
// batch inversion of k_sinv (babble_amd/csrc/verify_core.h BV_SINV_BLOCK),
// compiled from the device's own source with plain clang
// (tests/test_sinv_block.py).  Both kernels are replayed lane by lane: k_sinv
// (sinv_thread, one inversion per lane) and k_sinv_block<B> (sinv_lane_prefix,
// the totals to an array where the device has LDS, sinv_block_lane on the
// block's first 64 lanes, sinv_lane_finish), with the launcher's geometry.
// argv[1] is B; argv[2] names a file of cases,
//     CASE <n> <M>
//     <s 64 hex> <pre>          n lines
// and for each case the program prints
//     CASE <n> <M> <usable items> <differing>
//     W <i> <w of the block form, 64 hex>     for every usable item
// The buffers have exactly n items, so a sanitizer build catches any lane that
// reaches past the batch.  Exit status 1 if anything differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/verify_core.h"

namespace {

void replay_lanes(uint64_t n, uint32_t M, const uint32_t *s_be, const uint8_t *pre, uint32_t *w) {
  const uint64_t threads = (n + M - 1) / M, T = (threads + 255) / 256 * 256;
  for (uint64_t t = 0; t < T; t++) sinv_thread(t, T, n, M, s_be, pre, w);
}

void replay_block(uint32_t B, uint64_t n, uint32_t M, const uint32_t *s_be, const uint8_t *pre, uint32_t *w) {
  const uint64_t threads = (n + M - 1) / M, grid = (threads + B - 1) / B, T = grid * B;
  std::vector<uint32_t> tot(8 * (size_t)B), inv(8 * (size_t)B);
  for (uint64_t blk = 0; blk < grid; blk++) {
    for (uint32_t x = 0; x < B; x++) {
      sc acc;
      sinv_lane_prefix(acc, blk * B + x, T, n, M, s_be, pre, w);
      for (int k = 0; k < 8; k++) tot[8 * x + k] = acc.v[k];
    }
    // the barrier; the first wave
    for (uint32_t j = 0; j < 64; j++) sinv_block_lane(j, 64, B, tot.data(), inv.data());
    // the barrier
    for (uint32_t x = 0; x < B; x++) {
      sc a;
      for (int k = 0; k < 8; k++) a.v[k] = inv[8 * x + k];
      sinv_lane_finish(a, blk * B + x, T, n, M, s_be, pre, w);
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sinvblock <B> <cases file>\n");
    return 2;
  }
  const uint32_t B = (uint32_t)atoi(argv[1]);
  if (B == 0 || B % 64 != 0 || B > 1024) {
    fprintf(stderr, "B must be a multiple of 64 up to 1024\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::string tag;
  int bad = 0;
  while (in >> tag) {
    uint64_t n;
    uint32_t M;
    if (tag != "CASE" || !(in >> n >> M) || n == 0 || M == 0) {
      fprintf(stderr, "bad case header\n");
      return 2;
    }
    // exactly n items each: nothing to spare behind the last one
    std::vector<uint32_t> s_be(8 * n), w_a(8 * n, 0xA5A5A5A5u), w_b(8 * n, 0x5A5A5A5Au);
    std::vector<uint8_t> pre(n);
    for (uint64_t i = 0; i < n; i++) {
      std::string hex;
      int p;
      if (!(in >> hex >> p) || hex.size() != 64) {
        fprintf(stderr, "bad item %llu\n", (unsigned long long)i);
        return 2;
      }
      uint8_t *bytes = (uint8_t *)&s_be[8 * i];
      for (int k = 0; k < 32; k++) bytes[k] = (uint8_t)strtoul(hex.substr(2 * k, 2).c_str(), nullptr, 16);
      pre[i] = (uint8_t)p;
    }
    replay_lanes(n, M, s_be.data(), pre.data(), w_a.data());
    replay_block(B, n, M, s_be.data(), pre.data(), w_b.data());
    uint64_t usable = 0, differ = 0;
    std::string lines;
    for (uint64_t i = 0; i < n; i++) {
      sc s;
      sc_load_be_words(s, &s_be[8 * i]);
      if (!s_usable(pre.data(), i, s)) continue;
      usable++;
      if (memcmp(&w_a[8 * i], &w_b[8 * i], 32) != 0) differ++;
      char buf[96];
      int o = snprintf(buf, sizeof buf, "W %llu ", (unsigned long long)i);
      for (int k = 0; k < 8; k++) o += snprintf(buf + o, sizeof buf - o, "%08x", w_b[8 * i + 7 - k]);
      lines += buf;
      lines += '\n';
    }
    printf("CASE %llu %u %llu %llu\n%s", (unsigned long long)n, M, (unsigned long long)usable,
           (unsigned long long)differ, lines.c_str());
    if (differ) bad = 1;
  }
  return bad;
}
