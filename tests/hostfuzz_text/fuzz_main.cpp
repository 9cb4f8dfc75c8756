// fuzz_main.cpp — ASan/UBSan driver for bv_decode_signatures (hostparse.cpp;
// test infrastructure only, host code, plain clang).  The batch decode is what
// bv_verify_batch_text's small path and its callers' comparison batches rest
// on; the text is attacker-controlled (a BlockSignature or an
// InternalTransaction off the wire).
//
// stdin: one corpus text per line as hex ("-" = the empty text);
// tests/test_text_items.py sends tests/test_hostfuzz.py's signature cases.
// The driver cuts (1) the corpus texts in order, (2) random bytes and (3) the
// corpus bytes run together at random offsets into batches, with empty texts,
// texts of only "|" and one 100 kB text among them, decodes each batch with
// ONE bv_decode_signatures call over exactly-sized heap buffers (an over-read
// or over-write aborts under ASan) and compares every item with
// bv_decode_signature on its own exactly-sized copy.  It also checks the
// argument errors.  stdout: "ok <batches> <items>"; exit status 1 on a
// mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/babbleverify.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static uint64_t n_batches = 0, n_items = 0;

// one batch: the texts, decoded in one call and one by one
static bool check(const std::vector<std::string> &texts) {
  const size_t n = texts.size();
  size_t total = 0;
  for (const std::string &t : texts) total += t.size();
  std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
  std::unique_ptr<uint8_t[]> text(total ? new uint8_t[total] : nullptr);  // all empty: NULL is allowed
  off[0] = 0;
  for (size_t i = 0; i < n; i++) {
    if (!texts[i].empty()) memcpy(text.get() + off[i], texts[i].data(), texts[i].size());
    off[i + 1] = off[i] + texts[i].size();
  }
  std::unique_ptr<uint8_t[]> r(new uint8_t[32 * n ? 32 * n : 1]), s(new uint8_t[32 * n ? 32 * n : 1]),
      pre(new uint8_t[n ? n : 1]);
  memset(r.get(), 0xA5, 32 * n);
  memset(s.get(), 0xA5, 32 * n);
  memset(pre.get(), 0xA5, n);
  const int rc = bv_decode_signatures(n, off.get(), text.get(), r.get(), s.get(), pre.get());
  if (rc != BV_OK) {
    fprintf(stderr, "bv_decode_signatures returned %d on a valid batch of %zu\n", rc, n);
    return false;
  }
  for (size_t i = 0; i < n; i++) {
    const size_t len = texts[i].size();
    std::unique_ptr<char[]> one(new char[len ? len : 1]);  // exact size: no terminator
    if (len) memcpy(one.get(), texts[i].data(), len);
    uint8_t r1[32], s1[32];
    const uint8_t p1 = bv_decode_signature(one.get(), len, r1, s1);
    if (p1 != pre[i] || memcmp(r1, r.get() + 32 * i, 32) || memcmp(s1, s.get() + 32 * i, 32)) {
      fprintf(stderr, "item %zu of %zu (length %zu): batch pre %d, one-item pre %d, or r / s differ\n", i, n, len,
              (int)pre[i], (int)p1);
      return false;
    }
  }
  n_batches++;
  n_items += n;
  return true;
}

// `bytes` cut at random offsets into n texts (several empty when n is large)
static std::vector<std::string> split(const std::string &bytes, size_t n) {
  std::vector<size_t> cut(n + 1);
  cut[0] = 0, cut[n] = bytes.size();
  for (size_t i = 1; i < n; i++) cut[i] = bytes.empty() ? 0 : rnd() % (bytes.size() + 1);
  for (size_t i = 1; i < n; i++)  // insertion sort: n is small
    for (size_t j = i; j > 1 && cut[j - 1] > cut[j]; j--) std::swap(cut[j - 1], cut[j]);
  std::vector<std::string> out(n);
  for (size_t i = 0; i < n; i++) out[i] = bytes.substr(cut[i], cut[i + 1] - cut[i]);
  return out;
}

static bool check_errors() {
  uint8_t r[64], s[64], pre[2];
  const uint64_t good[3] = {0, 3, 6}, down[3] = {0, 5, 3};
  const uint8_t text[6] = {'1', '|', '2', '3', '|', '4'};
  bool ok = bv_decode_signatures(2, good, text, r, s, pre) == BV_OK && pre[0] == 0 && pre[1] == 0;
  ok = ok && bv_decode_signatures(2, down, text, r, s, pre) == BV_E_ARGS;
  ok = ok && bv_decode_signatures(2, nullptr, text, r, s, pre) == BV_E_ARGS;
  ok = ok && bv_decode_signatures(2, good, nullptr, r, s, pre) == BV_E_ARGS;
  ok = ok && bv_decode_signatures(2, good, text, nullptr, s, pre) == BV_E_ARGS;
  ok = ok && bv_decode_signatures(2, good, text, r, nullptr, pre) == BV_E_ARGS;
  ok = ok && bv_decode_signatures(2, good, text, r, s, nullptr) == BV_E_ARGS;
  ok = ok && bv_decode_signatures(0, nullptr, nullptr, nullptr, nullptr, nullptr) == BV_OK;
  if (!ok) fprintf(stderr, "argument checks\n");
  return ok;
}

int main() {
  std::vector<std::string> corpus;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "-") line.clear();
    std::string t(line.size() / 2, '\0');
    for (size_t i = 0; i < t.size(); i++) t[i] = (char)std::stoul(line.substr(2 * i, 2), nullptr, 16);
    corpus.push_back(t);
  }
  bool ok = check_errors();
  // fixed shapes: nothing but empty texts, a lone "|", a 100 kB text between short ones
  ok = ok && check({}) && check({""}) && check({"", "", ""}) && check({"|"}) && check({"", "|", "", "|", "|"});
  {
    std::string big(100 * 1000, '7');
    ok = ok && check({"1|2", big, "3|4"});  // one part: BV_PRE_PARTS_BAD
    big[50 * 1000] = '|';
    ok = ok && check({"", big, "|", big, "z|z"});  // two parts, both far past N
    for (size_t i = 0; i < big.size(); i++) big[i] = (char)rnd();
    ok = ok && check({big}) && check(split(big, 40));
  }
  // the corpus texts as they are, in batches of cycling sizes
  static const size_t sizes[] = {1, 2, 7, 16, 17, 64, 100, 257};
  for (size_t at = 0, c = 0; ok && at < corpus.size(); c++) {
    const size_t n = std::min(sizes[c % 8], corpus.size() - at);
    ok = check(std::vector<std::string>(corpus.begin() + at, corpus.begin() + at + n));
    at += n;
  }
  // corpus bytes run together, and random bytes over a signature's alphabet, cut at random offsets
  static const char alphabet[] = "0123456789abcdefghijklmnopqrstuvwxyzABCXYZ+-||||_ .";
  for (int round = 0; ok && round < 400; round++) {
    std::string bytes;
    if (round % 2 && !corpus.empty()) {
      for (int k = 0; k < 20; k++) bytes += corpus[rnd() % corpus.size()];
    } else {
      bytes.resize(rnd() % 3000);
      for (char &ch : bytes) ch = round % 4 ? alphabet[rnd() % (sizeof alphabet - 1)] : (char)rnd();
    }
    ok = check(split(bytes, 1 + rnd() % 60));
  }
  if (!ok) return 1;
  std::cout << "ok " << n_batches << " " << n_items << "\n";
  return 0;
}
