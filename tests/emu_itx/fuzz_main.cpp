// ASan + UBSan fuzz driver of the InternalTransaction serialiser
// (babble_amd/csrc/itxjson.h): random field sets and random offset tables in
// exactly-sized heap arrays (so any read past an array's end is reported), every
// *_len function against the bytes its emit function writes into an
// exactly-sized body, the streaming SHA sink (a 25-word row on the stack) over
// the same fields, and bv_hex_decode under the 66-byte cap the entry point
// stores a key with.  Stand-alone (its own main), host code only; run by
// tests/test_event_itx.py as a subprocess.
//   itxfuzz <seed> <rounds>     prints "ok <bodies> <bytes>" or aborts
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../babble_amd/csrc/itxjson.h"

namespace {
uint64_t g_state;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

struct CountSink {
  uint8_t *p, *end;
  void put(uint8_t c) {
    if (p >= end) {
      fprintf(stderr, "an emit function wrote past its length function\n");
      abort();
    }
    *p++ = c;
  }
};

// bytes that exercise the escaper: controls, quotes, HTML, UTF-8 leads and trails
uint8_t fuzz_byte() {
  static const uint8_t hot[] = {0x00, 0x09, 0x0A, 0x0D, 0x1F, 0x22, 0x26, 0x3C, 0x3E, 0x5C, 0x7F, 0x80, 0x8F, 0x90,
                                0x9F, 0xA0, 0xA8, 0xA9, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE2, 0xED, 0xEF, 0xF0,
                                0xF4, 0xF5, 0xFF, '0', 'X', 'a', 'F', 'g', '|'};
  return below(3) ? hot[below(sizeof hot)] : (uint8_t)rnd();
}

template <class LenFn, class EmitFn>
uint64_t check(uint64_t len, const LenFn &, const EmitFn &emit, const char *what) {
  std::unique_ptr<uint8_t[]> body(new uint8_t[len ? len : 1]);
  CountSink sink{body.get(), body.get() + len};
  emit(sink);
  if (sink.p != sink.end) {
    fprintf(stderr, "%s: emitted %zu bytes, the length function says %llu\n", what, (size_t)(sink.p - body.get()),
            (unsigned long long)len);
    exit(1);
  }
  uint32_t row[25], dig[8];  // the device's sink over the same fields
  EvjSha o = evj_sha_begin(row);
  emit(o);
  if ((uint64_t)o.nblk * 64 + o.n != len) {
    fprintf(stderr, "%s: the SHA sink took another byte count\n", what);
    exit(1);
  }
  evj_sha_finish(o, dig);
  return len;
}
}  // namespace

int main(int argc, char **argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int rounds = argc > 2 ? atoi(argv[2]) : 50;
  uint64_t n_bodies = 0, n_bytes = 0;
  for (int r = 0; r < rounds; r++) {
    const uint64_t n = 1 + below(10);
    // the events: transactions, parents (hash / none / an earlier event), one key each
    std::vector<int64_t> ix(n), ts(n);
    std::vector<uint32_t> cr(n);
    std::vector<uint8_t> pk(2 * n), ph, kb, txb, tln, txn, iln, ity, str;
    std::vector<uint64_t> pr(2 * n), koff{0}, txs{0}, txo{0}, is{0}, so{0};
    const uint32_t n_keys = 1 + (uint32_t)below(3);
    for (uint32_t k = 0; k < n_keys; k++) {
      const uint64_t len = below(4) ? 65 : below(70);
      for (uint64_t i = 0; i < len; i++) kb.push_back((uint8_t)rnd());
      koff.push_back(kb.size());
    }
    for (uint64_t e = 0; e < n; e++) {
      ix[e] = below(2) ? (int64_t)rnd() : (int64_t)below(100);
      ts[e] = below(2) ? (int64_t)rnd() : (int64_t)below(100);
      cr[e] = (uint32_t)below(n_keys);
      for (int p = 0; p < 2; p++) {
        const uint64_t kind = e ? below(3) : below(2);
        pk[2 * e + p] = (uint8_t)kind;
        pr[2 * e + p] = 0;
        if (kind == BV_PARENT_HASH) {
          pr[2 * e + p] = ph.size() / 32;
          for (int i = 0; i < 32; i++) ph.push_back((uint8_t)rnd());
        } else if (kind == BV_PARENT_EVENT) {
          pr[2 * e + p] = below(e);
        }
      }
      const bool list_nil = below(5) == 0;
      tln.push_back(list_nil);
      const uint64_t nt = list_nil ? 0 : below(4);
      for (uint64_t t = 0; t < nt; t++) {
        const bool nil = below(6) == 0;
        const uint64_t len = nil ? 0 : below(90);
        for (uint64_t i = 0; i < len; i++) txb.push_back((uint8_t)rnd());
        txo.push_back(txb.size());
        txn.push_back(nil);
      }
      txs.push_back(txo.size() - 1);
      // the ITXs: nil / empty / a few, four random strings each
      const bool inil = below(4) == 0;
      iln.push_back(inil);
      const uint64_t ni = inil ? 0 : below(4);
      for (uint64_t i = 0; i < ni; i++) {
        ity.push_back((uint8_t)rnd());
        for (int k = 0; k < 4; k++) {
          const uint64_t len = below(3) ? below(12) : below(160);
          for (uint64_t j = 0; j < len; j++) str.push_back(fuzz_byte());
          so.push_back(str.size());
        }
      }
      is.push_back(ity.size());
    }
    auto p_ix = exact(ix), p_ts = exact(ts);
    auto p_cr = exact(cr);
    auto p_pk = exact(pk), p_ph = exact(ph), p_kb = exact(kb), p_txb = exact(txb), p_tln = exact(tln),
         p_txn = exact(txn), p_iln = exact(iln), p_ity = exact(ity), p_str = exact(str);
    auto p_pr = exact(pr), p_koff = exact(koff), p_txs = exact(txs), p_txo = exact(txo), p_is = exact(is),
         p_so = exact(so);
    bv_event_itx_batch x = {};
    bv_event_batch &b = x.events;
    b.n_events = n, b.n_keys = n_keys;
    b.key_bytes = p_kb.get(), b.key_off = p_koff.get(), b.creator = p_cr.get();
    b.index = p_ix.get(), b.timestamp = p_ts.get();
    b.parent_kind = p_pk.get(), b.parent_ref = p_pr.get();
    b.n_parent_hashes = ph.size() / 32, b.parent_hashes = p_ph.get();
    b.tx_start = p_txs.get(), b.tx_off = p_txo.get(), b.tx_bytes = p_txb.get();
    b.tx_list_nil = below(4) ? p_tln.get() : nullptr;
    b.tx_nil = below(4) ? p_txn.get() : nullptr;
    x.itx_start = p_is.get();
    x.itx_list_nil = below(4) ? p_iln.get() : nullptr;
    x.itx_type = p_ity.get();
    x.itx_str_off = p_so.get();
    x.itx_str = p_str.get();
    const uint64_t m = ity.size();
    for (uint64_t i = 0; i < m; i++) {
      n_bytes += check(itx_body_len(x, i), 0, [&](auto &o) { itx_body_emit(x, i, o); }, "itx_body");
      n_bytes += check(itx_elem_len(x, i), 0, [&](auto &o) { itx_elem_emit(x, i, o); }, "itx_elem");
      for (int k = 0; k < 4; k++)
        check(gojson_string_len(itx_str_ptr(x, i, k), itx_str_len(x, i, k)), 0,
              [&](auto &o) { gojson_string(o, itx_str_ptr(x, i, k), itx_str_len(x, i, k)); }, "gojson_string");
      // the key as the entry point stores it: bv_hex_decode into a buffer of
      // exactly the decoded capacity, then at most 66 bytes kept
      const uint64_t len = itx_str_len(x, i, ITX_PUBKEYHEX);
      if (len >= 2) {
        std::unique_ptr<uint8_t[]> full(new uint8_t[(len - 2) / 2 + 1]);
        const int64_t k = bv_hex_decode((const char *)itx_str_ptr(x, i, ITX_PUBKEYHEX), len, full.get());
        if (k < 0 || (uint64_t)k > (len - 2) / 2) {
          fprintf(stderr, "bv_hex_decode returned %lld for %llu characters\n", (long long)k, (unsigned long long)len);
          return 1;
        }
        std::unique_ptr<uint8_t[]> kept(new uint8_t[66]);
        memcpy(kept.get(), full.get(), (size_t)std::min<int64_t>(k, 66));
      } else if (bv_hex_decode((const char *)itx_str_ptr(x, i, ITX_PUBKEYHEX), len, nullptr) != -1) {
        fprintf(stderr, "bv_hex_decode of a string shorter than 2 bytes must be -1\n");
        return 1;
      }
      n_bodies += 2;
    }
    for (uint64_t e = 0; e < n; e++) {
      uint32_t pp[2];
      const uint64_t len = evj_len(x, e, pp);
      n_bytes += check(len, 0, [&](auto &o) { evj_emit(x, e, o); }, "event body");
      std::unique_ptr<uint8_t[]> body(new uint8_t[len]);
      evj_write(x, e, body.get());
      for (int p = 0; p < 2; p++) {
        if ((pp[p] != EVJ_NOPOS) != (pk[2 * e + p] == BV_PARENT_EVENT)) {
          fprintf(stderr, "ppos set for a parent that is not in the batch (or not set for one that is)\n");
          return 1;
        }
        if (pp[p] == EVJ_NOPOS) continue;
        if ((uint64_t)pp[p] + 64 > len || pp[p] < 3 || memcmp(body.get() + pp[p] - 3, "\"0X", 3) != 0) {
          fprintf(stderr, "ppos does not point at a parent's hex\n");
          return 1;
        }
        for (int i = 0; i < 64; i++)
          if (body[pp[p] + i] != '0') {
            fprintf(stderr, "ppos does not point at the 64 placeholder characters\n");
            return 1;
          }
      }
      n_bodies++;
    }
  }
  printf("ok %llu %llu\n", (unsigned long long)n_bodies, (unsigned long long)n_bytes);
  return 0;
}
