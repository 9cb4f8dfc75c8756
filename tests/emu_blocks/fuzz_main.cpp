// ASan + UBSan fuzz driver of the BlockBody serialiser
// (babble_amd/csrc/blkjson.h): random block batches in exactly-sized heap
// arrays (so any read past an array's end is reported), blk_len against the
// bytes blk_emit writes into an exactly-sized body, and the streaming SHA
// sink (a 25-word row on the stack) over the same fields.  Stand-alone (its own main),
// host code only; run by tests/test_block_fields.py as a subprocess.
//   blkfuzz <seed> <rounds>     prints "ok <bodies> <bytes>" or aborts
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../babble_amd/csrc/blkjson.h"

namespace {
uint64_t g_state;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

// an exactly-sized heap copy of v (nullptr when empty and `null_ok`)
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
      fprintf(stderr, "blk_emit wrote past blk_len\n");
      abort();
    }
    *p++ = c;
  }
};

}  // namespace

int main(int argc, char **argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int rounds = argc > 2 ? atoi(argv[2]) : 50;
  const int64_t ints[] = {0, -1, 1, INT64_MAX, INT64_MIN, 1600000000, -9, 10, 99, 100};
  uint64_t n_bodies = 0, n_bytes = 0;
  for (int r = 0; r < rounds; r++) {
    const uint64_t n = 1 + below(12);
    std::vector<int64_t> ix(n), rr(n), ts(n);
    std::vector<uint64_t> ho{0}, txs{0}, txo{0}, io{0}, ro{0};
    std::vector<uint8_t> hb, hn, txb, tln, txn, ij, rj;
    for (uint64_t b = 0; b < n; b++) {
      ix[b] = below(3) ? ints[below(10)] : (int64_t)rnd();
      rr[b] = below(3) ? ints[below(10)] : (int64_t)rnd();
      ts[b] = below(3) ? ints[below(10)] : (int64_t)rnd();
      for (int h = 0; h < 3; h++) {
        const bool nil = below(5) == 0;
        const uint64_t len = nil ? 0 : below(3) ? below(5) : 30 + below(6);
        for (uint64_t i = 0; i < len; i++) hb.push_back((uint8_t)rnd());
        ho.push_back(hb.size());
        hn.push_back(nil);
      }
      const bool list_nil = below(6) == 0;
      tln.push_back(list_nil);
      const uint64_t nt = list_nil ? 0 : below(4) ? below(5) : below(40);
      for (uint64_t t = 0; t < nt; t++) {
        const bool nil = below(7) == 0;
        const uint64_t len = nil ? 0 : below(2) ? below(5) : below(200);
        for (uint64_t i = 0; i < len; i++) txb.push_back((uint8_t)rnd());
        txo.push_back(txb.size());
        txn.push_back(nil);
      }
      txs.push_back(txo.size() - 1);
      for (std::vector<uint8_t> *j : {&ij, &rj}) {
        const uint64_t len = below(3) == 0 ? below(300) : below(2) ? 2 : 0;
        for (uint64_t i = 0; i < len; i++) j->push_back((uint8_t)('a' + below(26)));
        (j == &ij ? io : ro).push_back(j->size());
      }
    }
    auto p_ix = exact(ix), p_rr = exact(rr), p_ts = exact(ts);
    auto p_ho = exact(ho), p_txs = exact(txs), p_txo = exact(txo), p_io = exact(io), p_ro = exact(ro);
    auto p_hb = exact(hb), p_hn = exact(hn), p_txb = exact(txb), p_tln = exact(tln), p_txn = exact(txn),
         p_ij = exact(ij), p_rj = exact(rj);
    bv_block_batch k = {};
    k.n_blocks = n;
    k.index = p_ix.get(), k.round_received = p_rr.get(), k.timestamp = p_ts.get();
    k.hash_off = p_ho.get(), k.hash_bytes = p_hb.get();
    k.hash_nil = below(4) ? p_hn.get() : nullptr;
    k.tx_start = p_txs.get(), k.tx_off = p_txo.get(), k.tx_bytes = p_txb.get();
    k.tx_list_nil = below(4) ? p_tln.get() : nullptr;
    k.tx_nil = below(4) ? p_txn.get() : nullptr;
    if (below(4)) k.itx_off = p_io.get(), k.itx_json = p_ij.get();
    if (below(4)) k.rcpt_off = p_ro.get(), k.rcpt_json = p_rj.get();
    for (uint64_t b = 0; b < n; b++) {
      const uint64_t len = blk_len(k, b);
      std::unique_ptr<uint8_t[]> body(new uint8_t[len]);
      CountSink sink{body.get(), body.get() + len};
      blk_emit(k, b, sink);
      if (sink.p != sink.end) {
        fprintf(stderr, "blk_emit wrote %zu bytes, blk_len says %llu\n", (size_t)(sink.p - body.get()),
                (unsigned long long)len);
        return 1;
      }
      if (len < 2 || body[0] != '{' || body[len - 2] != '}' || body[len - 1] != '\n') {
        fprintf(stderr, "body frame\n");
        return 1;
      }
      uint32_t row[25], dig[8];  // the device's sink over the same fields: every byte counted, row never overrun
      EvjSha o = evj_sha_begin(row);
      blk_emit(k, b, o);
      if ((uint64_t)o.nblk * 64 + o.n != len) {
        fprintf(stderr, "the SHA sink took another byte count than blk_len\n");
        return 1;
      }
      evj_sha_finish(o, dig);
      n_bodies++, n_bytes += len;
    }
  }
  printf("ok %llu %llu\n", (unsigned long long)n_bodies, (unsigned long long)n_bytes);
  return 0;
}
