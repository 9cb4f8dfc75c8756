// ASan + UBSan fuzz driver of bv_group_verify_blocks' host-checkable parts:
// the block-shard plan (bv_plan_block_shards, babble_amd/csrc/hostplan.cpp)
// and the rebased BlockBody serialiser (babble_amd/csrc/blkjson.h, blk_len /
// blk_emit with BlkBases).  Per round: a random block batch with random
// sorted items (item-less blocks at the ends and between), the plan over 1..6
// shards in exactly-sized arrays, and every shard's bodies built from
// exactly-sized heap COPIES of its slices alone (so any read outside a slice
// is reported) against the bodies the whole batch gives.  Stand-alone (its
// own main), host code only; run by tests/test_block_shards.py as a subprocess.
//   blkshardfuzz <seed> <rounds>     prints "ok <rounds> <shards> <bodies>" or aborts
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

// an exactly-sized heap copy of v[lo, hi)
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v, uint64_t lo, uint64_t hi) {
  std::unique_ptr<T[]> p(new T[hi > lo ? hi - lo : 1]);
  if (hi > lo) memcpy(p.get(), v.data() + lo, (hi - lo) * sizeof(T));
  return p;
}
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
  return exact(v, 0, v.size());
}

std::vector<uint8_t> body_of(const bv_block_batch &k, uint64_t b) {
  std::vector<uint8_t> out(blk_len(k, b));
  EvjMem m{out.data()};
  blk_emit(k, b, m);
  if (m.p != out.data() + out.size()) {
    fprintf(stderr, "blk_emit and blk_len disagree (whole batch)\n");
    abort();
  }
  return out;
}

struct CountSink {
  uint8_t *p, *end;
  void put(uint8_t c) {
    if (p >= end) {
      fprintf(stderr, "rebased blk_emit wrote past blk_len\n");
      abort();
    }
    *p++ = c;
  }
};

void fail(const char *what) {
  fprintf(stderr, "%s\n", what);
  exit(1);
}
}  // namespace

int main(int argc, char **argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int rounds = argc > 2 ? atoi(argv[2]) : 50;
  const int64_t ints[] = {0, -1, 1, INT64_MAX, INT64_MIN, 1600000000, -9, 10, 99, 100};
  uint64_t n_shards = 0, n_bodies = 0;
  {  // the BV_E_ARGS cases
    bv_block_batch k = {};
    uint64_t x[3] = {};
    const uint32_t ib[1] = {1};
    if (bv_plan_block_shards(nullptr, 2, x, x) != BV_E_ARGS || bv_plan_block_shards(&k, 2, nullptr, x) != BV_E_ARGS ||
        bv_plan_block_shards(&k, 2, x, nullptr) != BV_E_ARGS || bv_plan_block_shards(&k, 0, x, x) != BV_E_ARGS ||
        bv_plan_block_shards(&k, -1, x, x) != BV_E_ARGS)
      fail("bad arguments accepted");
    k.n_blocks = 1, k.n_items = 1;
    if (bv_plan_block_shards(&k, 2, x, x) != BV_E_ARGS) fail("null item_block accepted");
    k.item_block = ib;
    if (bv_plan_block_shards(&k, 2, x, x) != BV_E_ARGS) fail("item_block >= n_blocks accepted");
  }
  for (int r = 0; r < rounds; r++) {
    const uint64_t n = 1 + below(24);
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
    // items sorted by block: 0..4 per block, item-less runs at the ends in some rounds
    std::vector<uint32_t> ib;
    const uint64_t first = below(3) ? 0 : below(n), last = below(3) ? n : first + below(n - first + 1);
    for (uint64_t b = first; b < last; b++)
      for (uint64_t c = below(2) ? below(5) : 0; c > 0; c--) ib.push_back((uint32_t)b);
    if (below(8) == 0) ib.assign(below(9), (uint32_t)below(n));  // one block holds all items
    const bool use_hn = below(4), use_tln = below(4), use_txn = below(4), use_itx = below(4), use_rc = below(4);
    auto p_ix = exact(ix), p_rr = exact(rr), p_ts = exact(ts);
    auto p_ho = exact(ho), p_txs = exact(txs), p_txo = exact(txo), p_io = exact(io), p_ro = exact(ro);
    auto p_hb = exact(hb), p_hn = exact(hn), p_txb = exact(txb), p_tln = exact(tln), p_txn = exact(txn),
         p_ij = exact(ij), p_rj = exact(rj);
    auto p_ib = exact(ib);
    bv_block_batch k = {};
    k.n_blocks = n;
    k.index = p_ix.get(), k.round_received = p_rr.get(), k.timestamp = p_ts.get();
    k.hash_off = p_ho.get(), k.hash_bytes = p_hb.get();
    k.hash_nil = use_hn ? p_hn.get() : nullptr;
    k.tx_start = p_txs.get(), k.tx_off = p_txo.get(), k.tx_bytes = p_txb.get();
    k.tx_list_nil = use_tln ? p_tln.get() : nullptr;
    k.tx_nil = use_txn ? p_txn.get() : nullptr;
    if (use_itx) k.itx_off = p_io.get(), k.itx_json = p_ij.get();
    if (use_rc) k.rcpt_off = p_ro.get(), k.rcpt_json = p_rj.get();
    k.n_items = ib.size();
    k.item_block = p_ib.get();

    // the plan, read from a batch that holds nothing but the counts and item_block
    const int D = 1 + (int)below(6);
    bv_block_batch only = {};
    only.n_blocks = n, only.n_items = ib.size(), only.item_block = p_ib.get();
    std::unique_ptr<uint64_t[]> bb(new uint64_t[D + 1]), ibd(new uint64_t[D + 1]);
    if (bv_plan_block_shards(&only, D, bb.get(), ibd.get()) != 0) fail("sorted items: plan did not return 0");
    if (bb[0] || ibd[0] || bb[D] != n || ibd[D] != ib.size()) fail("plan ends");
    for (int d = 0; d < D; d++) {
      if (bb[d] > bb[d + 1] || ibd[d] > ibd[d + 1]) fail("plan not monotone");
      for (uint64_t i = ibd[d]; i < ibd[d + 1]; i++)
        if (ib[i] < bb[d] || ib[i] >= bb[d + 1]) fail("an item outside its shard's blocks");
    }
    if (ib.size() >= 2 && ib.front() != ib.back()) {  // unsorted: whole on shard 0
      std::vector<uint32_t> un(ib.rbegin(), ib.rend());
      auto p_un = exact(un);
      only.item_block = p_un.get();
      if (bv_plan_block_shards(&only, D, bb.get(), ibd.get()) != 1) fail("unsorted items: plan did not return 1");
      for (int d = 1; d <= D; d++)
        if (bb[0] || ibd[0] || bb[d] != n || ibd[d] != ib.size()) fail("unsorted items: not whole on shard 0");
      only.item_block = p_ib.get();
      if (bv_plan_block_shards(&only, D, bb.get(), ibd.get()) != 0) fail("plan");
    }

    // every shard's bodies from exactly-sized copies of its slices alone
    for (int d = 0; d < D; d++) {
      const uint64_t b0 = bb[d], b1 = bb[d + 1];
      if (b0 == b1) continue;
      n_shards++;
      BlkBases bs = {};
      bs.blk = b0, bs.hash = ho[3 * b0], bs.tx = txs[b0], bs.txb = txo[txs[b0]];
      bs.itx = use_itx ? io[b0] : 0, bs.rcpt = use_rc ? ro[b0] : 0;
      auto s_ix = exact(ix, b0, b1), s_rr = exact(rr, b0, b1), s_ts = exact(ts, b0, b1);
      auto s_ho = exact(ho, 3 * b0, 3 * b1 + 1);
      auto s_hn = exact(hn, 3 * b0, 3 * b1);
      auto s_hb = exact(hb, ho[3 * b0], ho[3 * b1]);
      auto s_txs = exact(txs, b0, b1 + 1), s_txo = exact(txo, txs[b0], txs[b1] + 1);
      auto s_txb = exact(txb, txo[txs[b0]], txo[txs[b1]]);
      auto s_tln = exact(tln, b0, b1), s_txn = exact(txn, txs[b0], txs[b1]);
      auto s_io = exact(io, b0, b1 + 1), s_ro = exact(ro, b0, b1 + 1);
      auto s_ij = exact(ij, io[b0], io[b1]), s_rj = exact(rj, ro[b0], ro[b1]);
      bv_block_batch s = {};
      s.n_blocks = b1 - b0;
      s.index = s_ix.get(), s.round_received = s_rr.get(), s.timestamp = s_ts.get();
      s.hash_off = s_ho.get(), s.hash_bytes = s_hb.get();
      s.hash_nil = use_hn ? s_hn.get() : nullptr;
      s.tx_start = s_txs.get(), s.tx_off = s_txo.get(), s.tx_bytes = s_txb.get();
      s.tx_list_nil = use_tln ? s_tln.get() : nullptr;
      s.tx_nil = use_txn ? s_txn.get() : nullptr;
      if (use_itx) s.itx_off = s_io.get(), s.itx_json = s_ij.get();
      if (use_rc) s.rcpt_off = s_ro.get(), s.rcpt_json = s_rj.get();
      for (uint64_t b = b0; b < b1; b++) {
        const std::vector<uint8_t> want = body_of(k, b);
        const uint64_t len = blk_len(s, b, bs);
        if (len != want.size()) fail("rebased blk_len differs from the whole batch's");
        std::unique_ptr<uint8_t[]> body(new uint8_t[len]);
        CountSink sink{body.get(), body.get() + len};
        blk_emit(s, b, sink, bs);
        if (sink.p != sink.end || memcmp(body.get(), want.data(), len)) fail("rebased body differs");
        EvjMem m{body.get()};  // the host's memory sink takes other overloads (table base64, memcpy)
        blk_emit(s, b, m, bs);
        if (m.p != body.get() + len || memcmp(body.get(), want.data(), len)) fail("rebased body (memory sink) differs");
        uint32_t row[25], dig[8];  // the device's sink: every byte counted, row never overrun
        EvjSha o = evj_sha_begin(row);
        blk_emit(s, b, o, bs);
        if ((uint64_t)o.nblk * 64 + o.n != len) fail("the SHA sink took another byte count than blk_len");
        evj_sha_finish(o, dig);
        n_bodies++;
      }
    }
  }
  printf("ok %d %llu %llu\n", rounds, (unsigned long long)n_shards, (unsigned long long)n_bodies);
  return 0;
}
