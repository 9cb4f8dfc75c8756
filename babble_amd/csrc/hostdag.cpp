// hostdag.cpp — bv_host_dag_hash (hostdag.h).
//
// Work per event (T=1 body, 8 SHA-256 blocks): the body written from its
// wire fields, then — all events in parallel — either its whole digest (level
// 0: no in-batch parent) or the midstate of the blocks wholly before its
// first in-batch parent's hex (2 of 8 blocks); then, level by level, the
// parents' hex spliced in and the remaining blocks (6 of 8) hashed from the
// midstate.  Only that last step is serial along the DAG: ~6 blocks per
// event at ~40 ns a block with the SHA extensions (a 1000-event SyncResponse
// of 333 levels: ~0.25 ms on one core, against ~14 us per level for one GPU
// wave, profiles/r03_chain_ab.log).  Wide levels are spread over the pool.
#include "hostdag.h"

#include <string.h>

#include "bsigjson.h"
#include "hostsha.h"

namespace {
// X: bv_event_batch (the InternalTransactions member from the verbatim
// fragment), bv_event_itx_batch (from the fields, itxjson.h) or
// bv_event_fields_batch (BlockSignatures from fields too, bsigjson.h); b: its
// events
template <class X>
void dag_hash(const X &x, const bv_event_batch &b, const uint32_t *order, const uint32_t *level_off,
              uint32_t n_levels, const HostParFor &pf, HostDagScratch &w, uint8_t *digests) {
  const uint64_t n = b.n_events;
  if (n == 0) return;
  w.off.assign(n + 1, 0);
  w.ppos.assign(2 * n, EVJ_NOPOS);
  w.mid.assign(8 * n, 0);
  uint64_t *off = w.off.data();
  uint32_t *ppos = w.ppos.data();
  pf(n, 512, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t e = lo; e < hi; e++) off[e + 1] = evj_len(x, e, ppos + 2 * e);
  });
  for (uint64_t e = 0; e < n; e++) off[e + 1] += off[e];
  w.bodies.resize(off[n] + 64);
  uint8_t *bodies = w.bodies.data();
  pf(n, 256, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t e = lo; e < hi; e++) evj_write(x, e, bodies + off[e]);
  });
  // level 0: whole digests; above: midstates of the parent-independent blocks
  const uint64_t n0 = level_off[1];
  uint32_t *mid = w.mid.data();
  pf(n, 64, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      const uint32_t e = order[i];
      const uint8_t *body = bodies + off[e];
      if (i < n0) {
        hsha::digest(body, off[e + 1] - off[e], digests + 32ull * e);
      } else {
        hsha::init(mid + 8ull * e);
        hsha::compress(mid + 8ull * e, body, ev_mid_blocks(ppos + 2 * e));
      }
    }
  });
  // the chain: level L's events need only levels < L; a level's events are
  // finished in pairs whose compressions interleave (hsha::finish2)
  auto splice = [&](uint32_t e) {
    uint8_t *body = bodies + off[e];
    for (int p = 0; p < 2; p++)
      if (ppos[2 * e + p] != EVJ_NOPOS) evj_hex32(body + ppos[2 * e + p], digests + 32ull * b.parent_ref[2 * e + p]);
  };
  auto finish = [&](uint64_t lo, uint64_t hi) {
    uint64_t i = lo;
    for (; i + 1 < hi; i += 2) {
      const uint32_t e = order[i], f = order[i + 1];
      splice(e);
      splice(f);
      uint32_t he[8], hf[8];
      memcpy(he, mid + 8ull * e, sizeof he);
      memcpy(hf, mid + 8ull * f, sizeof hf);
      hsha::finish2(he, bodies + off[e], 64ull * ev_mid_blocks(ppos + 2 * e), off[e + 1] - off[e],
                    digests + 32ull * e, hf, bodies + off[f], 64ull * ev_mid_blocks(ppos + 2 * f),
                    off[f + 1] - off[f], digests + 32ull * f);
    }
    if (i < hi) {
      const uint32_t e = order[i];
      splice(e);
      uint32_t h[8];
      memcpy(h, mid + 8ull * e, sizeof h);
      hsha::finish(h, bodies + off[e], 64ull * ev_mid_blocks(ppos + 2 * e), off[e + 1] - off[e], digests + 32ull * e);
    }
  };
  for (uint32_t L = 1; L < n_levels; L++) {
    const uint64_t a = level_off[L], z = level_off[L + 1];
    if (z - a >= 128)
      pf(z - a, 32, [&](uint64_t lo, uint64_t hi) { finish(a + lo, a + hi); });
    else
      finish(a, z);
  }
}
}  // namespace

const char *bv_check_event_fields(const bv_event_batch *b, CopyPool *pool, bool entry) {
  const uint64_t n = b->n_events;
  if (!n) return nullptr;
  if (!b->creator || !b->index || !b->timestamp || !b->parent_kind || !b->parent_ref || !b->tx_start ||
      (entry && !b->sig_text && (!b->r_be || !b->s_be)) || !b->key_off)
    return "null event array";
  if (entry && b->sig_text) {  // signature text: offsets from 0, monotone
    if (!b->sig_off || b->sig_off[0] != 0) return "sig_off missing or sig_off[0] != 0";
    if (!monotone(pool, b->sig_off, n)) return "sig_off not monotone";
  }
  if (b->key_off[0] != 0) return "key_off[0] != 0";
  if (!monotone(nullptr, b->key_off, b->n_keys)) return "key_off not monotone";
  if (b->key_off[b->n_keys] && !b->key_bytes) return "null key bytes";
  if (b->tx_start[0] != 0) return "tx_start[0] != 0";
  const uint64_t n_tx = b->tx_start[n];
  if (n_tx && !b->tx_off) return "null tx_off";
  if (n_tx && b->tx_off[0] != 0) return "tx_off[0] != 0";
  if (!monotone(pool, b->tx_off, n_tx)) return "tx_off not monotone";
  if (n_tx && b->tx_off[n_tx] && !b->tx_bytes) return "null tx bytes";
  const uint64_t *offs[2] = {entry ? b->itx_off : nullptr, b->bsig_off};
  const uint8_t *json[2] = {b->itx_json, b->bsig_json};
  for (const uint64_t *off : offs)
    if (off && off[0] != 0) return "fragment offsets must start at 0";
  for (int f = 0; f < 2; f++)
    if (offs[f] && offs[f][n] && !json[f]) return "null fragment bytes";
  for (const uint64_t *off : offs)
    if (off && !monotone(pool, off, n)) return "fragment offsets not monotone";
  const auto refs = [b](uint64_t lo, uint64_t hi) {
    for (uint64_t e = lo; e < hi; e++) {
      if (b->creator[e] >= b->n_keys || b->tx_start[e] > b->tx_start[e + 1]) return false;
      for (int p = 0; p < 2; p++) {
        const uint8_t k = b->parent_kind[2 * e + p];
        const uint64_t r = b->parent_ref[2 * e + p];
        if (k > BV_PARENT_EVENT) return false;
        if (k == BV_PARENT_HASH && (r >= b->n_parent_hashes || !b->parent_hashes)) return false;
        if (k == BV_PARENT_EVENT && r >= e) return false;  // an in-batch parent precedes its child
      }
    }
    return true;
  };
  if (!(pool ? pool->parallel_for(n, 1 << 17, refs) : refs(0, n)))
    return "bad event reference (creator, tx_start, or a parent not earlier in the batch / out of range)";
  return nullptr;
}

void bv_dag_levels(const bv_event_batch &b, std::vector<uint32_t> &order, std::vector<uint32_t> &level_off) {
  const uint64_t n = b.n_events;
  std::vector<uint32_t> level(n, 0);
  uint32_t nl = 1;
  for (uint64_t e = 0; e < n; e++) {
    uint32_t l = 0;
    for (int p = 0; p < 2; p++)
      if (b.parent_kind[2 * e + p] == BV_PARENT_EVENT) l = std::max(l, level[b.parent_ref[2 * e + p]] + 1);
    level[e] = l;
    nl = std::max(nl, l + 1);
  }
  level_off.assign(nl + 1, 0);
  for (uint64_t e = 0; e < n; e++) level_off[level[e] + 1]++;
  for (uint32_t l = 0; l < nl; l++) level_off[l + 1] += level_off[l];
  order.resize(n);
  std::vector<uint32_t> fill(level_off.begin(), level_off.end() - 1);
  for (uint64_t e = 0; e < n; e++) order[fill[level[e]]++] = (uint32_t)e;
}

void bv_host_dag_hash(const bv_event_batch &b, const uint32_t *order, const uint32_t *level_off, uint32_t n_levels,
                      const HostParFor &pf, HostDagScratch &w, uint8_t *digests) {
  dag_hash(b, b, order, level_off, n_levels, pf, w, digests);
}

void bv_host_dag_hash_itx(const bv_event_itx_batch &x, const uint32_t *order, const uint32_t *level_off,
                          uint32_t n_levels, const HostParFor &pf, HostDagScratch &w, uint8_t *digests) {
  dag_hash(x, x.events, order, level_off, n_levels, pf, w, digests);
}

void bv_host_dag_hash_fields(const bv_event_fields_batch &f, const uint32_t *order, const uint32_t *level_off,
                             uint32_t n_levels, const HostParFor &pf, HostDagScratch &w, uint8_t *digests) {
  dag_hash(f, f.ev.events, order, level_off, n_levels, pf, w, digests);
}
