// hostplan.cpp — host helpers of the multi-device group (no device, no HIP):
//
//   bv_plan_shards       contiguous item ranges balanced by count, cut only
//                        where the message changes (a BlockBody's validator
//                        signatures, block.go:343 / hashgraph.go:1599-1630,
//                        stay on one device);
//   bv_plan_group        the whole plan of bv_group_verify_batch: item order,
//                        item shards, message partition;
//   bv_merge_shard_bits  the accept bitmask from the all-gathered shard words;
//   bv_plan_event_shards the plan of bv_group_verify_events: 64-aligned event
//                        shards and each shard's range of parent hashes;
//   bv_plan_event_fields_shards  the plan of bv_group_verify_events_itx /
//                        _fields: that plan, and the ITXs and block
//                        signatures each shard's events own;
//   bv_plan_block_shards the plan of bv_group_verify_blocks: bv_plan_group's
//                        item shards and message partition over the blocks.
//
// Pure C++ so the same source links into the ASan/UBSan fuzz harnesses
// (tests/hostfuzz, tests/hostfuzz_events) and into libbabbleverify.so.
#include "hostplan.h"

#include <algorithm>
#include <cstring>

// Contiguous item ranges balanced by count, cut only where the next item
// names a different message than the previous one (message-aligned), so the
// items of one message are never split.  Empty shards are allowed.
extern "C" int bv_plan_shards(const bv_batch *b, int n_shards, uint64_t *bounds) {
  if (!b || n_shards <= 0 || !bounds) return BV_E_ARGS;
  const uint64_t n = b->n_items;
  if (n && !b->item_msg) return BV_E_ARGS;
  bounds[0] = 0;
  for (int g = 1; g < n_shards; g++) {
    uint64_t c = std::max<uint64_t>(bounds[g - 1], (uint64_t)((__uint128_t)n * g / n_shards));
    while (c > 0 && c < n && b->item_msg[c] == b->item_msg[c - 1]) c++;
    bounds[g] = std::min(c, n);
  }
  bounds[n_shards] = n;
  return BV_OK;
}

// The global accept bitmask from the all-gathered shard bitmasks: shard d's
// words start at gathered[d * words_per_shard], its bit 0 is item bounds[d].
// Bits past a shard's item count are ignored (the device pads with zeros, but
// the merge does not rely on it).  Host only.
extern "C" int bv_merge_shard_bits(const uint64_t *gathered, uint64_t words_per_shard, int n_shards,
                                   const uint64_t *bounds, uint64_t *out) {
  if (!bounds || n_shards <= 0 || bounds[0] != 0) return BV_E_ARGS;
  const uint64_t n_items = bounds[n_shards];
  for (int d = 0; d < n_shards; d++)
    if (bounds[d] > bounds[d + 1] || (bounds[d + 1] - bounds[d] + 63) / 64 > words_per_shard) return BV_E_ARGS;
  if (n_items == 0) return BV_OK;
  if (!gathered || !out) return BV_E_ARGS;
  const uint64_t W = (n_items + 63) / 64;
  memset(out, 0, W * 8);
  for (int d = 0; d < n_shards; d++) {
    const uint64_t a = bounds[d], n = bounds[d + 1] - a;
    const uint64_t *src = gathered + (uint64_t)d * words_per_shard;
    const uint64_t q0 = a / 64, s = a % 64;
    for (uint64_t w = 0; w < (n + 63) / 64; w++) {
      uint64_t v = src[w];
      const uint64_t valid = std::min<uint64_t>(64, n - 64 * w);
      if (valid < 64) v &= (1ull << valid) - 1;
      out[q0 + w] |= v << s;
      if (s && q0 + w + 1 < W) out[q0 + w + 1] |= v >> (64 - s);
    }
  }
  return BV_OK;
}

// The plan of bv_group_verify_events.  Bulk batches (no BV_PARENT_EVENT
// parent): contiguous event shards of whole 64-event words (the rule of
// babble_amd/shard.py shard_bounds: ceil(words / n_shards) words each, the
// last non-empty shard ends at n, trailing shards may be empty), and per
// shard the range [hash_lo, hash_hi) of parent hashes its BV_PARENT_HASH
// parents name (0, 0 without one).  A batch with in-batch parents stays whole
// on shard 0: bounds {0, n, n, ...}, returns 1.
extern "C" int bv_plan_event_shards(const bv_event_batch *b, int n_shards, uint64_t *event_bounds, uint64_t *hash_lo,
                                    uint64_t *hash_hi) {
  if (!b || n_shards <= 0 || !event_bounds || !hash_lo || !hash_hi) return BV_E_ARGS;
  const uint64_t n = b->n_events;
  if (n && (!b->parent_kind || !b->parent_ref)) return BV_E_ARGS;
  const bool dag = n && memchr(b->parent_kind, BV_PARENT_EVENT, 2 * n) != nullptr;
  plan_event_bounds(n, n_shards, dag, event_bounds);
  for (int d = 0; d < n_shards; d++)
    if (!event_hash_range(b, event_bounds[d], event_bounds[d + 1], &hash_lo[d], &hash_hi[d])) return BV_E_ARGS;
  return dag ? 1 : 0;
}

// The plan of bv_group_verify_events_itx / _fields: bv_plan_event_shards' event
// bounds and hash ranges (shards balanced by events, not items: ITXs are
// rare), and what else a shard owns, read off the batch's own start arrays at
// those bounds.
extern "C" int bv_plan_event_fields_shards(const bv_event_fields_batch *f, int n_shards, uint64_t *event_bounds,
                                           uint64_t *itx_bounds, uint64_t *bsig_bounds, uint64_t *hash_lo,
                                           uint64_t *hash_hi) {
  if (!f || !itx_bounds || !bsig_bounds) return BV_E_ARGS;
  const int rc = bv_plan_event_shards(&f->ev.events, n_shards, event_bounds, hash_lo, hash_hi);
  if (rc < 0) return rc;
  if (f->ev.events.n_events && !f->bsig_start) return BV_E_ARGS;
  for (int d = 0; d <= n_shards; d++) {
    itx_bounds[d] = f->ev.itx_start ? f->ev.itx_start[event_bounds[d]] : 0;
    bsig_bounds[d] = f->bsig_start ? f->bsig_start[event_bounds[d]] : 0;
  }
  return rc;
}

void plan_event_bounds(uint64_t n, int D, bool dag, uint64_t *bounds) {
  const uint64_t per = dag ? n : ((n + 63) / 64 + D - 1) / D * 64;
  for (int d = 0; d <= D; d++) bounds[d] = (uint64_t)std::min<__uint128_t>(n, (__uint128_t)d * per);
}

bool event_hash_range(const bv_event_batch *b, uint64_t a, uint64_t z, uint64_t *lo_out, uint64_t *hi_out) {
  uint64_t lo = UINT64_MAX, hi = 0;
  for (uint64_t i = 2 * a; i < 2 * z; i++) {
    if (b->parent_kind[i] > BV_PARENT_EVENT) return false;
    if (b->parent_kind[i] != BV_PARENT_HASH) continue;
    const uint64_t r = b->parent_ref[i];
    if (r >= b->n_parent_hashes) return false;
    lo = std::min(lo, r);
    hi = std::max(hi, r + 1);
  }
  *lo_out = hi ? lo : 0;
  *hi_out = hi;
  return true;
}

static bool items_in_message_order(const bv_batch *b) {
  for (uint64_t i = 1; i < b->n_items; i++)
    if (b->item_msg[i] < b->item_msg[i - 1]) return false;
  return true;
}

// One group call's host-side plan: items in message order (a stable counting
// sort when the caller's item_msg is not non-decreasing), message-aligned item
// shards, and a PARTITION of the messages [0, n_msgs) into contiguous device
// ranges — every message is hashed exactly once, including messages no item
// references (bv_verify_batch writes every digest too).
void plan_group(const bv_batch *b, int D, GroupPlan &p, bv_batch &sorted, int in_order) {
  sorted = *b;
  p.permuted = in_order < 0 ? !items_in_message_order(b) : in_order == 0;
  if (p.permuted) {
    const uint64_t n = b->n_items, M = b->n_msgs;
    std::vector<uint64_t> cnt(M + 1, 0);
    for (uint64_t i = 0; i < n; i++) cnt[b->item_msg[i] + 1]++;
    for (uint64_t m = 0; m < M; m++) cnt[m + 1] += cnt[m];
    p.perm.resize(n);
    for (uint64_t i = 0; i < n; i++) p.perm[cnt[b->item_msg[i]]++] = (uint32_t)i;
    p.s_msg.resize(n);
    p.s_key.resize(n);
    p.s_r.resize(32 * n);
    p.s_s.resize(32 * n);
    if (b->pre) p.s_pre.resize(n);
    for (uint64_t j = 0; j < n; j++) {
      const uint64_t i = p.perm[j];
      p.s_msg[j] = b->item_msg[i];
      p.s_key[j] = b->item_key[i];
      memcpy(&p.s_r[32 * j], b->r_be + 32 * i, 32);
      memcpy(&p.s_s[32 * j], b->s_be + 32 * i, 32);
      if (b->pre) p.s_pre[j] = b->pre[i];
    }
    sorted.item_msg = p.s_msg.data();
    sorted.item_key = p.s_key.data();
    sorted.r_be = p.s_r.data();
    sorted.s_be = p.s_s.data();
    sorted.pre = b->pre ? p.s_pre.data() : nullptr;
  }
  p.bounds.assign(D + 1, 0);
  bv_plan_shards(&sorted, D, p.bounds.data());
  // message cut d = the first message of item shard d (shards never split a
  // message, so shard d's items name messages in [cut d, cut d+1)); messages
  // before the first referenced one go to device 0, after the last to the
  // last device, between shards to the earlier shard
  p.mlo.assign(D, 0);
  p.mhi.assign(D, 0);
  uint64_t prev = 0;
  for (int d = 0; d < D; d++) {
    const uint64_t cut = d == 0 ? 0 : p.bounds[d] < b->n_items ? sorted.item_msg[p.bounds[d]] : b->n_msgs;
    p.mlo[d] = std::max(prev, cut);
    prev = p.mlo[d];
  }
  for (int d = 0; d < D; d++) p.mhi[d] = d + 1 < D ? p.mlo[d + 1] : b->n_msgs;
}

// The plan of bv_group_verify_blocks for item_block non-decreasing: plan_group
// over the items as bv_batch items with item_msg = item_block and n_msgs =
// n_blocks (no second rule).
void plan_block_bounds(const bv_block_batch *k, int D, uint64_t *block_bounds, uint64_t *item_bounds) {
  bv_batch v = {};
  v.n_msgs = k->n_blocks;
  v.n_items = k->n_items;
  v.item_msg = k->item_block;
  GroupPlan p;
  bv_batch sorted;
  plan_group(&v, D, p, sorted, 1);
  for (int d = 0; d <= D; d++) item_bounds[d] = p.bounds[d];
  for (int d = 0; d < D; d++) block_bounds[d] = p.mlo[d];
  block_bounds[D] = k->n_blocks;
}

void plan_blocks_whole(const bv_block_batch *k, int D, uint64_t *block_bounds, uint64_t *item_bounds) {
  block_bounds[0] = item_bounds[0] = 0;
  for (int d = 1; d <= D; d++) block_bounds[d] = k->n_blocks, item_bounds[d] = k->n_items;
}

extern "C" int bv_plan_block_shards(const bv_block_batch *k, int n_shards, uint64_t *block_bounds,
                                    uint64_t *item_bounds) {
  if (!k || n_shards <= 0 || !block_bounds || !item_bounds) return BV_E_ARGS;
  if (k->n_items && !k->item_block) return BV_E_ARGS;
  bool in_order = true;
  for (uint64_t i = 0; i < k->n_items; i++) {
    if (k->item_block[i] >= k->n_blocks) return BV_E_ARGS;
    if (i && k->item_block[i] < k->item_block[i - 1]) in_order = false;
  }
  if (!in_order) {
    plan_blocks_whole(k, n_shards, block_bounds, item_bounds);
    return 1;
  }
  plan_block_bounds(k, n_shards, block_bounds, item_bounds);
  return 0;
}

extern "C" int bv_plan_group(const bv_batch *b, int n_shards, uint64_t *item_bounds, uint64_t *msg_bounds,
                             uint32_t *perm) {
  if (!b || n_shards <= 0 || !item_bounds || !msg_bounds) return BV_E_ARGS;
  // the plan's permutation and sorted indices are u32 (item_msg is u32 too)
  if (b->n_items > UINT32_MAX || b->n_msgs > UINT32_MAX) return BV_E_ARGS;
  if (b->n_items && (!b->item_msg || !b->item_key || !b->r_be || !b->s_be)) return BV_E_ARGS;
  for (uint64_t i = 0; i < b->n_items; i++)
    if (b->item_msg[i] >= b->n_msgs) return BV_E_ARGS;
  GroupPlan p;
  bv_batch sorted;
  plan_group(b, n_shards, p, sorted);
  for (int d = 0; d <= n_shards; d++) item_bounds[d] = p.bounds[d];
  for (int d = 0; d < n_shards; d++) msg_bounds[d] = p.mlo[d];
  msg_bounds[n_shards] = b->n_msgs;
  if (perm)
    for (uint64_t j = 0; j < b->n_items; j++) perm[j] = p.permuted ? p.perm[j] : (uint32_t)j;
  return p.permuted ? 1 : 0;
}

