// hostplan.h — host-only planning of a multi-device group call (no HIP):
// item order, message-aligned item shards and the message partition
// (hostplan.cpp; used by bv_group.cpp, sanitized by tests/hostfuzz).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/babbleverify.h"

struct GroupPlan {
  std::vector<uint64_t> bounds, mlo, mhi;
  bool permuted = false;
  std::vector<uint32_t> perm;  // sorted position j -> caller's item index
  std::vector<uint32_t> s_msg, s_key;
  std::vector<uint8_t> s_r, s_s, s_pre, s_status;
  std::vector<uint64_t> s_bits;
};

// Fills `p` for `b` over D shards; `sorted` = b with its item arrays in the
// plan's order (p's own copies when permuted).  b's item_msg must be < n_msgs.
// `in_order`: whether item_msg is non-decreasing, when the caller already
// knows (-1: checked here).
void plan_group(const bv_batch *b, int D, GroupPlan &p, bv_batch &sorted, int in_order = -1);

// The two outcomes of bv_plan_block_shards, D + 1 block and item bounds each:
// plan_group over the blocks' items (item_block non-decreasing and < n_blocks,
// checked by the caller), or the whole batch on shard 0: {0, n, n, ...}.
void plan_block_bounds(const bv_block_batch *k, int D, uint64_t *block_bounds, uint64_t *item_bounds);
void plan_blocks_whole(const bv_block_batch *k, int D, uint64_t *block_bounds, uint64_t *item_bounds);

// The two halves of bv_plan_event_shards, for bv_group_verify_events (each
// shard's host thread finds its own hash range, in pieces on its copy pool).
// D + 1 event bounds: whole 64-event words per shard, or {0, n, n, ...} (dag).
void plan_event_bounds(uint64_t n, int D, bool dag, uint64_t *bounds);
// [lo, hi): from the smallest to the largest parent_ref among the
// BV_PARENT_HASH parents of events [a, z) (0, 0 without one); false on an
// unknown parent kind or a ref >= n_parent_hashes.
bool event_hash_range(const bv_event_batch *b, uint64_t a, uint64_t z, uint64_t *lo, uint64_t *hi);
