// hoststage.h — how a host entry's arrays cross PCIe, planned on the host:
// the staging layout (one block, identical in pinned memory and in HBM), the
// copy commands that move a byte range of it, and the commands that move one
// event chunk's slices.  The drivers (bv_host_launch, bv_events_launch,
// bv_verify_blocks, the ITX / fields driver) say which arrays go in which
// phase; bv_stage_run (bv_api.cpp) issues the commands.  Host-only code: the
// plan is a list of offsets and lengths, checked on the CPU (tests/hostfuzz_stage).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------
// the staging planner
// ---------------------------------------------------------------------------
// What differs between the entries, chosen per entry (never per call).
struct StagePolicy {
  static constexpr size_t kNever = ~(size_t)0;
  // the smallest array that may be DMA'd from the caller's bv_host_alloc
  // memory instead of being copied into the staging block (kNever: none)
  size_t direct_min = 0;
  // false: with a direct array in a piece, every staged array of the piece
  // crosses as a copy of its own (its pad stays behind).  true: whatever lies
  // between the direct arrays crosses as one copy, pads and unplanned bytes
  // included, and the commands go in layout order behind the pool copies.
  bool merge_runs = false;
};

// How a segment splits over an event chunk [e0, e1).  S_ALL: it does not (it
// crosses whole, in a range); the others are sliced and left out of ranges.
enum StageForm : uint8_t {
  S_ALL,
  S_ELEM,   // `unit` bytes per element
  S_OFFS,   // an n + 1 offset array: elements i0 ..= i1
  S_BYTES,  // the bytes through[i0] .. through[i1] (no bytes when `through` is null)
};
// What indexes it: events, or the transactions / block signatures of the
// chunk's events (StagePlan::space: element of event e = start[e] - base).
enum StageSpace : uint8_t { S_EV, S_TX, S_BS };
struct StageKind {
  StageForm form = S_ALL;
  StageSpace space = S_EV;
  const uint64_t *through = nullptr;  // S_BYTES: the offset array, at the shard's first element
  uint64_t base = 0;                  // S_BYTES: the shard's first byte (the offsets are the whole batch's)
};

struct StageOp {
  enum Type : uint8_t { DMA_CALLER, POOL_COPY, DMA_STAGED } type;
  size_t off;          // layout offset written (pinned side for POOL_COPY, device side for the DMAs)
  const uint8_t *src;  // caller memory (null for DMA_STAGED: the staging block at `off`)
  size_t n;
};

struct StagePlan {
  struct Seg {
    const uint8_t *src;
    size_t n, off;
    StageKind kind;
    size_t unit;
  };
  struct Space {
    const uint64_t *start = nullptr;  // n_events + 1 entries at the shard's first event (null: the event index)
    uint64_t base = 0;
  };
  StagePolicy policy;
  std::vector<Seg> segs;
  std::vector<char> direct;  // per segment: DMA'd from where it lies (mark_direct)
  Space space[3];
  size_t total = 0;

  explicit StagePlan(StagePolicy p = {}) : policy(p) {}
  // The next segment: its layout offset.  A null src or zero bytes makes an
  // empty segment that still takes its place (of align256(pad) bytes).
  size_t add(const void *src, size_t bytes, StageKind kind = {}, size_t unit = 1, size_t pad = 0);
  // Layout bytes nothing is planned into (the driver fills them, or the device does)
  size_t reserve(size_t bytes, size_t pad = 0);
  // direct[i] for every segment of at least policy.direct_min bytes that `pinned` says lies in bv_host_alloc memory
  void mark_direct(bool (*pinned)(const void *, size_t));
  // The commands that move layout bytes [a0, a1) in pieces of `piece` bytes.
  // Per piece: the DMAs from caller memory, the pool copies, then the staged
  // DMAs: one for the whole piece when nothing in it is direct, else one per
  // pool copy (policy.merge_runs: see there).  Sliced segments are left out.
  void range(size_t a0, size_t a1, size_t piece, std::vector<StageOp> &ops) const;
  // The byte range of sliced segment g that events [e0, e1) need
  void slice_range(const Seg &g, uint64_t e0, uint64_t e1, size_t *lo, size_t *hi) const;
  // The commands that move every sliced segment's part of events [e0, e1):
  // DMAs from caller memory, the pool copies, then one staged DMA per copy
  void slices(uint64_t e0, uint64_t e1, std::vector<StageOp> &ops) const;
};
