// Driver for the staging planner (babble_amd/csrc/hoststage.cpp) and the host
// helpers of hostdag.cpp (bv_dag_levels, bv_check_event_fields) under
// AddressSanitizer + UBSan (test infrastructure only; host code, no device).
// Every source array is an exactly-sized heap buffer and every planned command
// is carried out with memcpy, so a command that reads or writes out of bounds
// aborts the run.  One case per input line:
//   R <merge> <piece> <a0> <a1> <n_seg> {<bytes> <pad> <flag>}   flag: 0 staged, 1 direct, 2 sliced
//     -> R <total> then the commands in order: D<off>:<seg>+<src off>:<n> (DMA from caller memory),
//        C<off>:<seg>+<src off>:<n> (pool copy into staging), S<off>:<n> (DMA from staging)
//   M <direct_min> {<bytes>}      mark_direct with everything pinned (direct_min -1: never) -> M <flags>
//   F <seed> <count>              random layouts, flags, piece sizes and cuts: the range plan's properties
//   L                             the slice plan's scenarios
//   G                             bv_dag_levels against its restatement
//   V                             bv_check_event_fields with and without a pool -> V <name> <without> <with> ...
// F, L and G print "<op> ok <cases>" or the first property that failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/hostdag.h"
#include "../../babble_amd/csrc/hoststage.h"

namespace {

uint8_t *exact(size_t n, uint8_t seed) {  // exactly n bytes on the heap (never NULL), a pattern that differs per array
  uint8_t *p = (uint8_t *)malloc(n ? n : 1);
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(seed * 37 + i * 11 + (i >> 8));
  return p;
}

struct Layout {
  StagePlan plan;
  std::vector<uint8_t *> bufs;
  explicit Layout(StagePolicy p) : plan(p) {}
  ~Layout() {
    for (uint8_t *b : bufs) free(b);
  }
  void seg(size_t bytes, size_t pad, int flag, bool null_src = false) {
    uint8_t *b = null_src ? nullptr : exact(bytes, (uint8_t)bufs.size());
    bufs.push_back(b);
    plan.add(b, bytes, flag == 2 ? StageKind{S_ELEM, S_EV} : StageKind{}, 1, pad);
    plan.direct.back() = flag == 1 && b && bytes;
  }
  int seg_of(const uint8_t *src, size_t n, size_t *so) const {  // the segment whose buffer holds [src, src + n)
    for (size_t i = 0; i < plan.segs.size(); i++) {
      const StagePlan::Seg &g = plan.segs[i];
      if (g.n && src >= g.src && src + n <= g.src + g.n) {
        *so = src - g.src;
        return (int)i;
      }
    }
    return -1;
  }
};

void print_ops(const Layout &L, const std::vector<StageOp> &ops) {
  for (const StageOp &op : ops) {
    if (op.type == StageOp::DMA_STAGED) {
      printf(" S%zu:%zu", op.off, op.n);
      continue;
    }
    size_t so = 0;
    const int s = L.seg_of(op.src, op.n, &so);
    printf(" %c%zu:%d+%zu:%zu", op.type == StageOp::DMA_CALLER ? 'D' : 'C', op.off, s, so, op.n);
  }
}

#define REQUIRE(cond, ...)            \
  do {                                \
    if (!(cond)) {                    \
      char _b[512];                   \
      snprintf(_b, sizeof _b, __VA_ARGS__); \
      return std::string(_b);         \
    }                                 \
  } while (0)

// Carries the commands out over real buffers and checks the range plan's properties.
std::string check_range(const Layout &L, size_t a0, size_t a1, size_t piece) {
  const StagePlan &P = L.plan;
  std::vector<StageOp> ops;
  P.range(a0, a1, piece, ops);
  const size_t T = P.total;
  std::vector<uint8_t> pin(T, 0xEE), dev(T, 0xDD);
  std::vector<int> in_pin(T, 0), in_dev(T, 0);
  auto piece_of = [&](size_t off) { return (off - a0) / piece; };
  const size_t n_pieces = a1 > a0 ? (a1 - a0 + piece - 1) / piece : 0;
  std::vector<int> staged(n_pieces, 0), dmas(n_pieces, 0), last_type(n_pieces, -1);
  std::vector<size_t> staged_end(n_pieces, ~(size_t)0), last_dma_off(n_pieces, 0);
  size_t last_piece = 0;
  for (const StageOp &op : ops) {
    REQUIRE(op.n > 0, "an empty command at %zu", op.off);
    REQUIRE(op.off >= a0 && op.off + op.n <= a1 && op.off + op.n <= T, "command [%zu, +%zu) outside [%zu, %zu)", op.off,
            op.n, a0, a1);
    const size_t pc = piece_of(op.off);
    REQUIRE(piece_of(op.off + op.n - 1) == pc, "command [%zu, +%zu) crosses a piece boundary", op.off, op.n);
    REQUIRE(pc >= last_piece, "piece %zu after piece %zu", pc, last_piece);
    last_piece = pc;
    // order within a piece: piece by piece D, C, S; merging C, then the DMAs in layout order
    const int rank = P.policy.merge_runs ? (op.type == StageOp::POOL_COPY ? 0 : 1)
                                         : (op.type == StageOp::DMA_CALLER ? 0 : op.type == StageOp::POOL_COPY ? 1 : 2);
    REQUIRE(rank >= last_type[pc], "command order in piece %zu", pc);
    last_type[pc] = rank;
    if (op.type != StageOp::POOL_COPY) {
      if (P.policy.merge_runs) REQUIRE(dmas[pc] == 0 || op.off >= last_dma_off[pc], "DMAs out of layout order");
      last_dma_off[pc] = op.off;
      dmas[pc]++;
    }
    if (op.type == StageOp::DMA_STAGED) {
      if (P.policy.merge_runs) REQUIRE(staged_end[pc] != op.off, "two adjacent staged DMAs meet at %zu", op.off);
      staged_end[pc] = op.off + op.n;
      staged[pc]++;
      memcpy(dev.data() + op.off, pin.data() + op.off, op.n);
      for (size_t j = 0; j < op.n; j++) in_dev[op.off + j]++;
      continue;
    }
    size_t so = 0;
    const int s = L.seg_of(op.src, op.n, &so);
    REQUIRE(s >= 0, "a source outside every array (to %zu)", op.off);
    const StagePlan::Seg &g = P.segs[s];
    REQUIRE(g.off + so == op.off, "segment %d byte %zu sent to %zu", s, so, op.off);
    REQUIRE(g.kind.form == S_ALL, "sliced segment %d in a range", s);
    REQUIRE((op.type == StageOp::DMA_CALLER) == (bool)P.direct[s], "segment %d by the wrong route", s);
    if (op.type == StageOp::DMA_CALLER) {
      memcpy(dev.data() + op.off, op.src, op.n);
      for (size_t j = 0; j < op.n; j++) in_dev[op.off + j]++;
    } else {
      memcpy(pin.data() + op.off, op.src, op.n);
      for (size_t j = 0; j < op.n; j++) in_pin[op.off + j]++;
    }
  }
  // every byte of every non-empty whole segment inside the range: on the device once, from its source
  std::vector<int> hits(n_pieces, 0), direct_in(n_pieces, 0), holes(n_pieces, 0);
  for (size_t i = 0; i < P.segs.size(); i++) {
    const StagePlan::Seg &g = P.segs[i];
    const size_t lo = std::max(a0, g.off), hi = std::min(a1, g.off + g.n);
    for (size_t o = lo; o < hi; o++) {
      if (g.kind.form != S_ALL) {
        REQUIRE(in_pin[o] == 0, "sliced segment %zu copied in a range", i);
        if (P.policy.merge_runs) REQUIRE(in_dev[o] == 0, "sliced segment %zu sent in a merged run", i);
        continue;
      }
      REQUIRE(in_dev[o] == 1, "segment %zu byte %zu reached the device %d times", i, o - g.off, in_dev[o]);
      REQUIRE(in_pin[o] == (P.direct[i] ? 0 : 1), "segment %zu byte %zu staged %d times", i, o - g.off, in_pin[o]);
      REQUIRE(dev[o] == g.src[o - g.off], "segment %zu byte %zu arrived wrong", i, o - g.off);
    }
    for (size_t pc = 0; pc < n_pieces && lo < hi; pc++) {
      const size_t pa = a0 + pc * piece, pz = std::min(a1, pa + piece);
      if (std::max(lo, pa) >= std::min(hi, pz)) continue;
      if (g.kind.form != S_ALL) holes[pc]++;
      else hits[pc]++, direct_in[pc] += P.direct[i];
    }
  }
  for (size_t pc = 0; pc < n_pieces; pc++) {
    if (!direct_in[pc] && (!P.policy.merge_runs || !holes[pc]))
      REQUIRE(staged[pc] == 1 && dmas[pc] == 1, "piece %zu without direct arrays: %d staged DMAs", pc, staged[pc]);
    if (direct_in[pc] && !P.policy.merge_runs)
      REQUIRE(dmas[pc] == hits[pc], "piece %zu: %d DMAs for %d segment parts", pc, dmas[pc], hits[pc]);
  }
  return "";
}

std::string fuzz(uint64_t seed, int count) {
  std::mt19937_64 rng(seed);
  auto R = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  for (int t = 0; t < count; t++) {
    StagePolicy pol;
    pol.merge_runs = t % 2;
    Layout L(pol);
    const int nseg = (int)R(1, 9);
    std::vector<size_t> cuts{0};
    const int direct_pct = (int)R(0, 2) * 40;  // none, some, most
    for (int i = 0; i < nseg; i++) {
      const uint64_t k = R(0, 5);
      const size_t bytes = k == 0 ? 0 : k == 1 ? R(1, 300) : k == 2 ? 256 * R(1, 8) : R(1, 20000);
      const bool sliced = R(0, 9) == 0;
      L.seg(bytes, R(0, 1) * 64, sliced ? 2 : (int)R(0, 99) < direct_pct ? 1 : 0, R(0, 11) == 0);
      cuts.push_back(L.plan.total);  // the phase ends
    }
    const size_t T = L.plan.total;
    if (!T) continue;
    size_t a0 = R(0, 2) ? cuts[R(0, cuts.size() - 1)] : R(0, T), a1 = R(0, 2) ? cuts[R(0, cuts.size() - 1)] : R(0, T);
    if (a0 > a1) std::swap(a0, a1);
    const uint64_t pk = R(0, 3);
    const size_t piece = pk == 0 ? R(1, 700) : pk == 1 ? 4096 : pk == 2 ? R(701, 30000) : (a1 - a0 ? a1 - a0 : 1);
    const std::string why = check_range(L, a0, a1, piece);
    if (!why.empty()) {
      char b[160];
      snprintf(b, sizeof b, " (case %d: merge %d, [%zu, %zu) of %zu in pieces of %zu)", t, (int)pol.merge_runs, a0, a1, T,
               piece);
      return why + b;
    }
  }
  return "";
}

// ---------------------------------------------------------------------------
// the slice plan
// ---------------------------------------------------------------------------
struct U64 {  // an exactly-sized uint64_t array
  uint64_t *p;
  size_t n;
  explicit U64(size_t n_) : p((uint64_t *)malloc(n_ ? n_ * 8 : 1)), n(n_) {}
  ~U64() { free(p); }
};

// N events of a whole batch, of which the shard [a, z) is planned as
// bv_events_launch does (pointers at the shard's first elements, the values in
// the offset arrays the whole batch's), in chunks of `chunk` events.
// no_tx: no event has a transaction; no_frag: the fragment arrays are absent.
std::string slice_case(uint64_t N, uint64_t a, uint64_t z, uint64_t chunk, bool no_tx, bool no_frag, uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto R = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  const uint64_t n = z - a;
  U64 tx_start(N + 1), bs_start(N + 1), frag_off(N + 1);
  tx_start.p[0] = bs_start.p[0] = frag_off.p[0] = 0;
  for (uint64_t e = 0; e < N; e++) {
    // no transactions right before and after every chunk edge of the shard
    const bool edge = e >= a && ((e - a) % chunk == 0 || (e - a) % chunk == chunk - 1);
    tx_start.p[e + 1] = tx_start.p[e] + (no_tx || edge ? 0 : R(0, 3));
    bs_start.p[e + 1] = bs_start.p[e] + R(0, 2);
    frag_off.p[e + 1] = frag_off.p[e] + (R(0, 3) ? 0 : R(1, 40));
  }
  const uint64_t NT = tx_start.p[N], NB = bs_start.p[N];
  U64 tx_off(NT + 1), bs_off(NB + 1);
  tx_off.p[0] = bs_off.p[0] = 0;
  for (uint64_t t = 0; t < NT; t++) tx_off.p[t + 1] = tx_off.p[t] + R(0, 50);
  for (uint64_t j = 0; j < NB; j++) bs_off.p[j + 1] = bs_off.p[j] + R(1, 90);
  // the shard's bases and counts
  const uint64_t b_tx = tx_start.p[a], b_bs = bs_start.p[a], n_tx = tx_start.p[z] - b_tx, n_bs = bs_start.p[z] - b_bs;
  const uint64_t b_txb = NT ? tx_off.p[b_tx] : 0, b_bsb = bs_off.p[b_bs], b_fr = frag_off.p[a];
  const uint64_t tx_len = n_tx ? tx_off.p[b_tx + n_tx] - b_txb : 0, bs_len = bs_off.p[b_bs + n_bs] - b_bsb;
  const uint64_t fr_len = no_frag ? 0 : frag_off.p[z] - b_fr;
  if (a) REQUIRE((b_tx && b_txb || no_tx) && b_bs && b_bsb && b_fr, "one of the shard's bases is 0");

  StagePlan P;
  P.space[S_TX] = {tx_start.p + a, b_tx};
  P.space[S_BS] = {bs_start.p + a, b_bs};
  std::vector<uint8_t *> bufs;
  std::vector<const char *> names;
  auto add = [&](const char *name, size_t bytes, StageKind k, size_t unit, const void *src_or_null, size_t pad = 0) {
    uint8_t *b = src_or_null ? exact(bytes, (uint8_t)bufs.size()) : nullptr;
    bufs.push_back(b);
    names.push_back(name);
    P.add(b, bytes, k, unit, pad);
    P.direct.back() = b && bytes && bufs.size() % 3 == 0;  // every third array lies in pinned memory
  };
  const void *yes = &P;
  add("keys", 100, {}, 1, yes, 64);  // a whole segment ahead of the sliced ones: never in a slice
  add("index", n * 8, {S_ELEM, S_EV}, 8, yes);
  add("parent_kind", n * 2, {S_ELEM, S_EV}, 2, yes);
  add("tx_start", (n + 1) * 8, {S_OFFS, S_EV}, 8, yes);
  add("tx_off", n_tx ? (n_tx + 1) * 8 : 0, {S_OFFS, S_TX}, 8, yes);
  add("tx_bytes", tx_len, {S_BYTES, S_TX, n_tx ? tx_off.p + b_tx : nullptr, b_txb}, 1, yes, 64);
  add("tx_nil", n_tx, {S_ELEM, S_TX}, 1, yes);
  add("frag_off", (n + 1) * 8, {S_OFFS, S_EV}, 8, no_frag ? nullptr : yes);
  add("frag", fr_len, {S_BYTES, S_EV, no_frag ? nullptr : frag_off.p + a, b_fr}, 1, no_frag ? nullptr : yes);
  add("bsig_index", n_bs * 8, {S_ELEM, S_BS}, 8, yes);
  add("bsig_sig_off", (n_bs + 1) * 8, {S_OFFS, S_BS}, 8, yes);
  add("bsig_sig", bs_len, {S_BYTES, S_BS, bs_off.p + b_bs, b_bsb}, 1, yes, 64);

  const size_t T = P.total;
  std::vector<uint8_t> pin(T, 0xEE), dev(T, 0xDD);
  std::vector<size_t> prev_hi(P.segs.size(), 0);
  std::vector<char> seen(P.segs.size(), 0);
  std::string why;
  for (uint64_t e0 = 0; e0 < n && why.empty(); e0 += chunk) {
    const uint64_t e1 = std::min(n, e0 + chunk);
    for (size_t i = 1; i < P.segs.size(); i++) {  // the byte ranges: they tile each segment
      const StagePlan::Seg &g = P.segs[i];
      size_t lo, hi;
      P.slice_range(g, e0, e1, &lo, &hi);
      if (hi > g.n) why = std::string(names[i]) + ": a range past the segment's end";
      if (lo >= hi) continue;
      const size_t shared = g.kind.form == S_OFFS ? g.unit : 0;  // an n + 1 array's chunks share one element
      if (seen[i] ? lo + shared != prev_hi[i] : lo != 0) why = std::string(names[i]) + ": chunks overlap or leave a gap";
      seen[i] = 1;
      prev_hi[i] = hi;
    }
    std::vector<StageOp> ops;
    P.slices(e0, e1, ops);
    for (const StageOp &op : ops) {  // carried out: sources and destinations in bounds (ASan), copies before their DMA
      if (op.off + op.n > T) return "a slice command outside the layout";
      if (op.type == StageOp::POOL_COPY) memcpy(pin.data() + op.off, op.src, op.n);
      else memcpy(dev.data() + op.off, op.type == StageOp::DMA_CALLER ? op.src : pin.data() + op.off, op.n);
    }
  }
  for (size_t i = 1; i < P.segs.size() && why.empty(); i++) {
    const StagePlan::Seg &g = P.segs[i];
    if (g.n && (!seen[i] || prev_hi[i] != g.n)) why = std::string(names[i]) + ": the chunks do not cover the segment";
    if (g.n && memcmp(dev.data() + g.off, g.src, g.n)) why = std::string(names[i]) + ": arrived wrong";
  }
  if (dev[0] != 0xDD) why = "a whole segment crossed in a slice";
  for (uint8_t *b : bufs) free(b);
  return why;
}

std::string slice_cases(int *count) {
  struct {
    uint64_t N, a, z, chunk;
  } shapes[] = {{600, 0, 600, 256}, {200, 0, 200, 64}, {900, 192, 792, 256}, {300, 64, 264, 64}};
  for (auto &s : shapes)
    for (int no_tx = 0; no_tx < 2; no_tx++)
      for (int no_frag = 0; no_frag < 2; no_frag++)
        for (uint64_t seed = 1; seed <= 3; seed++) {
          const std::string why = slice_case(s.N, s.a, s.z, s.chunk, no_tx, no_frag, seed);
          if (!why.empty()) {
            char b[160];
            snprintf(b, sizeof b, " (%llu events [%llu, %llu) in chunks of %llu, no_tx %d, no_frag %d, seed %llu)",
                     (unsigned long long)s.N, (unsigned long long)s.a, (unsigned long long)s.z,
                     (unsigned long long)s.chunk, no_tx, no_frag, (unsigned long long)seed);
            return why + b;
          }
          ++*count;
        }
  return "";
}

// ---------------------------------------------------------------------------
// bv_dag_levels, bv_check_event_fields
// ---------------------------------------------------------------------------
std::string dag_case(const std::vector<uint8_t> &kind, const std::vector<uint64_t> &ref) {
  const uint64_t n = kind.size() / 2;
  uint8_t *k = (uint8_t *)malloc(2 * n + 1);
  uint64_t *r = (uint64_t *)malloc(16 * n + 1);
  memcpy(k, kind.data(), 2 * n);
  memcpy(r, ref.data(), 16 * n);
  bv_event_batch b = {};
  b.n_events = n;
  b.parent_kind = k;
  b.parent_ref = r;
  std::vector<uint32_t> order, level_off;
  bv_dag_levels(b, order, level_off);
  free(k);
  free(r);
  // the restatement: an event's level is one more than its highest in-batch
  // parent's; `order` lists the events level by level, in batch order within one
  std::vector<uint32_t> lv(n, 0), want_order, want_off{0};
  uint32_t top = 0;
  for (uint64_t e = 0; e < n; e++) {
    for (int p = 0; p < 2; p++)
      if (kind[2 * e + p] == BV_PARENT_EVENT) lv[e] = std::max(lv[e], lv[ref[2 * e + p]] + 1);
    top = std::max(top, lv[e]);
  }
  for (uint32_t l = 0; l <= top; l++) {
    for (uint64_t e = 0; e < n; e++)
      if (lv[e] == l) want_order.push_back((uint32_t)e);
    want_off.push_back((uint32_t)want_order.size());
  }
  if (order != want_order) return "order differs";
  if (level_off != want_off) return "level_off differs";
  return "";
}

std::string dag_cases(int *count) {
  auto run = [&](const char *name, const std::vector<uint8_t> &k, const std::vector<uint64_t> &r) {
    const std::string why = dag_case(k, r);
    ++*count;
    return why.empty() ? why : why + " (" + name + ")";
  };
  std::string why;
  for (uint64_t n : {1ull, 2ull, 7ull, 300ull}) {  // chains: each event's self-parent is the one before it
    std::vector<uint8_t> k(2 * n, BV_PARENT_NONE);
    std::vector<uint64_t> r(2 * n, 0);
    for (uint64_t e = 1; e < n; e++) k[2 * e] = BV_PARENT_EVENT, r[2 * e] = e - 1;
    if (!(why = run("chain", k, r)).empty()) return why;
  }
  {  // 64 events of 4 creators gossiping: self-parent, and the latest event of another creator
    std::mt19937_64 rng(5);
    std::vector<uint8_t> k(128, BV_PARENT_NONE);
    std::vector<uint64_t> r(128, 0);
    int64_t last[4] = {-1, -1, -1, -1};
    for (uint64_t e = 0; e < 64; e++) {
      const int c = (int)(rng() % 4), o = (c + 1 + (int)(rng() % 3)) % 4;
      if (last[c] >= 0) k[2 * e] = BV_PARENT_EVENT, r[2 * e] = (uint64_t)last[c];
      else k[2 * e] = BV_PARENT_HASH, r[2 * e] = (uint64_t)c;
      if (last[o] >= 0) k[2 * e + 1] = BV_PARENT_EVENT, r[2 * e + 1] = (uint64_t)last[o];
      last[c] = (int64_t)e;
    }
    if (!(why = run("gossip", k, r)).empty()) return why;
  }
  {  // no in-batch parent: one level
    std::vector<uint8_t> k(2 * 50, BV_PARENT_HASH);
    std::vector<uint64_t> r(2 * 50, 3);
    if (!(why = run("bulk", k, r)).empty()) return why;
  }
  return "";
}

// A valid batch of n events (2 keys, 0-2 transactions each, BlockSignature
// fragments, parents by hash), then one thing wrong at a time, near the end,
// where only a pool thread's range sees it (n is several grains long).
void check_cases() {
  const uint64_t n = 300000, nh = 5;
  std::vector<uint32_t> creator(n);
  std::vector<int64_t> index(n, 1), ts(n, 2);
  std::vector<uint8_t> kind(2 * n, BV_PARENT_HASH), hashes(nh * 32, 7), keys(130, 4), r_be(32 * n, 1), s_be(32 * n, 1);
  std::vector<uint64_t> ref(2 * n), tx_start(n + 1, 0), bsig_off(n + 1, 0), key_off{0, 65, 130};
  for (uint64_t e = 0; e < n; e++) {
    creator[e] = e & 1;
    ref[2 * e] = e % nh, ref[2 * e + 1] = (e + 1) % nh;
    tx_start[e + 1] = tx_start[e] + e % 3;
    bsig_off[e + 1] = bsig_off[e] + (e % 7 == 0 ? 9 : 0);
  }
  std::vector<uint64_t> tx_off(tx_start[n] + 1);
  for (size_t t = 0; t < tx_off.size(); t++) tx_off[t] = 10 * t;
  std::vector<uint8_t> tx_bytes(tx_off.back(), 3), bsig_json(bsig_off[n], '[');
  bv_event_batch good = {};
  good.n_events = n;
  good.creator = creator.data(), good.index = index.data(), good.timestamp = ts.data();
  good.parent_kind = kind.data(), good.parent_ref = ref.data();
  good.n_parent_hashes = nh, good.parent_hashes = hashes.data();
  good.tx_start = tx_start.data(), good.tx_off = tx_off.data(), good.tx_bytes = tx_bytes.data();
  good.bsig_off = bsig_off.data(), good.bsig_json = bsig_json.data();
  good.n_keys = 2, good.key_off = key_off.data(), good.key_bytes = keys.data();
  good.r_be = r_be.data(), good.s_be = s_be.data();
  CopyPool pool(3);
  const uint64_t e = n - 1000;
  auto verdicts = [&](const char *name, const bv_event_batch &b) {
    for (bool entry : {true, false})
      printf(" %s%s %d %d", name, entry ? "" : "/helper", bv_check_event_fields(&b, nullptr, entry) != nullptr,
             bv_check_event_fields(&b, &pool, entry) != nullptr);
  };
  printf("V");
  verdicts("valid", good);
  // (what tests/test_events.py builds: an EVENT parent that does not precede its child)
  kind[2 * e] = BV_PARENT_EVENT, ref[2 * e] = e + 2;
  verdicts("forward_reference", good);
  ref[2 * e] = e;
  verdicts("self_reference", good);
  ref[2 * e] = e - 1;
  verdicts("backward_reference", good);
  kind[2 * e] = 3;
  verdicts("parent_kind", good);
  kind[2 * e] = BV_PARENT_HASH, ref[2 * e] = nh;
  verdicts("hash_out_of_range", good);
  ref[2 * e] = 0;
  creator[e] = 2;
  verdicts("creator", good);
  creator[e] = 0;
  {
    bv_event_batch b = good;
    b.parent_hashes = nullptr;
    verdicts("null_parent_hashes", b);
    b = good, b.tx_off = nullptr;
    verdicts("null_tx_off", b);
    b = good, b.tx_bytes = nullptr;
    verdicts("null_tx_bytes", b);
    b = good, b.timestamp = nullptr;
    verdicts("null_timestamp", b);
    b = good, b.bsig_json = nullptr;
    verdicts("null_fragment_bytes", b);
    b = good, b.s_be = nullptr;  // (an entry's rule only)
    verdicts("null_s", b);
  }
  const uint64_t keep = tx_start[e];
  tx_start[e] = tx_start[e + 1] + 1;
  verdicts("tx_start_order", good);
  tx_start[e] = keep;
  const uint64_t t = tx_start[e], keep_t = tx_off[t];
  tx_off[t] = tx_off[t + 1] + 1;
  verdicts("tx_off_order", good);
  tx_off[t] = keep_t;
  tx_off[0] = 1;
  verdicts("tx_off_start", good);
  tx_off[0] = 0;
  bsig_off[e] += 100;
  verdicts("fragment_order", good);
  bsig_off[e] -= 100;
  key_off[1] = 200;
  verdicts("key_off_order", good);
  key_off[1] = 65;
  verdicts("valid_again", good);
  printf("\n");
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "R") {
      int merge = 0, nseg = 0;
      size_t piece = 0, a0 = 0, a1 = 0;
      in >> merge >> piece >> a0 >> a1 >> nseg;
      StagePolicy pol;
      pol.merge_runs = merge != 0;
      Layout L(pol);
      for (int i = 0; i < nseg; i++) {
        size_t bytes = 0, pad = 0;
        int flag = 0;
        in >> bytes >> pad >> flag;
        L.seg(bytes, pad, flag);
      }
      std::vector<StageOp> ops;
      L.plan.range(a0, a1, piece, ops);
      printf("R %zu", L.plan.total);
      print_ops(L, ops);
      const std::string why = check_range(L, a0, a1, piece);
      printf("%s%s\n", why.empty() ? "" : " FAIL ", why.c_str());
    } else if (op == "M") {
      long long dmin = 0;
      in >> dmin;
      StagePolicy pol;
      pol.direct_min = dmin < 0 ? StagePolicy::kNever : (size_t)dmin;
      Layout L(pol);
      size_t bytes;
      while (in >> bytes) L.seg(bytes, 0, 0);
      L.plan.mark_direct([](const void *, size_t) { return true; });
      printf("M ");
      for (char d : L.plan.direct) printf("%d", d);
      printf("\n");
    } else if (op == "F") {
      uint64_t seed = 0;
      int count = 0;
      in >> seed >> count;
      const std::string why = fuzz(seed, count);
      if (why.empty()) printf("F ok %d\n", count);
      else printf("F FAIL %s\n", why.c_str());
    } else if (op == "L" || op == "G") {
      int count = 0;
      const std::string why = op == "L" ? slice_cases(&count) : dag_cases(&count);
      if (why.empty()) printf("%s ok %d\n", op.c_str(), count);
      else printf("%s FAIL %s\n", op.c_str(), why.c_str());
    } else if (op == "V") {
      check_cases();
    }
  }
  return 0;
}
