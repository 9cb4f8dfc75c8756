// hoststage.cpp — the staging planner (hoststage.h).
#include "hoststage.h"

size_t StagePlan::add(const void *src, size_t bytes, StageKind kind, size_t unit, size_t pad) {
  if (!src) bytes = 0;
  const size_t o = total;
  segs.push_back({(const uint8_t *)src, bytes, o, kind, unit});
  direct.push_back(0);
  total += align256(bytes + pad);
  return o;
}

size_t StagePlan::reserve(size_t bytes, size_t pad) {
  const size_t o = total;
  total += align256(bytes + pad);
  return o;
}

void StagePlan::mark_direct(bool (*pinned)(const void *, size_t)) {
  for (size_t i = 0; i < segs.size(); i++)
    direct[i] = segs[i].n && segs[i].n >= policy.direct_min && pinned(segs[i].src, segs[i].n);
}

void StagePlan::range(size_t a0, size_t a1, size_t piece, std::vector<StageOp> &ops) const {
  std::vector<StageOp> copies;
  for (size_t a = a0; a < a1;) {
    const size_t z = a1 - a > piece ? a + piece : a1;
    copies.clear();
    bool any_direct = false;
    size_t at = a;  // (merge_runs) the staged run not yet sent starts here
    std::vector<StageOp> dmas;
    for (size_t i = 0; i < segs.size(); i++) {
      const Seg &g = segs[i];
      const size_t lo = std::max(a, g.off), hi = std::min(z, g.off + g.n);
      if (lo >= hi) continue;
      const bool sliced = g.kind.form != S_ALL;
      if (!direct[i] && !sliced) {
        copies.push_back({StageOp::POOL_COPY, lo, g.src + (lo - g.off), hi - lo});
        continue;
      }
      if (policy.merge_runs) {  // a direct or sliced array ends the staged run before it
        if (lo > at) dmas.push_back({StageOp::DMA_STAGED, at, nullptr, lo - at});
        at = hi;
      }
      if (sliced) continue;
      any_direct = true;
      dmas.push_back({StageOp::DMA_CALLER, lo, g.src + (lo - g.off), hi - lo});
    }
    if (policy.merge_runs) {
      if (z > at) dmas.push_back({StageOp::DMA_STAGED, at, nullptr, z - at});
      ops.insert(ops.end(), copies.begin(), copies.end());
      ops.insert(ops.end(), dmas.begin(), dmas.end());
    } else {
      ops.insert(ops.end(), dmas.begin(), dmas.end());
      ops.insert(ops.end(), copies.begin(), copies.end());
      if (!any_direct) ops.push_back({StageOp::DMA_STAGED, a, nullptr, z - a});
      else
        for (const StageOp &c : copies) ops.push_back({StageOp::DMA_STAGED, c.off, nullptr, c.n});
    }
    a = z;
  }
}

void StagePlan::slice_range(const Seg &g, uint64_t e0, uint64_t e1, size_t *lo, size_t *hi) const {
  const Space &sp = space[g.kind.space];
  const uint64_t i0 = sp.start ? sp.start[e0] - sp.base : e0, i1 = sp.start ? sp.start[e1] - sp.base : e1;
  switch (g.kind.form) {
    case S_ALL: *lo = 0, *hi = g.n; break;
    case S_ELEM: *lo = i0 * g.unit, *hi = i1 * g.unit; break;
    case S_OFFS: *lo = i0 * g.unit, *hi = (i1 + 1) * g.unit; break;
    case S_BYTES:
      *lo = g.kind.through ? g.kind.through[i0] - g.kind.base : 0;
      *hi = g.kind.through ? g.kind.through[i1] - g.kind.base : 0;
      break;
  }
  *hi = std::min(*hi, g.n);
  *lo = std::min(*lo, *hi);
}

void StagePlan::slices(uint64_t e0, uint64_t e1, std::vector<StageOp> &ops) const {
  std::vector<StageOp> copies;
  for (size_t i = 0; i < segs.size(); i++) {
    const Seg &g = segs[i];
    if (g.kind.form == S_ALL || !g.n) continue;
    size_t lo, hi;
    slice_range(g, e0, e1, &lo, &hi);
    if (lo >= hi) continue;
    const StageOp op{direct[i] ? StageOp::DMA_CALLER : StageOp::POOL_COPY, g.off + lo, g.src + lo, hi - lo};
    (direct[i] ? ops : copies).push_back(op);
  }
  ops.insert(ops.end(), copies.begin(), copies.end());
  for (const StageOp &c : copies) ops.push_back({StageOp::DMA_STAGED, c.off, nullptr, c.n});
}
