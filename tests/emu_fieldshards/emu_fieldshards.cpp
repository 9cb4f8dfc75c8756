// Host build of the rebased serialisers and the rebased fold
// (babble_amd/csrc/itxjson.h, bsigjson.h: itx_body_emit and the evj_emit
// variants with EvjBases / ItxBases / BsigBases, ev_fold with an ITX base):
// what k_itx_body_hash_rb, k_ev_body_hash_itx_rb, k_ev_body_hash_fields_rb and
// k_ev_compose_rb run per lane, given ONLY a shard's slices of a batch and the
// shard's bases.  Test infrastructure only (tests/test_event_fields_shards.py).
#include <cstdint>
#include <cstring>

#include "../../babble_amd/csrc/bsigjson.h"

namespace {
// bases: ev, tx, txb, ph (EvjBases; the fragment bases itx and bsig follow), itx, str (ItxBases), bsig, sig, val
// (BsigBases), then the two fragment bases
EvjBases evj_bases(const uint64_t b[11]) { return EvjBases{b[0], b[1], b[2], b[9], b[10], b[3]}; }
ItxBases itx_bases(const uint64_t b[11]) { return ItxBases{b[4], b[5]}; }
BsigBases bsig_bases(const uint64_t b[11]) { return BsigBases{b[6], b[7], b[8]}; }
}  // namespace

extern "C" {

// Digests of the shard's ITXs [0, n_itx) (the shard's own indices): digests + 32 * i
void emufs_itx_body_hash(const bv_event_itx_batch *x, uint64_t n_itx, const uint64_t bases[11], uint8_t *digests) {
  const ItxBases ib = itx_bases(bases);
  for (uint64_t i = 0; i < n_itx; i++) {
    uint32_t row[25], be[8];
    EvjSha o = evj_sha_begin(row);
    itx_body_emit(*x, i, o, ib);
    evj_sha_finish(o, be);
    memcpy(digests + 32 * i, be, 32);
  }
}

// Digests of events [e0, e1) (the whole batch's indices) of the shard whose
// slices are `x` (the ITX form: BlockSignatures as fragments): digests + 32 * (e - ev)
void emufs_ev_body_hash_itx(const bv_event_itx_batch *x, uint64_t e0, uint64_t e1, const uint64_t bases[11],
                            uint8_t *digests) {
  const EvjBases bs = evj_bases(bases);
  const ItxBases ib = itx_bases(bases);
  for (uint64_t e = e0; e < e1; e++) {
    uint32_t row[25], be[8];
    EvjSha o = evj_sha_begin(row);
    evj_emit(*x, e, o, bs, ib);
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (e - bs.ev), be, 32);
  }
}

// The same for the fields form (`f`: every member from fields)
void emufs_ev_body_hash_fields(const bv_event_fields_batch *f, uint64_t e0, uint64_t e1, const uint64_t bases[11],
                               uint8_t *digests) {
  const EvjBases bs = evj_bases(bases);
  const ItxBases ib = itx_bases(bases);
  const BsigBases sb = bsig_bases(bases);
  for (uint64_t e = e0; e < e1; e++) {
    uint32_t row[25], be[8];
    EvjSha o = evj_sha_begin(row);
    evj_emit(*f, e, o, bs, ib, sb);
    evj_sha_finish(o, be);
    memcpy(digests + 32 * (e - bs.ev), be, 32);
  }
}

// k_ev_compose_rb over a shard of n_ev events: itx_start is the shard's slice
// (the whole batch's values), every other array the shard's own; bits: one
// word per 64 events, as the kernel's ballot writes them
void emufs_compose(uint64_t n_ev, const uint64_t *itx_start, uint64_t itx_base, const uint8_t *item_status,
                   const uint8_t *force_panic, uint8_t *ev_status, uint32_t *decided_by, uint64_t *bits,
                   uint8_t *itx_status) {
  for (uint64_t w = 0; w < (n_ev + 63) / 64; w++) bits[w] = 0;
  for (uint64_t e = 0; e < n_ev; e++)
    if (ev_fold(n_ev, e, itx_start, itx_base, item_status, force_panic, ev_status, decided_by, itx_status))
      bits[e >> 6] |= 1ull << (e & 63);
}

}  // extern "C"
