// bsigjson.h — EventBody.BlockSignatures built from fields
// (bv_event_fields_batch, include/babbleverify.h), in the style of itxjson.h:
// __host__ __device__ templates over an output sink.  The device streams each
// body into SHA-256 (k_ev_body_hash_fields: EvjSha), the host writes it to
// memory (bv_event_fields_bodies, the in-batch DAG path, the one-launch small
// path) and the emulator (tests/emu_fields) runs the device's sink on the CPU.
//
// BlockSignature (src/hashgraph/block.go:59-66) under Go 1.13 encoding/json:
//   {"Validator":V,"Index":D,"Signature":S}
//   V  padded StdEncoding base64 in quotes (empty -> ""), nil -> null
//   D  decimal of a Go int
//   S  a Go string through encodeState.string, escapeHTML = true (gojson_string)
// The list is null (nil), [] or [e,e,...].  With these the whole of
// EventBody.Marshal comes from fields: evj_emit below takes no JSON from the
// caller (ev.events.itx_off and bsig_off are NULL).
#pragma once
#include "itxjson.h"

#define BSIG_L0 "{\"Validator\":"
#define BSIG_L1 ",\"Index\":"
#define BSIG_L2 ",\"Signature\":"

// Bases of a shard (bv_group_verify_events_fields), as EvjBases / ItxBases: the
// block-signature arrays of `f` are the slices one event range of a larger
// batch needs, and the values in bsig_start, bsig_sig_off and bsig_val_off are
// still the whole batch's.
//   bsig  bsig_start[a]: the per-signature arrays start at that signature
//   sig   bsig_sig_off[bsig]: bsig_sig starts at that byte
//   val   bsig_val_off[bsig] (0 when no entry is BV_BSIG_VAL_BYTES: the array
//         is not read then): bsig_val_bytes starts at that byte
// BsigNoBases (all zero, compile-time) is the whole batch.
struct BsigBases {
  uint64_t bsig, sig, val;
};
struct BsigNoBases {
  static constexpr uint64_t bsig = 0, sig = 0, val = 0;
};

DEV uint8_t bsig_val_kind(const bv_event_fields_batch &f, uint64_t j) {
  return f.bsig_val_kind ? f.bsig_val_kind[j] : (uint8_t)BV_BSIG_VAL_CREATOR;
}

// One element of EventBody.BlockSignatures: signature j, carried by event e.
// (Each Validator kind emits from its own array: on the device a pointer
// chosen per lane between two of the batch's arrays must not be formed, the
// array bases are wave-uniform values.  tests/test_gpu_event_fields.py runs
// CREATOR, BYTES and NIL entries side by side in one wave.)
template <class O, class B = BsigNoBases>
DEV void bsig_elem_emit(const bv_event_fields_batch &f, uint64_t e, uint64_t j, O &o, const B &bs = B{}) {
  const bv_event_batch &b = f.ev.events;
  const uint8_t kind = bsig_val_kind(f, j);
  evj_lit(o, BSIG_L0);
  if (kind == BV_BSIG_VAL_NIL) {
    evj_lit(o, "null");
  } else if (kind == BV_BSIG_VAL_BYTES) {
    o.put('"');
    evj_b64(o, f.bsig_val_bytes + (f.bsig_val_off[j] - bs.val), f.bsig_val_off[j + 1] - f.bsig_val_off[j]);
    o.put('"');
  } else {
    const uint32_t c = b.creator[e];
    o.put('"');
    evj_b64(o, b.key_bytes + b.key_off[c], b.key_off[c + 1] - b.key_off[c]);
    o.put('"');
  }
  evj_lit(o, BSIG_L1);
  evj_dec(o, f.bsig_index[j]);
  evj_lit(o, BSIG_L2);
  gojson_string(o, f.bsig_sig + (f.bsig_sig_off[j] - bs.sig), f.bsig_sig_off[j + 1] - f.bsig_sig_off[j]);
  o.put('}');
}

DEV uint64_t bsig_elem_len(const bv_event_fields_batch &f, uint64_t e, uint64_t j) {
  const bv_event_batch &b = f.ev.events;
  const uint8_t kind = bsig_val_kind(f, j);
  uint64_t n = EVJ_LEN(BSIG_L0) + EVJ_LEN(BSIG_L1) + EVJ_LEN(BSIG_L2) + 1;
  if (kind == BV_BSIG_VAL_NIL) {
    n += 4;
  } else if (kind == BV_BSIG_VAL_BYTES) {
    n += 2 + evj_b64_len(f.bsig_val_off[j + 1] - f.bsig_val_off[j]);
  } else {
    const uint32_t c = b.creator[e];
    n += 2 + evj_b64_len(b.key_off[c + 1] - b.key_off[c]);
  }
  n += evj_dec_len(f.bsig_index[j]);
  return n + gojson_string_len(f.bsig_sig + f.bsig_sig_off[j], f.bsig_sig_off[j + 1] - f.bsig_sig_off[j]);
}

DEV bool bsig_list_is_nil(const bv_event_fields_batch &f, uint64_t e) { return f.bsig_list_nil && f.bsig_list_nil[e]; }

DEV uint64_t bsig_list_len(const bv_event_fields_batch &f, uint64_t e) {
  if (bsig_list_is_nil(f, e)) return 4;
  const uint64_t j0 = f.bsig_start[e], j1 = f.bsig_start[e + 1];
  uint64_t n = 2 + (j1 > j0 ? j1 - j0 - 1 : 0);
  for (uint64_t j = j0; j < j1; j++) n += bsig_elem_len(f, e, j);
  return n;
}

template <class O, class B = BsigNoBases>
DEV void bsig_list_emit(const bv_event_fields_batch &f, uint64_t e, O &o, const B &bs = B{}) {
  if (bsig_list_is_nil(f, e)) {
    evj_lit(o, "null");
    return;
  }
  const uint64_t j0 = f.bsig_start[e] - bs.bsig, j1 = f.bsig_start[e + 1] - bs.bsig;
  o.put('[');
  for (uint64_t j = j0; j < j1; j++) {
    if (j > j0) o.put(',');
    bsig_elem_emit(f, e, j, o, bs);
  }
  o.put(']');
}

// The InternalTransactions member of a fields batch: itxjson.h's, or, for a
// batch without ITX fields (ev.itx_start == NULL), null unless itx_list_nil
// says the event's list is empty and not nil
DEV bool evf_itx_empty(const bv_event_fields_batch &f, uint64_t e) {
  return f.ev.itx_list_nil && f.ev.itx_list_nil[e] == 0;
}

// The evj_len / evj_emit variants: event e's body, every member from fields.
// ppos: as evj_len, after the ITX text and before the block signatures'.
DEV uint64_t evj_len(const bv_event_fields_batch &f, uint64_t e, uint32_t ppos[2]) {
  const bv_event_batch &b = f.ev.events;
  uint64_t n = evj_len_txs(b, e);
  n += f.ev.itx_start ? itx_list_len(f.ev, e) : (evf_itx_empty(f, e) ? 2 : 4);
  n = evj_len_mid(b, e, n, ppos);
  return evj_len_tail(b, e, n + bsig_list_len(f, e));
}

// (bs, ib, sb: a shard's bases; `e` is then the whole batch's index, as evj_emit's)
template <class O, class B = EvjNoBases, class IB = ItxNoBases, class SB = BsigNoBases>
DEV void evj_emit(const bv_event_fields_batch &f, uint64_t e, O &o, const B &bs = B{}, const IB &ib = IB{},
                  const SB &sb = SB{}) {
  const bv_event_batch &b = f.ev.events;
  e -= bs.ev;
  evj_emit_txs(b, e, o, bs);
  if (f.ev.itx_start) {
    itx_list_emit(f.ev, e, o, ib);
  } else {
    if (evf_itx_empty(f, e)) evj_lit(o, "[]");
    else evj_lit(o, "null");
  }
  evj_emit_mid(b, e, o, bs);
  bsig_list_emit(f, e, o, sb);
  evj_emit_tail(b, e, o);
}

DEV void evj_write(const bv_event_fields_batch &f, uint64_t e, uint8_t *o) {
  EvjMem m{o};
  evj_emit(f, e, m);
}

// The block-signature fields as the functions above read them: nullptr, or
// what is wrong (bv_verify_events_fields' BV_E_ARGS texts).  Host code;
// mono(off, n): off[0..n] does not decrease (the driver spreads that scan over
// its thread pool, the host helpers and the tests run it in place).
template <class Mono>
inline const char *bsig_check(const bv_event_fields_batch &f, const Mono &mono) {
  const bv_event_batch &eb = f.ev.events;
  const uint64_t n = eb.n_events;
  if (eb.bsig_off || eb.bsig_json)
    return "events.bsig_off / bsig_json must be NULL (the block signatures come from fields)";
  if (n > (1ull << 32)) return "more than 2^32 events";
  if (!n) return nullptr;
  if (!f.bsig_start) return "null bsig_start";
  if (f.bsig_start[0] != 0) return "bsig_start[0] != 0";
  if (!mono(f.bsig_start, n)) return "bsig_start not monotone";
  const uint64_t nb = f.bsig_start[n];
  if (nb > (1ull << 32)) return "more than 2^32 block signatures";
  if (!nb) return nullptr;
  if (!f.bsig_index) return "null bsig_index";
  if (!f.bsig_sig_off) return "null bsig_sig_off";
  if (f.bsig_sig_off[0] != 0) return "bsig_sig_off[0] != 0";
  if (!mono(f.bsig_sig_off, nb)) return "bsig_sig_off not monotone";
  if (f.bsig_sig_off[nb] && !f.bsig_sig) return "null bsig_sig";
  if (!f.bsig_val_kind) return nullptr;
  bool bytes = false;
  for (uint64_t j = 0; j < nb; j++) {
    if (f.bsig_val_kind[j] > BV_BSIG_VAL_NIL) return "bad bsig_val_kind";
    bytes |= f.bsig_val_kind[j] == BV_BSIG_VAL_BYTES;
  }
  if (!bytes) return nullptr;
  if (!f.bsig_val_off) return "null bsig_val_off";
  if (!mono(f.bsig_val_off, nb)) return "bsig_val_off not monotone";
  if (f.bsig_val_off[nb] && !f.bsig_val_bytes) return "null bsig_val_bytes";
  return nullptr;
}
