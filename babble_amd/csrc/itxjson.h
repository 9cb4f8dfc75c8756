// itxjson.h — InternalTransactions built from their fields (bv_event_itx_batch,
// include/babbleverify.h), as __host__ __device__ templates over an output
// sink in the style of blkjson.h: the device streams each body into SHA-256
// (k_itx_body_hash, k_ev_body_hash_itx: EvjSha), the host writes it to memory
// (bv_itx_bodies, bv_event_itx_bodies, the in-batch DAG path) and the emulator
// (tests/emu_itx) runs the device's sink on the CPU.
//
// InternalTransactionBody.Marshal (src/hashgraph/internal_transaction.go) is
// Go 1.13 encoding/json of the exported fields, then '\n' (json.Encoder):
//   {"Type":T,"Peer":{"NetAddr":S,"PubKeyHex":S,"Moniker":S}}\n
// and one element of EventBody.InternalTransactions is
//   {"Body":{"Type":T,"Peer":{...}},"Signature":S}
//   T  decimal of a uint8
//   S  a Go string through encodeState.string with escapeHTML = true
//      (gojson_string below)
#pragma once
#include "evjson.h"

// Length of the valid UTF-8 sequence that starts at s[i] (2..4), or 0 when
// utf8.DecodeRuneInString would return (RuneError, 1) there: a continuation or
// 0xC0 / 0xC1 / > 0xF4 lead byte, an overlong or surrogate or > U+10FFFF
// second byte, a bad continuation, or a sequence cut short by the end of the
// string.  s[i] >= 0x80.
DEV uint32_t gojson_rune_len(const uint8_t *s, uint64_t i, uint64_t n) {
  const uint8_t c0 = s[i];
  if (c0 < 0xC2 || c0 > 0xF4) return 0;
  uint32_t need;
  uint8_t lo = 0x80, hi = 0xBF;
  if (c0 < 0xE0) {
    need = 1;
  } else if (c0 < 0xF0) {
    need = 2;
    if (c0 == 0xE0) lo = 0xA0;
    if (c0 == 0xED) hi = 0x9F;
  } else {
    need = 3;
    if (c0 == 0xF0) lo = 0x90;
    if (c0 == 0xF4) hi = 0x8F;
  }
  if (n - i <= need) return 0;
  if (s[i + 1] < lo || s[i + 1] > hi) return 0;
  for (uint32_t k = 2; k <= need; k++)
    if (s[i + k] < 0x80 || s[i + k] > 0xBF) return 0;
  return need + 1;
}

DEV uint8_t gojson_hexc(uint32_t x) { return (uint8_t)(x < 10 ? '0' + x : 'a' + x - 10); }

// Go 1.13 encodeState.string(s, escapeHTML = true), quotes included: `"` and
// `\` escaped; \n \r \t; other bytes < 0x20 and < > & as \u00XX (lowercase
// hex); 0x7F verbatim; U+2028 / U+2029 as backslash-u escapes (u2028, u2029);
// one ufffd escape per byte that starts no valid UTF-8 sequence; every other
// rune verbatim.
template <class O>
DEV void gojson_string(O &o, const uint8_t *s, uint64_t n) {
  o.put('"');
  for (uint64_t i = 0; i < n;) {
    const uint8_t c = s[i];
    if (c < 0x80) {
      i++;
      if (c >= 0x20 && c != '"' && c != '\\' && c != '<' && c != '>' && c != '&') {
        o.put(c);
        continue;
      }
      o.put('\\');
      if (c == '"' || c == '\\') {
        o.put(c);
      } else if (c == '\n') {
        o.put('n');
      } else if (c == '\r') {
        o.put('r');
      } else if (c == '\t') {
        o.put('t');
      } else {
        evj_lit(o, "u00");
        o.put(gojson_hexc(c >> 4));
        o.put(gojson_hexc(c & 15));
      }
      continue;
    }
    const uint32_t len = gojson_rune_len(s, i, n);
    if (len == 0) {
      evj_lit(o, "\\ufffd");
      i++;
      continue;
    }
    if (len == 3 && c == 0xE2 && s[i + 1] == 0x80 && (s[i + 2] & 0xFE) == 0xA8) {
      evj_lit(o, "\\u202");
      o.put(gojson_hexc(s[i + 2] & 15));
    } else {
      for (uint32_t k = 0; k < len; k++) o.put(s[i + k]);
    }
    i += len;
  }
  o.put('"');
}

DEV uint64_t gojson_string_len(const uint8_t *s, uint64_t n) {
  uint64_t out = 2;
  for (uint64_t i = 0; i < n;) {
    const uint8_t c = s[i];
    if (c < 0x80) {
      i++;
      if (c >= 0x20 && c != '"' && c != '\\' && c != '<' && c != '>' && c != '&') out += 1;
      else if (c == '"' || c == '\\' || c == '\n' || c == '\r' || c == '\t') out += 2;
      else out += 6;
      continue;
    }
    const uint32_t len = gojson_rune_len(s, i, n);
    if (len == 0) {
      out += 6;
      i++;
      continue;
    }
    out += (len == 3 && c == 0xE2 && s[i + 1] == 0x80 && (s[i + 2] & 0xFE) == 0xA8) ? 6 : len;
    i += len;
  }
  return out;
}

#define ITX_L0 "{\"Type\":"
#define ITX_L1 ",\"Peer\":{\"NetAddr\":"
#define ITX_L2 ",\"PubKeyHex\":"
#define ITX_L3 ",\"Moniker\":"
#define ITX_L4 "}}"
#define ITX_E0 "{\"Body\":"
#define ITX_E1 ",\"Signature\":"

// string k of ITX i: 0 NetAddr, 1 PubKeyHex, 2 Moniker, 3 Signature
#define ITX_NETADDR 0
#define ITX_PUBKEYHEX 1
#define ITX_MONIKER 2
#define ITX_SIGNATURE 3
// Bases of a shard (bv_group_verify_events_itx / _fields), as EvjBases: the ITX
// arrays of `x` are the slices one event range of a larger batch needs, and
// the values in itx_start and itx_str_off are still the whole batch's.
//   itx  itx_start[a]: itx_type and itx_str_off start at that ITX (an ITX
//        index passed to the functions below is already the slice's, i - itx)
//   str  itx_str_off[4 * itx]: itx_str starts at that byte
// ItxNoBases (all zero, compile-time) is the whole batch: the subtractions
// fold away and the emitters compile as they did without them.
struct ItxBases {
  uint64_t itx, str;
};
struct ItxNoBases {
  static constexpr uint64_t itx = 0, str = 0;
};

template <class B = ItxNoBases>
DEV const uint8_t *itx_str_ptr(const bv_event_itx_batch &x, uint64_t i, int k, const B &bs = B{}) {
  return x.itx_str + (x.itx_str_off[4 * i + k] - bs.str);
}
DEV uint64_t itx_str_len(const bv_event_itx_batch &x, uint64_t i, int k) {
  return x.itx_str_off[4 * i + k + 1] - x.itx_str_off[4 * i + k];
}

// {"Type":T,"Peer":{...}} of ITX i: the body without Marshal's newline
template <class O, class B = ItxNoBases>
DEV void itx_body_json(const bv_event_itx_batch &x, uint64_t i, O &o, const B &bs = B{}) {
  evj_lit(o, ITX_L0);
  evj_dec(o, (int64_t)x.itx_type[i]);
  evj_lit(o, ITX_L1);
  gojson_string(o, itx_str_ptr(x, i, ITX_NETADDR, bs), itx_str_len(x, i, ITX_NETADDR));
  evj_lit(o, ITX_L2);
  gojson_string(o, itx_str_ptr(x, i, ITX_PUBKEYHEX, bs), itx_str_len(x, i, ITX_PUBKEYHEX));
  evj_lit(o, ITX_L3);
  gojson_string(o, itx_str_ptr(x, i, ITX_MONIKER, bs), itx_str_len(x, i, ITX_MONIKER));
  evj_lit(o, ITX_L4);
}

DEV uint64_t itx_body_json_len(const bv_event_itx_batch &x, uint64_t i) {
  uint64_t n = EVJ_LEN(ITX_L0) + evj_dec_len((int64_t)x.itx_type[i]) + EVJ_LEN(ITX_L1) + EVJ_LEN(ITX_L2) +
               EVJ_LEN(ITX_L3) + EVJ_LEN(ITX_L4);
  for (int k = ITX_NETADDR; k <= ITX_MONIKER; k++) n += gojson_string_len(itx_str_ptr(x, i, k), itx_str_len(x, i, k));
  return n;
}

// InternalTransactionBody.Marshal() of ITX i (what its Signature is over)
template <class O, class B = ItxNoBases>
DEV void itx_body_emit(const bv_event_itx_batch &x, uint64_t i, O &o, const B &bs = B{}) {
  itx_body_json(x, i, o, bs);
  o.put('\n');
}
DEV uint64_t itx_body_len(const bv_event_itx_batch &x, uint64_t i) { return itx_body_json_len(x, i) + 1; }

// One element of EventBody.InternalTransactions
template <class O, class B = ItxNoBases>
DEV void itx_elem_emit(const bv_event_itx_batch &x, uint64_t i, O &o, const B &bs = B{}) {
  evj_lit(o, ITX_E0);
  itx_body_json(x, i, o, bs);
  evj_lit(o, ITX_E1);
  gojson_string(o, itx_str_ptr(x, i, ITX_SIGNATURE, bs), itx_str_len(x, i, ITX_SIGNATURE));
  o.put('}');
}
DEV uint64_t itx_elem_len(const bv_event_itx_batch &x, uint64_t i) {
  return EVJ_LEN(ITX_E0) + itx_body_json_len(x, i) + EVJ_LEN(ITX_E1) +
         gojson_string_len(itx_str_ptr(x, i, ITX_SIGNATURE), itx_str_len(x, i, ITX_SIGNATURE)) + 1;
}

DEV bool itx_list_is_nil(const bv_event_itx_batch &x, uint64_t e) { return x.itx_list_nil && x.itx_list_nil[e]; }

// The evj_len / evj_emit variants: event e's body with the InternalTransactions
// member built from the fields (x.events.itx_off is NULL).  ppos: as evj_len,
// the in-batch parents' hex positions, after the ITX text.
// (the member's value on its own: bsigjson.h builds the rest differently)
DEV uint64_t itx_list_len(const bv_event_itx_batch &x, uint64_t e) {
  if (itx_list_is_nil(x, e)) return 4;
  const uint64_t i0 = x.itx_start[e], i1 = x.itx_start[e + 1];
  uint64_t n = 2 + (i1 > i0 ? i1 - i0 - 1 : 0);
  for (uint64_t i = i0; i < i1; i++) n += itx_elem_len(x, i);
  return n;
}

template <class O, class B = ItxNoBases>
DEV void itx_list_emit(const bv_event_itx_batch &x, uint64_t e, O &o, const B &bs = B{}) {
  if (itx_list_is_nil(x, e)) {
    evj_lit(o, "null");
  } else {
    const uint64_t i0 = x.itx_start[e] - bs.itx, i1 = x.itx_start[e + 1] - bs.itx;
    o.put('[');
    for (uint64_t i = i0; i < i1; i++) {
      if (i > i0) o.put(',');
      itx_elem_emit(x, i, o, bs);
    }
    o.put(']');
  }
}

DEV uint64_t evj_len(const bv_event_itx_batch &x, uint64_t e, uint32_t ppos[2]) {
  return evj_len_rest(x.events, e, evj_len_txs(x.events, e) + itx_list_len(x, e), ppos);
}

// (bs, ib: a shard's bases; `e` is then the whole batch's index, as evj_emit's)
template <class O, class B = EvjNoBases, class IB = ItxNoBases>
DEV void evj_emit(const bv_event_itx_batch &x, uint64_t e, O &o, const B &bs = B{}, const IB &ib = IB{}) {
  e -= bs.ev;
  evj_emit_txs(x.events, e, o, bs);
  itx_list_emit(x, e, o, ib);
  evj_emit_rest(x.events, e, o, bs);
}

DEV void evj_write(const bv_event_itx_batch &x, uint64_t e, uint8_t *o) {
  EvjMem m{o};
  evj_emit(x, e, m);
}

// Event.Verify's fold for event e (event.go:219-247) over the item statuses:
// item e is the event signature, item n_ev + i ITX i; an ITX with force_panic
// set is BV_REF_PANIC whatever its item says.  The first ITX of the event that
// is not ACCEPT decides it, else the event signature does.  Writes the event's
// status and decided_by and its ITXs' own statuses; returns status ==
// BV_ACCEPT.  itx_base: itx_start holds a larger batch's values while every
// other array starts at the shard's first event / ITX (0: the whole batch).
DEV bool ev_fold(uint64_t n_ev, uint64_t e, const uint64_t *__restrict__ itx_start, uint64_t itx_base,
                 const uint8_t *__restrict__ item_status, const uint8_t *__restrict__ force_panic,
                 uint8_t *__restrict__ ev_status, uint32_t *__restrict__ decided_by,
                 uint8_t *__restrict__ itx_status) {
  uint8_t st = item_status[e];
  uint32_t by = BV_EV_SELF;
  const uint64_t i0 = itx_start[e] - itx_base, i1 = itx_start[e + 1] - itx_base;
  for (uint64_t i = i0; i < i1; i++) {
    const uint8_t c = force_panic[i] ? (uint8_t)BV_REF_PANIC : item_status[n_ev + i];
    itx_status[i] = c;
    if (by == BV_EV_SELF && c != BV_ACCEPT) {
      by = (uint32_t)(i - i0);
      st = c == BV_REJECT ? (uint8_t)BV_EV_ITX_INVALID : c;
    }
  }
  ev_status[e] = st;
  decided_by[e] = by;
  return st == BV_ACCEPT;
}
