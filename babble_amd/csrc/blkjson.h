// blkjson.h — canonical BlockBody JSON built from a block's fields
// (bv_block_batch, include/babbleverify.h), as __host__ __device__ templates
// over an output sink in the style of evjson.h: the device streams each body
// into SHA-256 (k_blk_body_hash, EvjSha), the host writes it to memory
// (bv_block_bodies, the small-batch path, long bodies) and the emulator
// (tests/emu_blocks) runs the device's sink on the CPU.
//
// BlockBody.Marshal (src/hashgraph/block.go:16-36) is Go 1.13 encoding/json
// of the exported fields in declaration order, then '\n' (json.Encoder):
//   {"Index":d,"RoundReceived":d,"Timestamp":d,"StateHash":H,"FrameHash":H,
//    "PeersHash":H,"Transactions":T,"InternalTransactions":I,
//    "InternalTransactionReceipts":R}\n
//   d  decimal int64
//   H  null (nil []byte), else "<b64>" (padded StdEncoding; empty -> "")
//   T  nil -> null, else [x,...] with x = null (nil []byte) or "<b64>"
//   I, R  verbatim JSON from the host (encoding/json of the slices); an
//      empty fragment means nil -> null ("[]" is a fragment)
#pragma once
#include <string.h>

#include "evjson.h"

#define BLK_L0 "{\"Index\":"
#define BLK_L1 ",\"RoundReceived\":"
#define BLK_L2 ",\"Timestamp\":"
#define BLK_L3 ",\"StateHash\":"
#define BLK_L4 ",\"FrameHash\":"
#define BLK_L5 ",\"PeersHash\":"
#define BLK_L6 ",\"Transactions\":"
#define BLK_L7 ",\"InternalTransactions\":"
#define BLK_L8 ",\"InternalTransactionReceipts\":"

// Bases of a shard (bv_group_verify_blocks): the arrays of `k` are the slices
// one block range [blk, ...) of a larger batch needs, and the values in them
// (hash_off, tx_start, tx_off, itx_off, rcpt_off) are still the whole
// batch's.  Wherever such a value indexes another array, its base — the value
// at which that slice starts — is subtracted:
//   blk   the per-block arrays start at block blk (hash_off and hash_nil at
//         3 blk; b is the batch's index)
//   hash  hash_off[3 blk]: hash_bytes starts at that byte
//   tx    tx_start[blk]: tx_off and tx_nil start at that transaction
//   txb   tx_off[tx_start[blk]]: tx_bytes starts at that byte
//   itx   itx_off[blk], rcpt  rcpt_off[blk]: the fragment bytes start there
// BlkNoBases (all zero, compile-time) is the whole batch: the subtractions
// fold away and blk_len / blk_emit compile as they did without them.
struct BlkBases {
  uint64_t blk, hash, tx, txb, itx, rcpt;
};
struct BlkNoBases {
  static constexpr uint64_t blk = 0, hash = 0, tx = 0, txb = 0, itx = 0, rcpt = 0;
};

// Body length of block b.
template <class B = BlkNoBases>
DEV uint64_t blk_len(const bv_block_batch &k, uint64_t b, const B &bs = B{}) {
  b -= bs.blk;
  uint64_t n = EVJ_LEN(BLK_L0) + evj_dec_len(k.index[b]) + EVJ_LEN(BLK_L1) + evj_dec_len(k.round_received[b]) +
               EVJ_LEN(BLK_L2) + evj_dec_len(k.timestamp[b]) + EVJ_LEN(BLK_L3) + EVJ_LEN(BLK_L4) + EVJ_LEN(BLK_L5);
  for (int h = 0; h < 3; h++) {
    const uint64_t i = 3 * b + h;
    n += (k.hash_nil && k.hash_nil[i]) ? 4 : 2 + evj_b64_len(k.hash_off[i + 1] - k.hash_off[i]);
  }
  n += EVJ_LEN(BLK_L6);
  if (k.tx_list_nil && k.tx_list_nil[b]) {
    n += 4;
  } else {
    const uint64_t t0 = k.tx_start[b] - bs.tx, t1 = k.tx_start[b + 1] - bs.tx;
    n += 2 + (t1 > t0 ? t1 - t0 - 1 : 0);
    for (uint64_t t = t0; t < t1; t++)
      n += (k.tx_nil && k.tx_nil[t]) ? 4 : 2 + evj_b64_len(k.tx_off[t + 1] - k.tx_off[t]);
  }
  const uint64_t il = evj_frag_len(k.itx_off, b), rl = evj_frag_len(k.rcpt_off, b);
  n += EVJ_LEN(BLK_L7) + (il ? il : 4) + EVJ_LEN(BLK_L8) + (rl ? rl : 4) + 2;  // "}\n"
  return n;
}

// base64 and verbatim bytes into a sink: the generic forms (every sink, the
// device's among them) go byte by byte through put(); on the host the memory
// sink takes table look-ups and memcpy instead (bv_block_bodies, the small
// path and the long bodies; C5 bodies on one core: 0.14 GB/s through put(),
// 2.0 GB/s so).
template <class O>
DEV void blk_b64(O &o, const uint8_t *src, uint64_t n) {
  evj_b64(o, src, n);
}
template <class O>
DEV void blk_copy(O &o, const uint8_t *src, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) o.put(src[i]);
}
#if !defined(__HIP_DEVICE_COMPILE__)
inline void blk_b64(EvjMem &o, const uint8_t *src, uint64_t n) {
  static const char T[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  uint8_t *p = o.p;
  uint64_t i = 0;
  for (; i + 3 <= n; i += 3, p += 4) {
    const uint32_t v = ((uint32_t)src[i] << 16) | ((uint32_t)src[i + 1] << 8) | src[i + 2];
    p[0] = (uint8_t)T[v >> 18], p[1] = (uint8_t)T[(v >> 12) & 63], p[2] = (uint8_t)T[(v >> 6) & 63];
    p[3] = (uint8_t)T[v & 63];
  }
  o.p = p;
  evj_b64(o, src + i, n - i);  // the last 1 or 2 bytes and their padding
}
inline void blk_copy(EvjMem &o, const uint8_t *src, uint64_t n) {
  if (n) memcpy(o.p, src, n);
  o.p += n;
}
#endif

// Block b's body into sink `o` (blk_len bytes).
template <class O, class B = BlkNoBases>
DEV void blk_emit(const bv_block_batch &k, uint64_t b, O &o, const B &bs = B{}) {
  b -= bs.blk;
  evj_lit(o, BLK_L0);
  evj_dec(o, k.index[b]);
  evj_lit(o, BLK_L1);
  evj_dec(o, k.round_received[b]);
  evj_lit(o, BLK_L2);
  evj_dec(o, k.timestamp[b]);
  for (int h = 0; h < 3; h++) {
    evj_lit(o, h == 0 ? BLK_L3 : h == 1 ? BLK_L4 : BLK_L5);
    const uint64_t i = 3 * b + h;
    if (k.hash_nil && k.hash_nil[i]) {
      evj_lit(o, "null");
    } else {
      o.put('"');
      blk_b64(o, k.hash_bytes + (k.hash_off[i] - bs.hash), k.hash_off[i + 1] - k.hash_off[i]);
      o.put('"');
    }
  }
  evj_lit(o, BLK_L6);
  if (k.tx_list_nil && k.tx_list_nil[b]) {
    evj_lit(o, "null");
  } else {
    const uint64_t t0 = k.tx_start[b] - bs.tx, t1 = k.tx_start[b + 1] - bs.tx;
    o.put('[');
    for (uint64_t t = t0; t < t1; t++) {
      if (t > t0) o.put(',');
      if (k.tx_nil && k.tx_nil[t]) {
        evj_lit(o, "null");
      } else {
        o.put('"');
        blk_b64(o, k.tx_bytes + (k.tx_off[t] - bs.txb), k.tx_off[t + 1] - k.tx_off[t]);
        o.put('"');
      }
    }
    o.put(']');
  }
  evj_lit(o, BLK_L7);
  const uint64_t il = evj_frag_len(k.itx_off, b);
  if (il) {
    blk_copy(o, k.itx_json + (k.itx_off[b] - bs.itx), il);
  } else {
    evj_lit(o, "null");
  }
  evj_lit(o, BLK_L8);
  const uint64_t rl = evj_frag_len(k.rcpt_off, b);
  if (rl) {
    blk_copy(o, k.rcpt_json + (k.rcpt_off[b] - bs.rcpt), rl);
  } else {
    evj_lit(o, "null");
  }
  o.put('}');
  o.put('\n');
}

// Block b's body written at `o` (blk_len bytes).
DEV void blk_write(const bv_block_batch &k, uint64_t b, uint8_t *o) {
  EvjMem m{o};
  blk_emit(k, b, m);
}
