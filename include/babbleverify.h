/*
 * babbleverify.h — C ABI of libbabbleverify.so, the MI355X batch verifier for
 * Babble's event-ingestion hot path (SHA-256 of canonical bodies + ECDSA over
 * secp256k1).  Plain C types only: this is what a Go cgo shim (see
 * INTEGRATION.md) or any other FFI binds.
 *
 * Reference interfaces each entry point replaces (paths under the reference
 * tree, sikoba/babble v0.8.4):
 *   bv_verify_batch   N x { crypto.SHA256(body)              src/crypto/hash.go:8
 *                           keys.ToPublicKey(pub)             src/crypto/keys/public_key.go:14
 *                           keys.Verify(pub, hash, r, s) }    src/crypto/keys/signature.go:20
 *                     as composed by Event.Verify             src/hashgraph/event.go:219-247
 *                     InternalTransaction.Verify              src/hashgraph/internal_transaction.go:139-154
 *                     Block.Verify                            src/hashgraph/block.go:343-357
 *   bv_verify_batch_text  the same items from their Signature text:
 *                     keys.DecodeSignature applied by the library
 *                                                             src/crypto/keys/signature.go:31-39
 *   bv_verify_blocks  the same for block signatures, from the
 *                     BlockBody's fields: BlockBody.Marshal   src/hashgraph/block.go:16-36
 *                     and CheckBlock's tally                  src/hashgraph/hashgraph.go:1599-1630
 *   bv_sha256_batch   N x crypto.SHA256                       src/crypto/hash.go:8-13
 *   bv_decode_signature  keys.DecodeSignature + the sign/range
 *                     pre-checks of ecdsa.Verify              src/crypto/keys/signature.go:31-39
 *   bv_hex_decode     common.DecodeFromString                 src/common/hex.go:15-17
 *
 * Threading: every entry point is re-entrant.  A bv_ctx serialises its own
 * calls with an internal mutex (processJoinRequest, node_rpc.go:250-260, calls
 * the verifier outside Node.coreLock); use one ctx per thread for concurrency.
 * Ownership: all pointers are caller-owned and only read/written during the
 * call; nothing is retained.  There is no CPU fallback: if no gfx950 device is
 * usable the calls fail with BV_E_NODEVICE.
 */
#ifndef BABBLEVERIFY_H
#define BABBLEVERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BV_ABI_VERSION 6

/* Return codes (per-item outcomes are never errors; they go to status[]). */
#define BV_OK 0
#define BV_E_ARGS (-1)
#define BV_E_NODEVICE (-2)
#define BV_E_OOM (-3)
#define BV_E_LAUNCH (-4)
#define BV_E_COMM (-5)

/* Item status (SURVEY §8a-9 decision table). */
#define BV_REJECT 0     /* keys.Verify returned false                          */
#define BV_ACCEPT 1     /* keys.Verify returned true                           */
#define BV_REJECT_ERR 2 /* DecodeSignature returned an error (parts != 2)      */
#define BV_REF_PANIC 3  /* the Go reference would panic on this input          */

/* Pre-class byte per item, decided on the host from the signature text.
 * bits 0-1: class of r, bits 2-3: class of s, bit 7: parts != 2.
 * pre == 0 means "r and s parsed and both in [1, N-1]": run the math.       */
#define BV_SC_OK 0     /* 0 < v < N                                          */
#define BV_SC_NIL 1    /* big.Int SetString failed -> nil (Go would panic)   */
#define BV_SC_NONPOS 2 /* v <= 0                                             */
#define BV_SC_GE_N 3   /* v >= N (possibly wider than 256 bits)              */
#define BV_PRE_PARTS_BAD 0x80
#define BV_PRE(rc, sc) ((uint8_t)((rc) | ((sc) << 2)))

/* Flags for bv_create (any other bit is BV_E_ARGS). */
#define BV_F_DEFAULT 0u
#define BV_F_KEY_CACHE 1u /* keep per-key tables in HBM across calls, keyed by
                             the raw pubkey bytes (validator sets are stable,
                             peers/peer_set.go): 22-bit signed-window GLV
                             tables, 805 MB per valid key.  A key gets a table
                             when it is registered (bv_kc_register: the
                             PeerSet) or once it has been seen in 2 batches
                             (env BV_KC_ADMIT); tables are LRU-evicted past
                             the cache budget (env BV_KEY_CACHE_GB, default
                             96), registered keys only for other registered
                             keys.  Malformed keys are never given a table.
                             A batch with one valid key that has no table
                             takes the per-batch table path.  With env
                             BV_KC_PARTIAL=1 (opt-in) a batch whose valid keys
                             without a table are at most 1 in 16 of its valid
                             keys, carrying at most 1 in 16 of its items,
                             keeps the cache instead (their items are
                             finished by the generic path after the cached
                             ones).  Off by default: tables are then rebuilt
                             for every batch.                                  */
#define BV_F_K8 2u        /* per-batch tables: never use the 12-bit tables
                             (2.75 MiB per key); 8-bit only (512 KiB per key) */
#define BV_F_KC_COMPACT 4u /* with BV_F_KEY_CACHE only (alone: BV_E_ARGS): the
                             context's cached tables use the compact KC18
                             geometry, for validator sets past the 119 keys
                             the 805 MB tables hold: 18-bit signed windows x 8
                             over each GLV half, 67,108,928 bytes (67.1 MB)
                             per valid key, so the default 96 GB budget holds
                             1430 tables; 16 additions + 8 multiplies per item
                             for u2 Q against 12 + 6.  A context has ONE
                             cached geometry, fixed here.  Admission,
                             registration, eviction and the budget work as
                             above, per 67.1 MB table; bv_timing.key_path
                             reports 18.  Small batches: by default the
                             one-launch small path does not read KC18 tables,
                             so batches of at most 256 items (env
                             BV_SMALL_MAX) run it as for keys without a table
                             (key_path 0), the 257-1024 item extension for
                             fully cached batches is off, and those batches
                             take the bulk pipeline, which uses the tables
                             (key_path 18).  After bv_kc_small_tables(ctx, 1)
                             the small path reads the KC18 tables as it reads
                             the 22-bit ones (26 table leaves instead of 22):
                             a key with a table skips the doubling chain,
                             fully cached batches of up to 1024 items (env
                             BV_SMALL_WARM_MAX) take the one launch, and
                             key_path reports 18 there too.                    */
#define BV_F_KNOWN (BV_F_KEY_CACHE | BV_F_K8 | BV_F_KC_COMPACT)

typedef struct bv_ctx bv_ctx;

/* One batch, struct-of-arrays.  Messages are hashed once each; items point
 * at a message and a key, so one BlockBody serves its 100 signatures. */
typedef struct {
  uint64_t n_msgs;
  const uint8_t *msg_bytes;  /* concatenated canonical JSON bodies            */
  const uint64_t *msg_off;   /* n_msgs + 1 offsets into msg_bytes            */
  uint32_t n_keys;
  const uint8_t *key_bytes;  /* concatenated raw pubkey bytes (any length)   */
  const uint64_t *key_off;   /* n_keys + 1 offsets into key_bytes            */
  uint64_t n_items;
  const uint32_t *item_msg;  /* message index per item                       */
  const uint32_t *item_key;  /* key index per item                           */
  const uint8_t *r_be;       /* 32 * n_items, big-endian r (valid if class OK) */
  const uint8_t *s_be;       /* 32 * n_items, big-endian s                    */
  const uint8_t *pre;        /* n_items pre-class bytes (NULL = all 0)       */
} bv_batch;

typedef struct {
  uint8_t *msg_hash;     /* 32 * n_msgs digests (NULL: not returned)          */
  uint8_t *status;       /* n_items BV_* statuses (NULL: not returned)        */
  uint64_t *accept_bits; /* ceil(n_items/64) words, bit i = item i ACCEPT,
                            LSB-first (NULL: not returned)                     */
} bv_result;

/* Timing of the last call, device-side (HIP events on the ctx stream). */
typedef struct {
  float ms_total;    /* first kernel start -> last kernel end                  */
  float ms_sha256;   /* k_sha256: message hashing                              */
  float ms_keyprep;  /* key decode + per-key table build (own stream, overlaps
                        hashing, s^-1 and the u1 G phase)                       */
  float ms_scalar;   /* k_sinv: batched s^-1 (own stream, from batch start)     */
  float ms_verify_g; /* k_verify_g: u1, u2 + GLV split, u1 G from the G table   */
  float ms_verify;   /* k_verify_q (+ u2 Q, decision, bits) or k_verify_generic */
  float ms_h2d;      /* host -> device staging (host-buffer entry point only):
                        call start -> last input byte in HBM                    */
  float ms_d2h;      /* device -> host results after the last kernel            */
  float ms_host;     /* wall clock of the whole call on the host (host entry
                        point: staging, PCIe, kernels, copy-out)                */
  float ms_host_prep; /* host: validation + staging copies, call start -> the
                         last input copy enqueued                               */
  float ms_host_out;  /* host: results copied out after the device finished    */
  uint32_t key_path; /* 0: per-lane generic path; 8 / 12: per-batch K8 / K12
                        key tables; 22: key-cache (KC) tables; 18: compact
                        key-cache (KC18) tables, BV_F_KC_COMPACT                */
  uint32_t kc_hits;   /* batch keys found in the key cache                      */
  uint32_t kc_builds; /* key tables built into the cache by this call           */
  uint32_t kc_keys;   /* keys held by the cache after the call                  */
} bv_timing;

int bv_abi_version(void);

/* Create a context on `device` (HIP ordinal; -1 = current device). */
int bv_create(bv_ctx **out, int device, uint32_t flags);
void bv_destroy(bv_ctx *ctx);
const char *bv_last_error(const bv_ctx *ctx);

/* Key cache (BV_F_KEY_CACHE contexts only): set the registered keys — the
 * PeerSet's PubKeyBytes (src/peers/peer_set.go; Babble calls this where the
 * peer set changes) — replacing the previous set, and build the tables of the
 * registered valid keys that have none, before returning.  Registered tables
 * are never evicted for unregistered keys.  BV_E_ARGS on a ctx without the
 * cache or more than 4096 keys.  Cap: the budget holds floor(BV_KEY_CACHE_GB
 * / 0.805) tables (119 at the default 96 GB), or with BV_F_KC_COMPACT
 * floor(BV_KEY_CACHE_GB / 0.0671) (1430); past it, the first registered
 * keys in the caller's order that fit get tables and the rest none (their
 * batches take the per-batch path), still BV_OK.  bv_get_timing's kc_builds
 * / kc_keys report what was built and what the cache holds. */
int bv_kc_register(bv_ctx *ctx, uint32_t n_keys, const uint8_t *key_bytes, const uint64_t *key_off);

/* Compact key cache (BV_F_KEY_CACHE | BV_F_KC_COMPACT contexts only): let the
 * one-launch small-batch path read the context's KC18 tables (on != 0) or
 * not (on == 0, the state after bv_create).  On: a small batch resolves its
 * keys against the cache on the host (LRU touch and kc_hits as for 22-bit
 * tables, never a build); items of a key with a table sum 10 + 2 x 8 table
 * leaves, items of other keys run the doubling chain in the same launch; a
 * batch of 257..1024 items (env BV_SMALL_WARM_MAX) takes the small path when
 * every well-formed key has a table; bv_timing.key_path is 18 when there were
 * hits.  Off: small batches run as for keys without a table.  Host state
 * only (no device work); takes effect from the next call.  BV_E_ARGS on a
 * NULL ctx and on a ctx without BV_F_KC_COMPACT (bv_last_error says so): a
 * 22-bit context's small path always reads its tables. */
int bv_kc_small_tables(bv_ctx *ctx, int on);

/* Synchronous batch verify from host buffers (the cgo entry point).  Any
 * input array or result buffer that lies in memory from bv_host_alloc is
 * moved by DMA from / to where it is; other (pageable) buffers go through
 * the ctx's pinned staging, one extra host copy each. */
int bv_verify_batch(bv_ctx *ctx, const bv_batch *batch, bv_result *result);

/* bv_verify_batch for callers that hold each item's signature as Go text:
 * Block.Verify over BlockSignature.Signature (src/hashgraph/block.go:343-357),
 * InternalTransaction.Verify (internal_transaction.go:139-154),
 * ProcessSigPool and processJoinRequest.  Instead of one bv_decode_signature
 * call per item the caller appends each "r|s" string's bytes to sig_text and
 * an offset to sig_off; the library decodes every text as
 * bv_decode_signature does (keys.DecodeSignature + the range checks,
 * src/crypto/keys/signature.go:31-39).  A batch that takes the bulk pipeline
 * ships the text instead of r / s / pre and decodes it on the device
 * (k_sig_decode, ahead of s^-1); a small batch (the one-launch path) is
 * decoded by the host parser inside the call.  Results are bit-identical to
 * bv_verify_batch over the host-decoded arrays either way. */
typedef struct {
  bv_batch items;          /* r_be, s_be, pre are ignored and may be NULL  */
  const uint64_t *sig_off; /* n_items + 1 byte offsets into sig_text       */
  const uint8_t *sig_text; /* each item's Signature text ("r|s", base 36)  */
} bv_text_batch;

/* The result contract, the threading and the pinned-memory rule are
 * bv_verify_batch's; sig_off and sig_text in bv_host_alloc memory are DMA'd
 * in place too.  BV_E_ARGS (with a bv_last_error text) beyond
 * bv_verify_batch's cases: sig_off NULL with n_items > 0, sig_off[0] != 0,
 * sig_off not monotone, sig_text NULL with sig_off[n_items] > 0.  n_items == 0
 * is BV_OK (the messages are still hashed). */
int bv_verify_batch_text(bv_ctx *ctx, const bv_text_batch *tb, bv_result *result);

/* Page-locked host memory (hipHostMalloc, portable to every device) for
 * callers that build their batches in place (the cgo shim allocates its
 * bv_batch arrays here instead of C.CBytes copies).  bv_host_free ignores
 * pointers it did not allocate.  No device context is needed. */
int bv_host_alloc(size_t bytes, void **out);
void bv_host_free(void *p);

/* A pinned arena: BV_ARENA_SLOTS growable blocks of bv_host_alloc memory
 * that persist until bv_arena_destroy.  A caller that keeps its arena across
 * calls (the cgo shim's pooled batch builders)
 * page-locks and frees nothing per call: hipHostMalloc / hipHostFree cost
 * tens of microseconds each and hipHostFree synchronises the device.  Arena
 * memory is bv_host_alloc memory, so batches built in it are DMA'd in place.
 * An arena is not thread-safe: one per concurrent builder.  No device
 * context is needed. */
#define BV_ARENA_SLOTS 32
typedef struct bv_arena bv_arena;
int bv_arena_create(bv_arena **out);
void bv_arena_destroy(bv_arena *arena);
/* Block `slot` (< BV_ARENA_SLOTS) with capacity >= `bytes`.  When it must
 * grow, the new block holds max(bytes, 2 x the old capacity) bytes and its
 * first `keep` bytes (<= the old capacity) are copied from the old one, which
 * is freed.  *out = the block's base, *cap (may be NULL) = its capacity.
 * BV_E_ARGS, BV_E_OOM (the old block is then kept). */
int bv_arena_reserve(bv_arena *arena, uint32_t slot, size_t bytes, size_t keep, void **out, size_t *cap);

/* Same, with every bv_batch / bv_result pointer in device memory of the ctx's
 * device (inputs already resident in HBM).  `stream` is a hipStream_t (NULL =
 * the ctx stream); the call returns after the work is enqueued when
 * `async` != 0, else after it completes.  msg_bytes and key_bytes must stay
 * readable for 64 bytes past their last byte (the kernels read them with
 * aligned vector loads; the host entry points pad their staging copies). */
int bv_verify_batch_device(bv_ctx *ctx, const bv_batch *dbatch, bv_result *dresult,
                           void *stream, int async);
/* Streams: a process holds ONE set per device, shared by all its contexts
 * (HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware
 * queues, 4 by default; streams sharing a queue run serially): one lane per
 * work slot, the s^-1 stream and a high-priority key-table stream, plus a
 * copy stream created by the first host-entry call.  A NULL `stream` above
 * runs the call on its slot's lane, so consecutive async calls overlap
 * without the caller creating streams.  bv_last_stream returns the stream
 * the ctx's last call ran on (a hipStream_t), to order the caller's own
 * work after an async NULL-stream call. */
void *bv_last_stream(const bv_ctx *ctx);
/* The ctx holds two sets of work buffers.  Consecutive bv_verify_batch_device
 * calls alternate them, and each waits (on the device) only for the last call
 * that used the same set — and for the call before it when their result
 * buffers overlap: two async calls on different streams writing different
 * results overlap, one call's key tables building beside the other's verify
 * (the caller orders a call whose inputs an earlier in-flight call's results
 * write, as for any two streams).  Every other entry
 * point first waits for all earlier calls.  bv_sync waits for every call's
 * work and updates bv_get_timing (the last call's). */
int bv_sync(bv_ctx *ctx);

/* Events from their wire fields.  Instead of the
 * serialized bodies, the caller passes what a WireEvent carries
 * (src/hashgraph/event.go:413-449) with the parents resolved as in
 * Hashgraph.ReadWireInfo (hashgraph.go:1540-1595); the device builds every
 * canonical EventBody JSON (event.go:38-45, Go 1.13 encoding/json, bit-exact),
 * hashes it and verifies the creator's signature over it.  A parent may be an
 * EARLIER event of the same batch (the in-batch DAG dependency of core.sync,
 * core.go:214-245): its "0X"+hex is spliced into the child's body once the
 * parent's digest is known.  Such a batch (a SyncResponse) is built and
 * hashed in topological order on the host while the device decodes the keys,
 * builds the key tables and inverts s; then only the digests cross PCIe and
 * the device verifies.  Batches without in-batch parents are built and hashed
 * on the device; ~2-3x fewer bytes cross PCIe than the serialized bodies
 * (64-B tx: ~250 B per event instead of ~530).
 * Per-event result: msg_hash (the body digest = Event.Hash) and status of the
 * event signature (keys.Verify as composed by Event.Verify, event.go:232-247).
 * InternalTransactions are serialized from the verbatim fragment but their
 * own signatures are NOT verified here (use bv_verify_batch items, as the Go
 * shim does for Event.Verify's ITX loop), or pass the ITXs' fields to
 * bv_verify_events_itx below, which verifies them in the same call). */
#define BV_PARENT_NONE 0  /* "" (wire index < 0)                              */
#define BV_PARENT_HASH 1  /* known hash: parent_ref indexes parent_hashes     */
#define BV_PARENT_EVENT 2 /* an earlier event of this batch: parent_ref = its
                             index (< the child's)                            */
typedef struct {
  uint64_t n_events;
  uint32_t n_keys;
  const uint8_t *key_bytes;      /* creator keys, raw bytes (as bv_batch)      */
  const uint64_t *key_off;       /* n_keys + 1                                 */
  const uint32_t *creator;       /* key index per event (EventBody.Creator)    */
  const int64_t *index;          /* EventBody.Index                            */
  const int64_t *timestamp;      /* EventBody.Timestamp                        */
  const uint8_t *parent_kind;    /* 2 per event: self-parent, other-parent     */
  const uint64_t *parent_ref;    /* 2 per event (see BV_PARENT_*)              */
  uint64_t n_parent_hashes;
  const uint8_t *parent_hashes;  /* 32 bytes each                              */
  const uint64_t *tx_start;      /* n_events + 1: event e has transactions
                                    [tx_start[e], tx_start[e+1])               */
  const uint64_t *tx_off;        /* n_tx + 1 byte offsets into tx_bytes        */
  const uint8_t *tx_bytes;
  const uint8_t *tx_list_nil;    /* per event, 1: Transactions is nil (NULL: none) */
  const uint8_t *tx_nil;         /* per tx, 1: that []byte is nil (NULL: none)  */
  const uint64_t *itx_off;       /* n_events + 1 into itx_json: encoding/json of
                                    InternalTransactions; empty = nil (NULL: all nil) */
  const uint8_t *itx_json;
  const uint64_t *bsig_off;      /* same for BlockSignatures (creator = Validator) */
  const uint8_t *bsig_json;
  const uint8_t *r_be;           /* the event signature, as in bv_batch        */
  const uint8_t *s_be;
  const uint8_t *pre;
  /* OR the Event.Signature text of every event (sig_off: n_events + 1 byte
   * offsets into sig_text).  When sig_text is non-NULL, r_be / s_be / pre are
   * ignored (may be NULL): the device decodes each signature as
   * bv_decode_signature does (keys.DecodeSignature + the range checks) beside
   * the key decode, so a caller holding Go strings copies bytes and makes no
   * call per event. */
  const uint64_t *sig_off;
  const uint8_t *sig_text;
} bv_event_batch;

/* Host buffers in, results out (msg_hash: 32 * n_events; status, accept_bits
 * per event).  BV_E_ARGS for a bad reference (an EVENT parent not earlier in
 * the batch, an out-of-range key / hash / offset).  As for bv_verify_batch,
 * arrays and result buffers in bv_host_alloc memory are DMA'd in place. */
int bv_verify_events(bv_ctx *ctx, const bv_event_batch *events, bv_result *result);

/* The whole of Event.Verify (event.go:219-247) in one call: the events as
 * above, and their InternalTransactions from FIELDS instead of a JSON
 * fragment.  The library builds each InternalTransactionBody.Marshal() and
 * each element of EventBody.InternalTransactions on the device (Go 1.13
 * encoding/json string escaping included), hashes them, verifies every ITX
 * signature (InternalTransaction.Verify, internal_transaction.go:139-154) and
 * the event signature, and folds them in Event.Verify's order: the first ITX
 * of an event that is not ACCEPT decides it (REJECT_ERR -> BV_REJECT_ERR,
 * REF_PANIC -> BV_REF_PANIC, REJECT -> BV_EV_ITX_INVALID), else the event
 * signature's class does.  An ITX whose PubKeyHex is shorter than 2 bytes is
 * BV_REF_PANIC whatever its Signature is (Go panics in PubKeyBytes before
 * DecodeSignature runs).
 * result: per event, as bv_verify_events; msg_hash holds the event body
 * digests (written for every event, also one whose ITX fails), status the
 * fold, accept_bits bit e = status[e] == BV_ACCEPT.
 * BV_E_ARGS (with a bv_last_error text): everything bv_verify_events rejects;
 * events.itx_off or events.itx_json non-NULL; events.sig_text NULL; itx_start
 * NULL, not starting at 0 or not monotone; itx_str_off NULL while n_itx > 0,
 * not starting at 0 or not monotone; itx_str NULL while bytes are named;
 * itx_type NULL while n_itx > 0; n_events + n_itx > 2^32.  n_itx == 0 is
 * valid and returns exactly what bv_verify_events returns for the same events
 * with nil or "[]" fragments.
 * Over several devices: bv_group_verify_events_itx below. */
#define BV_EV_ITX_INVALID 4 /* (false, "invalid signature on internal transaction") */
#define BV_EV_SELF 0xFFFFFFFFu
typedef struct {
  bv_event_batch events;       /* itx_off / itx_json must be NULL; sig_text / sig_off required */
  const uint64_t *itx_start;   /* n_events + 1: event e owns ITXs [itx_start[e], itx_start[e+1]) */
  const uint8_t *itx_list_nil; /* per event, 1: the slice is nil -> null (NULL: none; an empty
                                  non-nil list is []), exactly as tx_list_nil */
  const uint8_t *itx_type;     /* per ITX: Body.Type */
  const uint64_t *itx_str_off; /* 4 * n_itx + 1 offsets into itx_str, per ITX in the order
                                  NetAddr, PubKeyHex, Moniker, Signature (raw Go string bytes) */
  const uint8_t *itx_str;
} bv_event_itx_batch;

typedef struct {        /* every pointer may be NULL */
  uint8_t *itx_hash;    /* 32 * n_itx: InternalTransactionBody.Hash */
  uint8_t *itx_status;  /* n_itx: the ITX's own InternalTransaction.Verify class, 0..3 */
  uint32_t *decided_by; /* n_events: BV_EV_SELF, or the event-local index of the ITX whose
                           failure is the event's outcome */
} bv_event_itx_out;

int bv_verify_events_itx(bv_ctx *ctx, const bv_event_itx_batch *batch, bv_result *result, bv_event_itx_out *out);
/* The serialiser's public form (host only, no device; as bv_block_body_lens /
 * bv_block_bodies): off[i + 1] - off[i] = the length of body i, off[0] = 0;
 * then the bodies at out + off[i] (each at least as long as the length).
 * bv_itx_*: InternalTransactionBody.Marshal() of every ITX; bv_event_itx_*:
 * EventBody.Marshal() of every event, an in-batch parent's hash as 64 '0'.
 * Only the fields the serialiser reads are checked.  BV_E_ARGS on a NULL
 * pointer or malformed offsets. */
int bv_itx_body_lens(const bv_event_itx_batch *batch, uint64_t *off /* n_itx + 1 */);
int bv_itx_bodies(const bv_event_itx_batch *batch, const uint64_t *off, uint8_t *out);
int bv_event_itx_body_lens(const bv_event_itx_batch *batch, uint64_t *off /* n_events + 1 */);
int bv_event_itx_bodies(const bv_event_itx_batch *batch, const uint64_t *off, uint8_t *out);

/* A whole Event from FIELDS: bv_verify_events_itx with the seventh member of
 * EventBody, BlockSignatures, built by the library too, so that the caller
 * serialises no JSON at all.  Every validator ships its signature of each
 * committed block in its next self-event (hashgraph.go:744, event.go:432-446),
 * so most events of a SyncResponse carry one or more.  One list element is
 *   {"Validator":V,"Index":D,"Signature":S}          (block.go:59-66)
 * V padded StdEncoding base64 in quotes (or null), D the decimal of a Go int,
 * S a Go string through encoding/json (Go 1.13, escapeHTML); the list is null,
 * [] or [e,e,...] exactly as the ITX list.
 * The block signatures are serialised and hashed ONLY: Event.Verify does not
 * verify them (ProcessSigPool does, later, against blocks that may not exist
 * yet; bv_verify_blocks / bv_verify_batch_text are the calls for that).
 * result / out: exactly bv_verify_events_itx's.
 * ev.itx_start == NULL: the batch has no ITX fields; every event's
 * InternalTransactions is nil (null), except where ev.itx_list_nil is given
 * and itx_list_nil[e] == 0, which is [].  No ITX array is read then.
 * BV_E_ARGS (with a bv_last_error text): everything bv_verify_events_itx
 * rejects except the NULL itx_start above; ev.events.bsig_off or bsig_json
 * non-NULL; bsig_start NULL while n_events > 0, not starting at 0 or not
 * monotone; bsig_index or bsig_sig_off NULL while n_bsig > 0; bsig_sig_off not
 * starting at 0 or not monotone; bsig_sig NULL while bytes are named; a kind
 * above 2; a kind BV_BSIG_VAL_BYTES with bsig_val_off NULL or not monotone
 * (over all n_bsig + 1 offsets, the entries of other kinds included), or
 * with bytes named and bsig_val_bytes NULL; n_bsig > 2^32.  n_bsig == 0 is
 * valid and returns exactly what bv_verify_events_itx (for a NULL itx_start:
 * bv_verify_events) returns for the same events with nil or "[]" fragments.
 * Over several devices: bv_group_verify_events_fields below. */
#define BV_BSIG_VAL_CREATOR 0 /* Validator = the event's creator key bytes (WireEvent.BlockSignatures) */
#define BV_BSIG_VAL_BYTES   1 /* Validator = bsig_val_bytes[bsig_val_off[j] .. bsig_val_off[j+1]) (any length, 0 -> "") */
#define BV_BSIG_VAL_NIL     2 /* Validator is a nil []byte -> null */
typedef struct {
  bv_event_itx_batch ev;        /* ev.events.bsig_off / bsig_json (and itx_off / itx_json) must be NULL */
  const uint64_t *bsig_start;   /* n_events + 1: event e owns block signatures [bsig_start[e], bsig_start[e+1]) */
  const uint8_t *bsig_list_nil; /* per event, 1: the slice is nil -> null (NULL: none; empty non-nil -> []) */
  const int64_t *bsig_index;    /* per signature: BlockSignature.Index (Go int) */
  const uint64_t *bsig_sig_off; /* n_bsig + 1 offsets into bsig_sig */
  const uint8_t *bsig_sig;      /* BlockSignature.Signature, raw Go string bytes */
  const uint8_t *bsig_val_kind; /* per signature (NULL: all BV_BSIG_VAL_CREATOR) */
  const uint64_t *bsig_val_off; /* n_bsig + 1 offsets into bsig_val_bytes.  Not read when no entry is
                                   BV_BSIG_VAL_BYTES (may be NULL).  Once any entry is, the WHOLE array must be
                                   valid and monotone (a non-BYTES entry owns an empty range) and
                                   bsig_val_bytes[0 .. bsig_val_off[n_bsig]) is read */
  const uint8_t *bsig_val_bytes;
} bv_event_fields_batch;

int bv_verify_events_fields(bv_ctx *ctx, const bv_event_fields_batch *batch, bv_result *result,
                            bv_event_itx_out *out /* may be NULL */);
/* The serialiser's public form, as bv_event_itx_body_lens / bv_event_itx_bodies:
 * EventBody.Marshal() of every event (host only, no device). */
int bv_event_fields_body_lens(const bv_event_fields_batch *batch, uint64_t *off /* n_events + 1 */);
int bv_event_fields_bodies(const bv_event_fields_batch *batch, const uint64_t *off, uint8_t *out);

/* Multi-GPU: one verifier over several devices of this process (one bv_ctx
 * per device, the caller's device ordinals).  bv_group_verify_batch shards
 * the items into contiguous ranges that never split the items of one
 * message (a BlockBody's signatures stay on one device), balanced by item
 * count (bv_plan_shards); each device stages, hashes and verifies its shard
 * (messages of the shard only), and the per-device accept bitmasks come back
 * through ONE RCCL all-gather (ncclAllGather over xGMI, librccl loaded at
 * bv_group_create) into device 0, from which the merged bitmask is copied
 * once.  Digests and statuses come back per device.  Errors: BV_E_COMM if
 * RCCL is unavailable or a collective fails; BV_E_ARGS if a device appears
 * twice in a list of several devices.  A list naming ONE device n times
 * makes n logical shards on it (one ctx each, no RCCL: the shard bitmasks
 * are gathered by device copies; the key-cache budget is split between the
 * shards). */
typedef struct bv_group bv_group;
int bv_group_create(bv_group **out, const int *devices, int n_devices, uint32_t flags);
void bv_group_destroy(bv_group *g);
const char *bv_group_last_error(const bv_group *g);
int bv_group_verify_batch(bv_group *g, const bv_batch *batch, bv_result *result);
/* Timing of the last group call on device slot `i` (its ctx's bv_timing). */
int bv_group_get_timing(const bv_group *g, int i, bv_timing *out);
/* Host helper (no device): the shard plan bv_group_verify_batch uses.
 * Writes n_shards + 1 item bounds (bounds[0] = 0, bounds[n] = n_items). */
int bv_plan_shards(const bv_batch *batch, int n_shards, uint64_t *bounds);
/* Host helper (no device): the bitmask merge bv_group_verify_batch does
 * after its all-gather.  Shard d's words start at gathered[d *
 * words_per_shard]; its bit 0 is item bounds[d].  Writes
 * ceil(bounds[n_shards] / 64) words to `out`; BV_E_ARGS on non-monotone
 * bounds or a shard wider than words_per_shard words.
 * bv_group_verify_batch accepts items in any message order: the items are
 * sorted by message (stably) for sharding, the messages are partitioned into
 * contiguous device ranges (each hashed once, also messages no item names),
 * and statuses / bits come back in the caller's item order. */
int bv_merge_shard_bits(const uint64_t *gathered, uint64_t words_per_shard, int n_shards,
                        const uint64_t *bounds, uint64_t *out);
/* Host helper (no device): the whole plan of bv_group_verify_batch.  perm
 * (n_items entries, may be NULL): the item order used, perm[j] = the caller's
 * index of the j-th item (identity when item_msg is non-decreasing);
 * item_bounds (n_shards + 1): the shards over that order (bv_plan_shards);
 * msg_bounds (n_shards + 1): device d hashes messages [msg_bounds[d],
 * msg_bounds[d+1]) — a partition of [0, n_msgs).  Returns 1 when the items
 * were permuted, 0 when not, BV_E_ARGS on bad arguments. */
int bv_plan_group(const bv_batch *batch, int n_shards, uint64_t *item_bounds, uint64_t *msg_bounds,
                  uint32_t *perm);

/* bv_verify_events over the group: events from their wire fields, sharded by
 * event index.  The result contract is bv_verify_events' (msg_hash 32 * n
 * bytes, status n bytes, accept_bits ceil(n / 64) words, any of them NULL;
 * buffers in bv_host_alloc memory are reached by DMA in place), and so are
 * the validation rules and their BV_E_ARGS cases, checked once over the whole
 * batch; more than 2^32 events are BV_E_ARGS too.
 * A batch without BV_PARENT_EVENT parents (a store / Bootstrap replay) is cut
 * into contiguous event shards of whole 64-event words, one per device slot
 * (bv_plan_event_shards).  Each slot stages, builds, hashes and verifies only
 * its shard, concurrently, and writes its digests and statuses straight into
 * the caller's buffers; the accept bitmasks come back through the same gather
 * as bv_group_verify_batch's.  A shard ships the keys (whole), its slice of
 * every per-event array, of the transactions, the fragments and the signature
 * text, and the parent hashes [hash_lo, hash_hi) its BV_PARENT_HASH parents
 * name.  The slices keep the caller's offsets and indices (nothing is
 * rewritten on the host): the device subtracts the shard's bases.  A caller
 * that lists parent_hashes in first-use order ships about 1 / n_devices of
 * them per device; any other order is as correct but ships more (up to all of
 * them to every device).
 * A batch WITH in-batch parents (a SyncResponse DAG) is not sharded: it runs
 * as one bv_verify_events call on device slot 0.
 * After a failed call nothing stays in flight on any slot. */
int bv_group_verify_events(bv_group *g, const bv_event_batch *events, bv_result *result);
/* bv_kc_register on every slot's context (a BV_F_KEY_CACHE group's validator
 * set; without it the slots' caches fill by the seen-twice rule only).
 * Returns the first slot's failure, its text in bv_group_last_error;
 * BV_E_ARGS on a group created without BV_F_KEY_CACHE. */
int bv_group_kc_register(bv_group *g, uint32_t n_keys, const uint8_t *key_bytes, const uint64_t *key_off);
/* Host helper (no device): the plan bv_group_verify_events follows.  Returns
 * 0 for a batch without BV_PARENT_EVENT parents: event_bounds (n_shards + 1)
 * are multiples of 64 except that the last non-empty shard ends at n_events
 * (ceil(words / n_shards) 64-event words per shard; trailing shards may be
 * empty), and [hash_lo[d], hash_hi[d]) spans the smallest to the largest
 * parent_ref among shard d's BV_PARENT_HASH parents (0, 0 without one).
 * Returns 1 for a batch with in-batch parents: event_bounds = {0, n, n, ...}
 * and shard 0's hash range is computed the same way.  BV_E_ARGS on NULL
 * pointers, n_shards <= 0, an unknown parent kind or a BV_PARENT_HASH ref >=
 * n_parent_hashes.  Only n_events, parent_kind, parent_ref and
 * n_parent_hashes are read. */
int bv_plan_event_shards(const bv_event_batch *events, int n_shards, uint64_t *event_bounds, uint64_t *hash_lo,
                         uint64_t *hash_hi);

/* bv_verify_events_itx / bv_verify_events_fields over the group: the whole of
 * Event.Verify in one call, sharded by event index.  The result contract, the
 * validation rules with their BV_E_ARGS cases and texts (checked once over the
 * whole batch; the text in bv_group_last_error), the pinned-memory rule for
 * the inputs and the semantics of `out` are exactly those of the
 * single-context entries; msg_hash, status, accept_bits, out and every member
 * of out may be NULL.  The fall-back equalities hold through the group too:
 * n_itx == 0 (bv_group_verify_events_itx) returns what bv_group_verify_events
 * returns for the same events with nil or "[]" fragments, n_bsig == 0
 * (bv_group_verify_events_fields) what bv_group_verify_events_itx (for a NULL
 * itx_start: bv_group_verify_events) returns.
 * A batch without BV_PARENT_EVENT parents that the single-context entry would
 * send down its bulk pipeline is cut at the bounds of bv_plan_event_shards
 * (whole 64-event words per slot, trailing shards possibly empty): the shards
 * are balanced by EVENTS, not by items, because ITXs are rare.  Shard [a, z)
 * owns the ITXs [itx_start[a], itx_start[z]), the block signatures
 * [bsig_start[a], bsig_start[z]), the transactions [tx_start[a], tx_start[z])
 * and the parent hashes [hash_lo, hash_hi) (bv_plan_event_fields_shards); its
 * items are its events followed by its ITXs.  Every non-empty shard takes the
 * bulk pipeline on its slot, however small it is (an empty shard launches
 * nothing).  It ships the creators' keys whole, then the distinct decoded keys
 * of its own ITXs (the key cache is resolved per slot on those), its event
 * range of every per-event array, its ITX range of itx_type, itx_str_off and
 * the string bytes, its block-signature range of the bsig_* arrays and their
 * bytes, its transaction slices, parent-hash range and signature text.  The
 * slices keep the caller's values (nothing is rewritten on the host; arrays in
 * bv_host_alloc memory cross by DMA from where they lie): the device subtracts
 * the shard's bases.  Each slot's msg_hash, status, decided_by, itx_hash and
 * itx_status land in the caller's buffers at its event / ITX bounds, copied by
 * the host out of the slot's pinned result block as the single-context entries
 * copy theirs (not by DMA into pinned caller buffers); only the accept
 * bitmasks go through the gather of bv_group_verify_batch.
 * A batch WITH in-batch parents (a SyncResponse DAG), or one the
 * single-context entry runs on its one-launch small path (its routing
 * decision, for the whole batch), is not sharded: it runs as one
 * single-context call on device slot 0.
 * After a failed call nothing stays in flight on any slot. */
int bv_group_verify_events_itx(bv_group *g, const bv_event_itx_batch *batch, bv_result *result,
                               bv_event_itx_out *out /* may be NULL */);
int bv_group_verify_events_fields(bv_group *g, const bv_event_fields_batch *batch, bv_result *result,
                                  bv_event_itx_out *out /* may be NULL */);
/* Host helper (no device): the plan the two entries above follow.
 * event_bounds, hash_lo, hash_hi and the return value (1: a batch with
 * in-batch parents, whole on shard 0) are bv_plan_event_shards'; itx_bounds[d]
 * = ev.itx_start[event_bounds[d]] (all 0 when ev.itx_start is NULL) and
 * bsig_bounds[d] = bsig_start[event_bounds[d]], n_shards + 1 entries each.
 * Reads only n_events, parent_kind, parent_ref, n_parent_hashes and those two
 * start arrays at the bounds.  BV_E_ARGS on NULL pointers (bsig_start may be
 * NULL only with n_events == 0), n_shards <= 0 and everything
 * bv_plan_event_shards rejects. */
int bv_plan_event_fields_shards(const bv_event_fields_batch *batch, int n_shards, uint64_t *event_bounds,
                                uint64_t *itx_bounds, uint64_t *bsig_bounds, uint64_t *hash_lo, uint64_t *hash_hi);

/* Blocks from their fields: Block.Verify (src/hashgraph/block.go:343-357),
 * CheckBlock (hashgraph.go:1599-1630), ProcessSigPool and the fast-forward
 * check without the caller serialising anything.  Instead of
 * BlockBody.Marshal() per block the caller passes the BlockBody's fields
 * (block.go:16-26); the device builds every canonical body (Go 1.13
 * encoding/json of the exported fields in declaration order, then '\n',
 * bit-exact), hashes it as it is built (no body is stored) and verifies the
 * block signatures listed as items over blocks and validator keys, as
 * bv_batch items are over messages.  Bodies longer than 16 KiB are built and
 * hashed by the library's host threads beside the device's hashing; a batch
 * that bv_verify_batch_text would run on its one-launch small path (same item
 * count and keys) has its bodies built on the host and takes that path. */
typedef struct {
  uint64_t n_blocks;
  const int64_t *index, *round_received, *timestamp; /* per block (Go int / int64)      */
  /* StateHash, FrameHash, PeersHash: 3 byte strings per block, in that order */
  const uint64_t *hash_off;   /* 3 * n_blocks + 1 offsets into hash_bytes (any length)  */
  const uint8_t *hash_bytes;
  const uint8_t *hash_nil;    /* 3 per block, 1: that []byte is nil -> null (NULL: none) */
  /* Transactions, exactly as in bv_event_batch */
  const uint64_t *tx_start;   /* n_blocks + 1 */
  const uint64_t *tx_off; const uint8_t *tx_bytes;
  const uint8_t *tx_list_nil; /* per block */
  const uint8_t *tx_nil;      /* per tx    */
  /* verbatim encoding/json of the slices; an empty fragment = nil -> null ("[]" is a fragment);
   * a NULL offset array: every block's slice is nil */
  const uint64_t *itx_off;  const uint8_t *itx_json;   /* InternalTransactions        */
  const uint64_t *rcpt_off; const uint8_t *rcpt_json;  /* InternalTransactionReceipts */
  /* the signatures: items over blocks and validator keys, as bv_batch items over messages */
  uint32_t n_keys; const uint8_t *key_bytes; const uint64_t *key_off;
  uint64_t n_items;
  const uint32_t *item_block, *item_key;
  const uint64_t *sig_off; const uint8_t *sig_text;    /* BlockSignature.Signature text, OR */
  const uint8_t *r_be, *s_be, *pre;                    /* host-decoded, as bv_event_batch   */
} bv_block_batch;

/* The result contract is bv_verify_batch_text's: msg_hash is 32 * n_blocks
 * bytes and holds every BlockBody.Hash (a block without items is still
 * hashed); status and accept_bits are per item, in the caller's item order,
 * and the items may come in any block order; the pinned-memory rule (every
 * array and result buffer in bv_host_alloc memory moves by DMA in place), the
 * threading and the bv_last_error texts are the same.  When sig_text is
 * non-NULL r_be / s_be / pre are ignored.
 * valid_count (n_blocks words, may be NULL): valid_count[b] = the number of
 * items of block b whose status is BV_ACCEPT, tallied on the device (on the
 * host for a batch that takes the one-launch small path, whose statuses are
 * written into host memory) — CheckBlock's count.  A caller that passes
 * status == NULL gets 4 * n_blocks bytes back instead of a per-item array.
 * The caller lists ONLY the signatures of validators in the block's peer
 * set: CheckBlock skips the others before Block.Verify (Go `continue`s,
 * hashgraph.go:1612-1616), so they must not be counted.  BV_REF_PANIC items
 * count as not accepted and stay visible in status.
 * BV_E_ARGS (with a bv_last_error text): a NULL required array, offsets that
 * are not monotone or do not start at 0, item_block >= n_blocks, item_key >=
 * n_keys, more than 2^32 blocks, neither sig_text nor r_be / s_be, and
 * everything bv_verify_batch_text rejects for sig_off / sig_text.  n_blocks
 * == 0 and n_items == 0 are BV_OK. */
int bv_verify_blocks(bv_ctx *ctx, const bv_block_batch *blocks, bv_result *result,
                     uint32_t *valid_count /* n_blocks, may be NULL */);
/* Host helpers (no device): the serialiser bv_verify_blocks runs, as
 * bv_decode_signatures is the parser's public form.  bv_block_body_lens
 * writes n_blocks + 1 offsets (body_off[0] = 0, body b is body_off[b+1] -
 * body_off[b] bytes long); bv_block_bodies writes body b at out +
 * body_off[b] for any monotone body_off that leaves each body its length.
 * Only the block fields are read (not the keys or items).  BV_E_ARGS on a
 * NULL pointer, on block offsets that are not monotone or do not start at 0
 * and on a body_off slot shorter than its body; n_blocks == 0 is BV_OK. */
int bv_block_body_lens(const bv_block_batch *blocks, uint64_t *body_off /* n_blocks + 1 */);
int bv_block_bodies(const bv_block_batch *blocks, const uint64_t *body_off, uint8_t *out);

/* bv_verify_blocks over the group: blocks from their fields, sharded by block
 * (each block's signatures stay on one device, so its count is local).  The
 * result contract, the validation rules with their BV_E_ARGS cases and texts
 * (checked once over the whole batch) and the pinned-memory rule are
 * bv_verify_blocks'; msg_hash, status, accept_bits and valid_count may each
 * be NULL (status == NULL with valid_count included).
 * A batch whose item_block is non-decreasing is cut by bv_plan_block_shards:
 * item shards balanced by count that never split a block's items, and a
 * partition of the blocks, so blocks without items are hashed too.  Each
 * non-empty shard takes the bulk pipeline on its slot, however small it is
 * (an empty shard launches nothing), and writes its digests, statuses and
 * counts straight into the caller's buffers at its block / item bounds; only
 * the accept bitmasks go through the gather of bv_group_verify_batch, merged
 * at the item bounds (not multiples of 64).  A shard ships the keys (whole),
 * its block range of every per-block array, the matching ranges of the hash,
 * transaction and fragment bytes, and its item range of item_block, item_key
 * and the signature text or r_be / s_be / pre.  The slices keep the caller's
 * values (nothing is rewritten on the host): the device subtracts the shard's
 * bases.
 * A batch whose items are NOT sorted by block, or that bv_verify_blocks runs
 * on its one-launch small path (its routing decision, for the whole batch),
 * is not sharded: it runs as one bv_verify_blocks call on device slot 0.
 * After a failed call nothing stays in flight on any slot. */
int bv_group_verify_blocks(bv_group *g, const bv_block_batch *blocks, bv_result *result,
                           uint32_t *valid_count /* n_blocks, may be NULL */);
/* Host helper (no device): the plan bv_group_verify_blocks follows.  Only
 * n_blocks, n_items and item_block are read.  Returns 0 when item_block is
 * non-decreasing: the plan is bv_plan_group's for a bv_batch with item_msg =
 * item_block and n_msgs = n_blocks (item_bounds: bv_plan_shards'; block_bounds:
 * its msg_bounds, a partition of [0, n_blocks)).  Returns 1 when it is not
 * sorted: block_bounds = {0, n_blocks, n_blocks, ...}, item_bounds = {0,
 * n_items, n_items, ...} (the whole batch on slot 0).  BV_E_ARGS on NULL
 * pointers, n_shards <= 0 or item_block >= n_blocks. */
int bv_plan_block_shards(const bv_block_batch *blocks, int n_shards, uint64_t *block_bounds /* n_shards + 1 */,
                         uint64_t *item_bounds /* n_shards + 1 */);

/* SHA-256 of n messages (host buffers) -> 32*n bytes. */
int bv_sha256_batch(bv_ctx *ctx, uint64_t n_msgs, const uint8_t *msg_bytes,
                    const uint64_t *msg_off, uint8_t *out_hash);

/* PeerSet.Hash (src/peers/peer_set.go:104-115): h = [] then h = SHA256(h ||
 * pubkey) over the n peers' raw key bytes in order (PubKeyBytes), as ONE
 * device launch (the chain is serial).  n_peers == 0: the hash is empty
 * ([]byte{}) and out_hash is not written. */
int bv_peer_set_hash(bv_ctx *ctx, uint32_t n_peers, const uint8_t *key_bytes, const uint64_t *key_off,
                     uint8_t out_hash[32]);

/* Device-timing breakdown of the last verify call on this ctx. */
int bv_get_timing(const bv_ctx *ctx, bv_timing *out);

/* Host helpers mirroring the Go parsing semantics (no device needed). */
/* keys.DecodeSignature + classification: writes 32-byte BE r,s (zero when the
 * class is not OK) and returns the pre byte. */
uint8_t bv_decode_signature(const char *sig, size_t len, uint8_t r_be[32], uint8_t s_be[32]);
/* bv_decode_signature over n texts in one call: text i is sig_text[sig_off[i]
 * .. sig_off[i+1]); writes 32 * n bytes of r and of s (zero where the class is
 * not OK, as above) and n pre bytes.  BV_OK, or BV_E_ARGS on a NULL pointer
 * (sig_text may be NULL when every text is empty) or offsets that are not
 * monotone; n == 0 is BV_OK and reads nothing. */
int bv_decode_signatures(uint64_t n, const uint64_t *sig_off, const uint8_t *sig_text,
                         uint8_t *r_be, uint8_t *s_be, uint8_t *pre);
/* common.DecodeFromString: hex.DecodeString(s[2:]) keeping the prefix decoded
 * before the first error.  Returns the decoded length, or -1 where Go panics
 * (len < 2).  `out` must hold (len-2)/2 bytes. */
int64_t bv_hex_decode(const char *s, size_t len, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BABBLEVERIFY_H */
