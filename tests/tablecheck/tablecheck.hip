// tablecheck.hip — TEST INFRASTRUCTURE (tests/test_gpu_table_audit.py): audits
// every required entry of the fixed-base tables on the device with the
// relations of audit.h.  The tables are built by the library's own exported
// builders (bvk::build_tables, bvk::build_kc) into guarded buffers of this
// harness, or read from a live context (its generator table, its cached key
// tables), which the harness only ever reads.  Nothing of the library changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../babble_amd/csrc/bv_internal.h"
#include "audit.h"

namespace {

constexpr size_t kGuard = 4096;     // bytes before and after every buffer a builder writes
constexpr uint32_t kMaxRec = 64;    // failures recorded
constexpr uint32_t kPattern = 0xA5A5A5A5u;

struct tc_dev {  // device-side results
  unsigned long long fails, audited;
  uint32_t rec[kMaxRec * 4];  // (relation, key, window, digit) of the first failures, in atomic order
};

enum { LAYOUT_SIGNED = 0, LAYOUT_SIGNED_PHI = 1, LAYOUT_UNSIGNED_PHI = 2 };

// One lane per (key, window, digit): grid (ceil(nwin * ent / 256), n_keys).
// A signed window's lane r audits digit r + 1 (1 .. 2^(W-1)), an unsigned
// window's lane r slot r (0: the identity).  Lanes past a window's last
// required digit do nothing.
template <int LAYOUT>
__global__ void __launch_bounds__(256) k_audit(tc_geom g, const uint64_t *__restrict__ tabs,
                                               const uint32_t *__restrict__ kxy, const uint8_t *__restrict__ kstatus,
                                               tc_dev *__restrict__ out) {
  constexpr bool SIGNED = LAYOUT != LAYOUT_UNSIGNED_PHI;
  const uint32_t key = blockIdx.y;
  if (kstatus && kstatus[key] != KS_OK) return;  // uniform per block
  const uint64_t ent = tc_ent(g), i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t j = (uint32_t)(i / ent);
  const uint64_t d = i % ent + (SIGNED ? 1 : 0);
  const bool live = j < g.nwin && d <= tc_required(g, j);
  const uint32_t *tab = (const uint32_t *)tabs[key];
  uint32_t bad = 0;
  if (live)
    bad = SIGNED ? tc_audit_signed(g, tab, kxy + (uint64_t)key * TC_ENTRY_U32, j, d)
                 : tc_audit_unsigned(g, tab, kxy + (uint64_t)key * TC_ENTRY_U32, j, d);
  const int n = __syncthreads_count(live && d != 0);
  if (threadIdx.x == 0 && n) atomicAdd(&out->audited, (unsigned long long)n * (g.phi ? 2 : 1));
  for (uint32_t r = 0; bad; r++, bad >>= 1) {
    if (!(bad & 1u)) continue;
    const unsigned long long at = atomicAdd(&out->fails, 1ull);
    if (at < kMaxRec) {
      out->rec[4 * at] = r;
      out->rec[4 * at + 1] = key;
      out->rec[4 * at + 2] = j;
      out->rec[4 * at + 3] = (uint32_t)d;
    }
  }
}

// bytes of [p, p + 4 n) that no longer hold the fill pattern
__global__ void __launch_bounds__(256) k_count_changed(const uint32_t *__restrict__ p, uint64_t n,
                                                       unsigned long long *__restrict__ cnt) {
  unsigned long long c = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t x = p[i] ^ kPattern;
    c += ((x & 0xFFu) != 0) + ((x & 0xFF00u) != 0) + ((x & 0xFF0000u) != 0) + ((x & 0xFF000000u) != 0);
  }
  if (c) atomicAdd(cnt, c);
}

struct Guarded {  // a device buffer between two guard regions, all filled with the pattern
  uint8_t *raw = nullptr;
  size_t bytes = 0;
  ~Guarded() {
    if (raw) (void)hipFree(raw);
  }
  hipError_t alloc(size_t n) {
    bytes = n;
    hipError_t e = hipMalloc((void **)&raw, n + 2 * kGuard);
    if (e == hipSuccess) e = hipMemset(raw, 0xA5, n + 2 * kGuard);
    return e;
  }
  template <class T>
  T *as() const {
    return (T *)(raw + kGuard);
  }
};

struct Plain {
  void *p = nullptr;
  ~Plain() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n); }
};

}  // namespace

extern "C" {

struct tc_result {
  uint64_t failures;  // relations that failed (all of them, not only the recorded ones)
  uint64_t audited;   // required entries audited, both halves counted
  uint64_t changed;   // guard bytes, and table bytes of skipped keys, that lost the pattern
  uint32_t n_rec;     // recorded failures, sorted
  float audit_ms;     // the audit kernel alone
  uint32_t rec[kMaxRec * 4];
  char err[160];
};

}  // extern "C"

namespace {

bool geom_of(int kw, tc_geom &g) {
  switch (kw) {
    case 0: g = {BV_GW, BV_GNWIN, 256, 1, 0}; return tc_table_u32(g) == BV_GTABLE_U32;
    case 8: g = {BV_KW, BV_KNWIN, 128, 0, 1}; return tc_table_u32(g) == BV_KTABLE_U32;
    case 12: g = {BV_K12W, BV_K12NWIN, 128, 1, 1}; return tc_table_u32(g) == BV_K12TABLE_U32;
    case BV_KCW: g = {BV_KCW, BV_KCNWIN, 128, 1, 0}; return tc_table_u32(g) == BV_KCTABLE_U32;
    case BV_KC18W: g = {BV_KC18W, BV_KC18NWIN, 128, 1, 0}; return tc_table_u32(g) == BV_KC18TABLE_U32;
  }
  return false;
}

int fail(tc_result *res, const char *what, hipError_t e) {
  snprintf(res->err, sizeof res->err, "%s: %s", what, e == hipSuccess ? "invalid" : hipGetErrorString(e));
  (void)hipGetLastError();
  return e == hipSuccess ? -1 : -(int)e;
}
#define TC_CK(expr, what)                              \
  do {                                                 \
    const hipError_t e_ = (expr);                      \
    if (e_ != hipSuccess) return fail(res, what, e_);  \
  } while (0)

// the audit over per-key table pointers (host array), results into res
int audit(hipStream_t st, const tc_geom &g, uint32_t n_keys, const uint64_t *h_tabs, const uint32_t *h_kxy,
          const uint8_t *d_kst, tc_result *res) {
  if (n_keys == 0 || n_keys > 65535) return fail(res, "key count", hipSuccess);
  // only the top window may be partial: R2 reads the digit 2^(W-1) of every window below it
  for (uint32_t j = 0; j + 1 < g.nwin; j++)
    if (g.is_signed && tc_required(g, j) != tc_ent(g)) return fail(res, "geometry: partial inner window", hipSuccess);
  Plain d_tabs, d_kxy, d_out;
  TC_CK(d_tabs.alloc(n_keys * 8ull), "alloc tabs");
  TC_CK(d_kxy.alloc(n_keys * 64ull), "alloc kxy");
  TC_CK(d_out.alloc(sizeof(tc_dev)), "alloc out");
  TC_CK(hipMemcpyAsync(d_tabs.p, h_tabs, n_keys * 8ull, hipMemcpyHostToDevice, st), "h2d tabs");
  TC_CK(hipMemcpyAsync(d_kxy.p, h_kxy, n_keys * 64ull, hipMemcpyHostToDevice, st), "h2d kxy");
  TC_CK(hipMemsetAsync(d_out.p, 0, sizeof(tc_dev), st), "zero out");
  hipEvent_t e0, e1;
  TC_CK(hipEventCreate(&e0), "event");
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return fail(res, "event", hipErrorOutOfMemory);
  }
  const uint64_t lanes = (uint64_t)g.nwin * tc_ent(g);
  const dim3 grid((uint32_t)((lanes + 255) / 256), n_keys);
  (void)hipEventRecord(e0, st);
  if (!g.is_signed)
    hipLaunchKernelGGL(k_audit<LAYOUT_UNSIGNED_PHI>, grid, dim3(256), 0, st, g, (const uint64_t *)d_tabs.p,
                       (const uint32_t *)d_kxy.p, d_kst, (tc_dev *)d_out.p);
  else if (g.phi)
    hipLaunchKernelGGL(k_audit<LAYOUT_SIGNED_PHI>, grid, dim3(256), 0, st, g, (const uint64_t *)d_tabs.p,
                       (const uint32_t *)d_kxy.p, d_kst, (tc_dev *)d_out.p);
  else
    hipLaunchKernelGGL(k_audit<LAYOUT_SIGNED>, grid, dim3(256), 0, st, g, (const uint64_t *)d_tabs.p,
                       (const uint32_t *)d_kxy.p, d_kst, (tc_dev *)d_out.p);
  hipError_t e = hipGetLastError();
  (void)hipEventRecord(e1, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) (void)hipEventElapsedTime(&res->audit_ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  TC_CK(e, "k_audit");
  tc_dev out;
  TC_CK(hipMemcpy(&out, d_out.p, sizeof out, hipMemcpyDeviceToHost), "d2h out");
  res->failures = out.fails;
  res->audited = out.audited;
  res->n_rec = (uint32_t)std::min<unsigned long long>(out.fails, kMaxRec);
  std::vector<std::array<uint32_t, 4>> v(res->n_rec);
  for (uint32_t i = 0; i < res->n_rec; i++) memcpy(v[i].data(), out.rec + 4 * i, 16);
  std::sort(v.begin(), v.end());  // the atomic order is not deterministic
  for (uint32_t i = 0; i < res->n_rec; i++) memcpy(res->rec + 4 * i, v[i].data(), 16);
  return 0;
}

// entries (key, slot) copied out: 32 words each, the plain entry then the phi entry (zeros without a phi half)
int gather(const tc_geom &g, uint32_t n_keys, const uint64_t *h_tabs, uint32_t n, const uint32_t *gkey,
           const uint64_t *gslot, uint32_t *gout, tc_result *res) {
  const uint64_t slots = tc_half_u32(g) / TC_ENTRY_U32;
  for (uint32_t i = 0; i < n; i++) {
    if (gkey[i] >= n_keys || gslot[i] >= slots) return fail(res, "gather index", hipSuccess);
    const uint32_t *e = (const uint32_t *)h_tabs[gkey[i]] + gslot[i] * TC_ENTRY_U32;
    memset(gout + 32ull * i, 0, 128);
    TC_CK(hipMemcpy(gout + 32ull * i, e, 64, hipMemcpyDeviceToHost), "gather");
    if (g.phi) TC_CK(hipMemcpy(gout + 32ull * i + 16, e + tc_half_u32(g), 64, hipMemcpyDeviceToHost), "gather phi");
  }
  return 0;
}

struct Corrupt {
  uint32_t kind, key, win;
  uint64_t digit;
};
enum { C_NONE = 0, C_FLIP_X = 1, C_NEG_Y = 2, C_SWAP_NEXT = 3, C_NEXT_WINDOW = 4, C_PHI_PLAIN_X = 5 };

// one named corruption of a required slot, in the harness's own table
int corrupt(const tc_geom &g, uint32_t *table, const Corrupt &c, tc_result *res) {
  if (c.win + 1 >= g.nwin || c.digit < 1 || c.digit > tc_required(g, c.win)) return fail(res, "corrupt slot", hipSuccess);
  if (c.kind == C_SWAP_NEXT && c.digit + 1 > tc_required(g, c.win)) return fail(res, "corrupt slot", hipSuccess);
  if (c.kind == C_NEXT_WINDOW && c.digit > tc_required(g, c.win + 1)) return fail(res, "corrupt slot", hipSuccess);
  const uint64_t half = tc_half_u32(g);
  uint32_t *e = table + c.key * tc_table_u32(g) + tc_slot(g, c.win, c.digit) * TC_ENTRY_U32;
  uint32_t a[16], b[16];
  TC_CK(hipMemcpy(a, e, 64, hipMemcpyDeviceToHost), "read entry");
  switch (c.kind) {
    case C_FLIP_X:
      a[0] ^= 1u;
      TC_CK(hipMemcpy(e, a, 64, hipMemcpyHostToDevice), "write entry");
      break;
    case C_NEG_Y: {  // p - y: still on the curve
      const uint32_t p[8] = {P0, P1, PX, PX, PX, PX, PX, PX};
      uint64_t br = 0;
      for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)p[i] - a[8 + i] - br;
        a[8 + i] = (uint32_t)t;
        br = (t >> 32) & 1;
      }
      TC_CK(hipMemcpy(e, a, 64, hipMemcpyHostToDevice), "write entry");
      break;
    }
    case C_SWAP_NEXT:
    case C_NEXT_WINDOW: {  // both halves, as an indexing slip of a builder would
      uint32_t *o = table + c.key * tc_table_u32(g) +
                    (c.kind == C_SWAP_NEXT ? tc_slot(g, c.win, c.digit + 1) : tc_slot(g, c.win + 1, c.digit)) * TC_ENTRY_U32;
      for (int h = 0; h < (g.phi ? 2 : 1); h++) {
        TC_CK(hipMemcpy(a, e + h * half, 64, hipMemcpyDeviceToHost), "read entry");
        TC_CK(hipMemcpy(b, o + h * half, 64, hipMemcpyDeviceToHost), "read entry");
        TC_CK(hipMemcpy(e + h * half, b, 64, hipMemcpyHostToDevice), "write entry");
        if (c.kind == C_SWAP_NEXT) TC_CK(hipMemcpy(o + h * half, a, 64, hipMemcpyHostToDevice), "write entry");
      }
      break;
    }
    case C_PHI_PLAIN_X:
      if (!g.phi) return fail(res, "no phi half", hipSuccess);
      TC_CK(hipMemcpy(e + half, a, 32, hipMemcpyHostToDevice), "write phi x");
      break;
    default:
      return fail(res, "corruption kind", hipSuccess);
  }
  return 0;
}

// Build the tables of n_keys keys with the library's builder into guarded,
// pattern-filled buffers of the sizes the library allocates for this geometry
// (bv_api.cpp bv_run_keys, bv_keycache.cpp bv_kc_prepare), audit them, and
// count the guard and skipped-key bytes that changed.
int build_audit(int kw, uint32_t n_keys, const uint32_t *kxy, const uint8_t *kstatus, uint64_t n_items,
                const Corrupt *c, uint32_t n_gather, const uint32_t *gkey, const uint64_t *gslot, uint32_t *gout,
                tc_result *res) {
  memset(res, 0, sizeof *res);
  tc_geom g;
  if (kw == 0 || !geom_of(kw, g)) return fail(res, "geometry", hipSuccess);
  if (n_keys == 0 || !kxy || !kstatus) return fail(res, "arguments", hipSuccess);
  const bool cached = BV_W_IS_CACHED(kw);
  const size_t table_bytes = tc_table_u32(g) * 4;
  const size_t bases_bytes = (size_t)n_keys * (cached ? 22 : 32) * 96;
  const size_t sub_bytes = (size_t)n_keys * (cached ? bvk::kc_sub_bytes(kw) : kw == 12 ? BV_K12SUB_U32 * 4 : BV_KSUB_U32 * 4);
  const size_t pscr_bytes = (size_t)n_keys * (cached    ? bvk::kc_pscr_bytes(kw)
                                              : kw == 12 ? (size_t)BV_K12NWIN * BV_K12ENT * 32
                                                         : (size_t)BV_KNWIN * (1u << BV_KW) * 32);
  if (cached && bvk::kc_table_bytes(kw) != table_bytes) return fail(res, "cached table size", hipSuccess);
  Guarded bases, sub, pscr;
  std::vector<Guarded> tables(cached ? n_keys : 1);  // cached tables: one allocation per key
  TC_CK(bases.alloc(bases_bytes), "alloc bases");
  TC_CK(sub.alloc(sub_bytes), "alloc sub-tables");
  TC_CK(pscr.alloc(pscr_bytes), "alloc prefix scratch");
  for (Guarded &t : tables) TC_CK(t.alloc(cached ? table_bytes : table_bytes * n_keys), "alloc tables");
  std::vector<uint64_t> h_tabs(n_keys);
  for (uint32_t k = 0; k < n_keys; k++)
    h_tabs[k] = (uint64_t)(uintptr_t)(cached ? tables[k].as<uint8_t>() : tables[0].as<uint8_t>() + k * table_bytes);
  Plain d_kxy, d_kst, d_tabs, d_cnt;
  TC_CK(d_kxy.alloc(n_keys * 64ull), "alloc kxy");
  TC_CK(d_kst.alloc(n_keys), "alloc kstatus");
  TC_CK(d_tabs.alloc(n_keys * 8ull), "alloc tabs");
  TC_CK(d_cnt.alloc(8), "alloc counter");
  TC_CK(hipMemcpy(d_kxy.p, kxy, n_keys * 64ull, hipMemcpyHostToDevice), "h2d kxy");
  TC_CK(hipMemcpy(d_kst.p, kstatus, n_keys, hipMemcpyHostToDevice), "h2d kstatus");
  TC_CK(hipMemcpy(d_tabs.p, h_tabs.data(), n_keys * 8ull, hipMemcpyHostToDevice), "h2d tabs");
  TC_CK(hipMemset(d_cnt.p, 0, 8), "zero counter");
  hipStream_t st;
  TC_CK(hipStreamCreate(&st), "stream");
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } sg{st};
  const hipError_t be =
      cached ? bvk::build_kc(st, kw, n_keys, (const uint32_t *)d_kxy.p, (const uint8_t *)d_kst.p, bases.as<uint32_t>(),
                             sub.as<uint32_t>(), pscr.as<uint32_t>(), (const uint64_t *)d_tabs.p)
             : bvk::build_tables(st, kw, n_keys, (const uint32_t *)d_kxy.p, (const uint8_t *)d_kst.p,
                                 bases.as<uint32_t>(), sub.as<uint32_t>(), pscr.as<uint32_t>(),
                                 tables[0].as<uint32_t>(), n_items);
  TC_CK(be, "build");
  TC_CK(hipStreamSynchronize(st), "build sync");
  if (c) {
    if (cached || c->key >= n_keys || kstatus[c->key] != KS_OK) return fail(res, "corrupt key", hipSuccess);
    const int rc = corrupt(g, tables[0].as<uint32_t>(), *c, res);
    if (rc) return rc;
  }
  int rc = audit(st, g, n_keys, h_tabs.data(), kxy, (const uint8_t *)d_kst.p, res);
  if (rc) return rc;
  // guards of every buffer, and the whole table of every skipped key
  auto count = [&](const uint8_t *p, size_t n) {
    hipLaunchKernelGGL(k_count_changed, dim3((uint32_t)std::min<uint64_t>((n / 4 + 255) / 256, 4096)), dim3(256), 0, st,
                       (const uint32_t *)p, (uint64_t)(n / 4), (unsigned long long *)d_cnt.p);
    return hipGetLastError();
  };
  std::vector<const Guarded *> all = {&bases, &sub, &pscr};
  for (const Guarded &t : tables) all.push_back(&t);
  for (const Guarded *b : all) {
    TC_CK(count(b->raw, kGuard), "guard check");
    TC_CK(count(b->raw + kGuard + b->bytes, kGuard), "guard check");
  }
  for (uint32_t k = 0; k < n_keys; k++)
    if (kstatus[k] != KS_OK) TC_CK(count((const uint8_t *)(uintptr_t)h_tabs[k], table_bytes), "skipped-key check");
  TC_CK(hipStreamSynchronize(st), "check sync");
  TC_CK(hipMemcpy(&res->changed, d_cnt.p, 8, hipMemcpyDeviceToHost), "d2h counter");
  if (n_gather) rc = gather(g, n_keys, h_tabs.data(), n_gather, gkey, gslot, gout, res);
  return rc;
}

}  // namespace

extern "C" {

// kw 8 / 12: bvk::build_tables (n_items only selects the build variant); kw
// 22 / 18: bvk::build_kc.  kxy: 16 words per key, kstatus: one byte per key
// (host arrays).  gout: 32 words per gathered (key, slot).  Returns 0, or a
// negative code with res->err set.
int tc_build_audit(int kw, uint32_t n_keys, const uint32_t *kxy, const uint8_t *kstatus, uint64_t n_items,
                   uint32_t n_gather, const uint32_t *gkey, const uint64_t *gslot, uint32_t *gout, tc_result *res) {
  return build_audit(kw, n_keys, kxy, kstatus, n_items, nullptr, n_gather, gkey, gslot, gout, res);
}

// The negative control: the same build (kw 8 or 12, n_items 1) with one named
// corruption applied to digit `digit` of window `win` of key `key` in the
// harness's copy before the audit.
int tc_corrupt_audit(int kw, uint32_t n_keys, const uint32_t *kxy, const uint8_t *kstatus, uint32_t kind, uint32_t key,
                     uint32_t win, uint64_t digit, tc_result *res) {
  const Corrupt c{kind, key, win, digit};
  return build_audit(kw, n_keys, kxy, kstatus, 1, &c, 0, nullptr, nullptr, nullptr, res);
}

// The generator table of a live context (read only).  kxy: G's 16 words.
int tc_audit_ctx_g(bv_ctx *ctx, const uint32_t *kxy, uint32_t n_gather, const uint64_t *gslot, uint32_t *gout,
                   tc_result *res) {
  memset(res, 0, sizeof *res);
  tc_geom g;
  if (!ctx || !ctx->g_table || !geom_of(0, g)) return fail(res, "no generator table", hipSuccess);
  TC_CK(hipSetDevice(ctx->device), "device");
  TC_CK(hipDeviceSynchronize(), "sync");
  const uint64_t tab = (uint64_t)(uintptr_t)ctx->g_table;
  int rc = audit(nullptr, g, 1, &tab, kxy, nullptr, res);
  if (rc) return rc;
  const std::vector<uint32_t> gkey(n_gather, 0);
  return n_gather ? gather(g, 1, &tab, n_gather, gkey.data(), gslot, gout, res) : 0;
}

// The cached tables of a live key-cache context (read only), after
// bv_kc_register and bv_sync.  Keys as the context got them (key_bytes,
// key_off); kxy: their decoded points.  A key without a table is an error.
int tc_audit_ctx_kc(bv_ctx *ctx, uint32_t n_keys, const uint8_t *key_bytes, const uint64_t *key_off,
                    const uint32_t *kxy, uint32_t n_gather, const uint32_t *gkey, const uint64_t *gslot,
                    uint32_t *gout, tc_result *res) {
  memset(res, 0, sizeof *res);
  tc_geom g;
  if (!ctx || !n_keys || !geom_of(ctx->kc_w, g) || !BV_W_IS_CACHED(ctx->kc_w)) return fail(res, "no key cache", hipSuccess);
  std::vector<uint64_t> tabs(n_keys);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->kc_table_bytes != tc_table_u32(g) * 4) return fail(res, "cached table size", hipSuccess);
    for (uint32_t k = 0; k < n_keys; k++) {
      const auto it = ctx->kc_index.find(std::string((const char *)key_bytes + key_off[k], key_off[k + 1] - key_off[k]));
      if (it == ctx->kc_index.end() || !ctx->kc_slots[it->second].table) {
        snprintf(res->err, sizeof res->err, "key %u has no cached table", k);
        return -2;
      }
      tabs[k] = (uint64_t)(uintptr_t)ctx->kc_slots[it->second].table;
    }
  }
  TC_CK(hipSetDevice(ctx->device), "device");
  TC_CK(hipDeviceSynchronize(), "sync");
  int rc = audit(nullptr, g, n_keys, tabs.data(), kxy, nullptr, res);
  if (rc) return rc;
  return n_gather ? gather(g, n_keys, tabs.data(), n_gather, gkey, gslot, gout, res) : 0;
}

}  // extern "C"
