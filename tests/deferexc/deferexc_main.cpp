// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for BV_DEFER_EXC /
// BV_FUSED_Y3 (babble_amd/csrc/verify_core.h, point.h): the throughput verify
// loops compiled for the host from the device's own source, through the host
// emulator's table builders (tests/emu/emu.cpp, included as is).
// tests/test_defer_exc.py builds it with the knobs at 1 and at 0 (and once
// under AddressSanitizer + UBSan) and compares the outputs item for item.
//
//   deferexc batch.bin [threads [digests.bin [8|12|18|22 [slots.txt|- [gslots.txt]]]]]
//
// digests.bin (optional; tests/test_chain_exceptions.py): n_msgs x 32 bytes
// that REPLACE the messages' SHA-256 digests in the emulator's pipeline (the
// oracle column still hashes the messages: ignore it then), so that the
// valid signatures of tests/chain_vectors.py, whose digest is chosen, can be
// replayed.  8 | 12: the per-batch key-table geometry (K8's unsigned windows
// or K12; default 12).  18 | 22: the key cache's chain instead
// (verify_item_gq_kc) over the sparse cached tables of slots.txt: run_cached,
// which also runs the host entries' order over them (verify_item_qfirst<W>,
// verify_item_gfinish) and fills st_host, redo_qf and redo_gf.  gslots.txt: the
// generator table is a sparse one too (sparse_g_table) instead of the
// emulator's, for a build with the product's generator geometry, whose full
// table no host holds (slots.txt is "-" for 8 | 12, which build their own key
// tables).
//
// batch.bin: tests/emu/emu.py dump_batch ("BVB1").  Per item, one line:
//   i oracle st_dev st_host redo_g redo_q redo_qf redo_gf  R_G  R_Q
// st_dev: verify_item_g then verify_item_q<K12> (the device entry's order);
// st_host: verify_item_qfirst<K12> then verify_item_gfinish (the host
// entries' order); redo_*: whether that call took the redo branch; R_G / R_Q:
// the stored partial sums (X Y ZZ ZZZ canonical hex, identity flag).
// Before the items, "unit <n>": n unchecked additions (general, trimmed and
// affine forms) on accumulators equal to +-the entry (ZZ3 must be 0 mod p)
// and on other entries (ZZ3 != 0, the same group element as the checked
// form); any failure exits 1.
#include <sys/mman.h>

#include <cstdio>

#include "../emu/emu.cpp"

extern "C" {
int oracle_verify_batch(const bv_batch *b, uint8_t *msg_hash, uint8_t *status, uint64_t *accept_bits, int n_threads);
void oracle_init(void);
}

namespace {

template <class T>
bool rd(FILE *f, std::vector<T> &v, uint64_t n) {
  v.resize(n ? n : 1);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

void put_fe(fe a) {
  fe_canon(a);
  for (int i = 7; i >= 0; i--) printf("%08x", a.v[i]);
  putchar(' ');
}

void put_acc(const uint32_t *buf, uint64_t n, uint64_t i) {
  gexz R;
  bool inf;
  rg_load(buf, n, i, R, inf);
  put_fe(R.X), put_fe(R.Y), put_fe(R.ZZ), put_fe(R.ZZZ);
  printf("%d ", buf[(uint64_t)32 * n + i] ? 1 : 0);
}

bool same_point(const gexz &a, const gexz &b) {  // both finite
  fe l, r;
  fe_mul(l, a.X, b.ZZ), fe_mul(r, b.X, a.ZZ);
  if (!fe_eq(l, r)) return false;
  fe_mul(l, a.Y, b.ZZZ), fe_mul(r, b.Y, a.ZZZ);
  return fe_eq(l, r);
}

// acc = (x, y) scaled by z (z = 1: affine)
gexz scaled(const fe &x, const fe &y, const fe &z) {
  gexz a;
  fe z2, z3;
  fe_sqr(z2, z);
  fe_mul(z3, z2, z);
  fe_mul(a.X, x, z2);
  fe_mul(a.Y, y, z3);
  a.ZZ = z2;
  a.ZZZ = z3;
  return a;
}

// the unchecked additions on table entries e (x, y at 16 words each)
int unit(const uint32_t *tab, uint32_t n_ent) {
  int n = 0;
  fe one;
  fe_set(one, 1);
  for (uint32_t t = 1; t + 2 < n_ent; t += 97) {
    fe x, y, ny, fx, fy, z;
    fe_load(x, tab + 16 * t), fe_load(y, tab + 16 * t + 8);
    fe_load(fx, tab + 16 * (t + 1)), fe_load(fy, tab + 16 * (t + 1) + 8);
    fe_load(z, tab + 16 * (t + 2));
    fe_neg(ny, y);
    for (int form = 0; form < 3; form++) {  // general, trimmed (xz_only), affine
      const gexz a0 = scaled(x, y, form == 2 ? one : z);
      const fe *ys[3] = {&y, &ny, &fy};
      for (int c = 0; c < 3; c++) {  // acc == entry, acc == -entry, another entry
        const fe &ex = c == 2 ? fx : x;
        gexz u = a0, k = a0;
        bool ui = false, ki = false;
        if (form == 2) {
          gexz_add_ge_aff<false, false>(u, ui, ex, *ys[c]);
          gexz_add_ge_aff<false, true>(k, ki, ex, *ys[c]);
        } else {
          gexz_add_ge<false>(u, ui, ex, *ys[c], form == 1, false);
          gexz_add_ge<true>(k, ki, ex, *ys[c], false);
        }
        n++;
        if (ui) return -n;  // the unchecked form never sets the flag
        if (c < 2) {
          if (!fe_is_zero(u.ZZ) || !defer_flagged(u, ui)) return -n;
          if (ki != (c == 1)) return -n;  // checked: a doubling stays finite, P + (-P) is the identity
        } else {
          if (fe_is_zero(u.ZZ) || ki) return -n;
          if (form == 1) {  // only X and ZZ are formed
            fe l, r;
            fe_mul(l, u.X, k.ZZ), fe_mul(r, k.X, u.ZZ);
            if (!fe_eq(l, r)) return -n;
          } else if (!same_point(u, k)) {
            return -n;
          }
        }
      }
    }
  }
  return n;
}

// The key cache's one-pass chain (verify_item_gq_kc<22, 6> or <18, 8>) over
// SPARSE cached tables: each key's table is an allocation of the geometry's
// full size, zero pages except the slots listed in `slots_path` (one line per
// entry: <key> <slot> <x, 64 hex> <y, 64 hex>; tests/kcsmall's form), which the
// test computes for the digits its items read.  A zero digit reads a slot that
// is then not added.  Per item: i oracle st st_host 0 redo redo_qf redo_gf.
fe fe_hex(const char *h) {
  fe a;
  for (int i = 0; i < 8; i++) {
    char w[9] = {0};
    memcpy(w, h + 8 * i, 8);
    a.v[7 - i] = (uint32_t)strtoul(w, nullptr, 16);
  }
  return a;
}

// The GENERATOR table of the geometry this program was built with, SPARSE in
// the same way (a build with the product's 26 x 10 windows: 21.5 GB of address
// space, no page touched except the listed slots): one line per entry,
// <slot> <x, 64 hex> <y, 64 hex>, slot j 2^(BV_GW-1) + |d| holding
// |d| 2^(BV_GW j) G, which the test computes for the digits of its items' u1.
const uint32_t *sparse_g_table(const char *path) {
  const size_t bytes = BV_GTABLE_U32 * 4 + 64;
  void *p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  FILE *f = fopen(path, "r");
  if (p == MAP_FAILED || !f) return nullptr;
  uint32_t *tab = (uint32_t *)p;
  unsigned long long slot;
  char hx[80], hy[80];
  while (fscanf(f, "%llu %79s %79s", &slot, hx, hy) == 3) {
    if (slot > (uint64_t)BV_GNWIN * BV_GENT || strlen(hx) != 64 || strlen(hy) != 64) return nullptr;
    const fe x = fe_hex(hx), y = fe_hex(hy);
    memcpy(tab + slot * BV_ENTRY_U32, x.v, 32);
    memcpy(tab + slot * BV_ENTRY_U32 + 8, y.v, 32);
  }
  fclose(f);
  return tab;
}

template <int W, int NWIN>
int run_cached_geom(const char *slots_path, const uint32_t *gt, const bv_batch &b, const uint8_t *kst,
                    const uint32_t *r, const uint32_t *s, const uint32_t *dig, const std::vector<uint8_t> &st0,
                    int nt) {
  constexpr uint64_t SLOTS = (uint64_t)NWIN * (1ull << (W - 1)) + 1;
  const uint64_t n = b.n_items;
  std::vector<uint32_t *> tabs(b.n_keys ? b.n_keys : 1, nullptr);
  std::vector<uint64_t> addr(tabs.size(), 0);
  for (uint32_t k = 0; k < b.n_keys; k++) {
    tabs[k] = (uint32_t *)calloc(SLOTS * BV_ENTRY_U32, 4);  // untouched pages stay unbacked
    if (!tabs[k]) return 2;
    addr[k] = (uint64_t)(uintptr_t)tabs[k];
  }
  FILE *f = slots_path ? fopen(slots_path, "r") : nullptr;
  if (!f) return 2;
  unsigned key;
  unsigned long long slot;
  char hx[80], hy[80];
  while (fscanf(f, "%u %llu %79s %79s", &key, &slot, hx, hy) == 4) {
    if (key >= b.n_keys || slot >= SLOTS || strlen(hx) != 64 || strlen(hy) != 64) return 2;
    const fe x = fe_hex(hx), y = fe_hex(hy);
    memcpy(tabs[key] + slot * BV_ENTRY_U32, x.v, 32);
    memcpy(tabs[key] + slot * BV_ENTRY_U32 + 8, y.v, 32);
  }
  fclose(f);
  std::vector<uint8_t> s_scr;
  uint32_t *w = aligned<uint32_t>(s_scr, n * 32 + 32);
  const uint32_t M = 16;
  const uint64_t T = ((n + M - 1) / M + 255) / 256 * 256;
  parallel_for(T, nt, [&](uint64_t t) { sinv_thread(t, T, n, M, s, b.pre, w); });
  if (!gt) gt = emu_g_table(nt);
  std::vector<uint8_t> s_rq;
  uint32_t *rq = aligned<uint32_t>(s_rq, (n + 1) * RG_WORDS * 4);
  printf("unit 0\n");
  uint64_t &cnt = bv_defer_redo_count();
  for (uint64_t i = 0; i < n; i++) {
    uint64_t c = cnt;
    const uint8_t st = verify_item_gq_kc<W, NWIN>(i, b.item_key, r, s, b.pre, kst, b.item_msg, dig, w, gt, addr.data());
    const int fq = cnt != c;
    // the host entries' order over the same tables (k_verify_qf<W>, k_verify_gf)
    c = cnt;
    verify_item_qfirst<W, NWIN>(i, n, b.item_key, r, s, b.pre, kst, w, nullptr, addr.data(), rq);
    const int fqf = cnt != c;
    c = cnt;
    const uint8_t st6 = verify_item_gfinish(i, n, b.item_key, r, s, b.pre, kst, b.item_msg, dig, w, gt, rq);
    const int fgf = cnt != c;
    printf("%llu %d %d %d 0 %d %d %d\n", (unsigned long long)i, st0[i], st, st6, fq, fqf, fgf);
  }
  for (uint32_t *t : tabs) free(t);
  return 0;
}

int run_cached(int kw, const char *slots_path, const uint32_t *gt, const bv_batch &b, const uint8_t *kst,
               const uint32_t *r, const uint32_t *s, const uint32_t *dig, const std::vector<uint8_t> &st0, int nt) {
  return kw == BV_KCW ? run_cached_geom<BV_KCW, BV_KCNWIN>(slots_path, gt, b, kst, r, s, dig, st0, nt)
                      : run_cached_geom<BV_KC18W, BV_KC18NWIN>(slots_path, gt, b, kst, r, s, dig, st0, nt);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const int nt = argc > 2 ? atoi(argv[2]) : 4;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  char magic[4];
  uint64_t hdr[6];
  if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "BVB1", 4) != 0 || fread(hdr, 8, 6, f) != 6) return 2;
  const uint64_t n_msgs = hdr[0], n_keys = hdr[1], n = hdr[2], msg_len = hdr[3], key_len = hdr[4];
  std::vector<uint64_t> msg_off, key_off;
  std::vector<uint8_t> msgv, key, rb, sb, pre;
  std::vector<uint32_t> im, ik;
  const bool ok = rd(f, msg_off, n_msgs + 1) && rd(f, msgv, msg_len) && rd(f, key_off, n_keys + 1) &&
                  rd(f, key, key_len) && rd(f, im, n) && rd(f, ik, n) && rd(f, rb, 32 * n) && rd(f, sb, 32 * n) &&
                  (!hdr[5] || rd(f, pre, n));
  fclose(f);
  if (!ok) return 2;
  bv_batch b{};
  b.n_msgs = n_msgs, b.msg_bytes = msgv.data(), b.msg_off = msg_off.data();
  b.n_keys = (uint32_t)n_keys, b.key_bytes = key.data(), b.key_off = key_off.data();
  b.n_items = n, b.item_msg = im.data(), b.item_key = ik.data(), b.r_be = rb.data(), b.s_be = sb.data();
  b.pre = hdr[5] ? pre.data() : nullptr;

  std::vector<uint8_t> h0(32 * n_msgs + 1), st0(n + 1);
  std::vector<uint64_t> b0((n + 63) / 64 + 1);
  oracle_init();
  oracle_verify_batch(&b, h0.data(), st0.data(), b0.data(), nt);

  // the emulator's pipeline (emu_verify_batch, K12 tables), item by item
  std::vector<uint8_t> s_msg, s_dig, s_kst, s_kxy, s_r, s_s, s_scr, s_u12, s_kt, s_rg, s_rq;
  uint8_t *msg = aligned<uint8_t>(s_msg, msg_len + 64);
  if (msg_len) memcpy(msg, b.msg_bytes, msg_len);
  uint32_t *dig = aligned<uint32_t>(s_dig, (n_msgs + 1) * 32);
  uint8_t *kst = aligned<uint8_t>(s_kst, n_keys + 1);
  uint32_t *kxy = aligned<uint32_t>(s_kxy, (n_keys + 1) * 64ull);
  uint32_t *r = aligned<uint32_t>(s_r, n * 32 + 32);
  uint32_t *s = aligned<uint32_t>(s_s, n * 32 + 32);
  memcpy(r, b.r_be, n * 32);
  memcpy(s, b.s_be, n * 32);
  uint32_t *w = aligned<uint32_t>(s_scr, n * 32 + 32);
  uint32_t *u12 = aligned<uint32_t>(s_u12, n * BV_U_STRIDE * 4 + 64);
  parallel_for(n_msgs, nt, [&](uint64_t m) { sha256_one(m, msg, b.msg_off, dig); });
  for (uint32_t k = 0; k < n_keys; k++) key_decode_one(k, b.key_bytes, b.key_off, kst, kxy);
  if (argc > 3) {  // digests-in mode
    FILE *df = fopen(argv[3], "rb");
    if (!df) return 2;
    const bool got = n_msgs == 0 || fread(dig, 32, n_msgs, df) == n_msgs;
    fclose(df);
    if (!got) return 2;
  }
  const int kw = argc > 4 ? atoi(argv[4]) : 12;
  const uint32_t *gt = argc > 6 ? sparse_g_table(argv[6]) : nullptr;
  if (argc > 6 && !gt) return 2;
  if (kw == BV_KCW || kw == BV_KC18W)
    return run_cached(kw, argc > 5 ? argv[5] : nullptr, gt, b, kst, r, s, dig, st0, nt);
  if (kw != 8 && kw != 12) return 2;
  if (!gt) gt = emu_g_table(nt);
  uint32_t *kt = aligned<uint32_t>(
      s_kt, (uint64_t)(n_keys ? n_keys : 1) * (kw == 12 ? (uint64_t)BV_K12TABLE_U32 : (uint64_t)BV_KTABLE_U32) * 4);
  emu_build_tables(kw, (uint32_t)n_keys, kxy, kst, kt, nt);
  uint32_t *rg = aligned<uint32_t>(s_rg, (n + 1) * RG_WORDS * 4);
  uint32_t *rq = aligned<uint32_t>(s_rq, (n + 1) * RG_WORDS * 4);
  const uint32_t M = 16;
  const uint64_t T = ((n + M - 1) / M + 255) / 256 * 256;
  parallel_for(T, nt, [&](uint64_t t) { sinv_thread(t, T, n, M, s, b.pre, w); });

  const int nu = unit(kt, 2048);
  if (nu <= 0) {
    fprintf(stderr, "unit case %d failed\n", -nu);
    return 1;
  }
  printf("unit %d\n", nu);

  uint64_t &cnt = bv_defer_redo_count();
  for (uint64_t i = 0; i < n; i++) {
    uint64_t c = cnt;
    verify_item_g(i, n, b.item_key, r, s, b.pre, kst, b.item_msg, dig, w, u12, gt, rg);
    const int fg = cnt != c;
    c = cnt;
    const uint8_t st2 =
        kw == 12 ? verify_item_q<BV_K12W, BV_K12NWIN>(i, n, b.item_key, r, s, b.pre, kst, u12, kt, nullptr, rg)
                 : verify_item_q<BV_KW, BV_KNWIN>(i, n, b.item_key, r, s, b.pre, kst, u12, kt, nullptr, rg);
    const int fq = cnt != c;
    c = cnt;
    if (kw == 12) verify_item_qfirst<BV_K12W, BV_K12NWIN>(i, n, b.item_key, r, s, b.pre, kst, w, kt, nullptr, rq);
    else verify_item_qfirst<BV_KW, BV_KNWIN>(i, n, b.item_key, r, s, b.pre, kst, w, kt, nullptr, rq);
    const int fqf = cnt != c;
    c = cnt;
    const uint8_t st6 = verify_item_gfinish(i, n, b.item_key, r, s, b.pre, kst, b.item_msg, dig, w, gt, rq);
    const int fgf = cnt != c;
    printf("%llu %d %d %d %d %d %d %d ", (unsigned long long)i, st0[i], st2, st6, fg, fq, fqf, fgf);
    put_acc(rg, n, i);
    put_acc(rq, n, i);
    putchar('\n');
  }
  return 0;
}
