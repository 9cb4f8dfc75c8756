// Stand-alone host driver (TEST INFRASTRUCTURE ONLY) for BV_Y_ALT
// (babble_amd/csrc/point.h, verify_core.h): the throughput verify loops
// compiled for the host from the device's own source, through the host
// emulator's table builders (tests/emu/emu.cpp, included as is).
// tests/test_y_alt.py builds it with the knob at 1 and at 0 (and once under
// AddressSanitizer + UBSan) and compares the outputs item for item.
//
//   yalt batch.bin [threads]
//
// batch.bin: tests/emu/emu.py dump_batch ("BVB1").  Per item, one line:
//   i oracle st_dev st_host skip set dbl opp  R_G  R_Q
// st_dev: verify_item_g then verify_item_q<K12> (the device entry's order);
// st_host: verify_item_qfirst<K12> then verify_item_gfinish (the host
// entries' order); skip / set / dbl / opp: how often the item's four calls
// entered the rare paths of the addition steps (a lane that adds nothing, the
// identity taking an entry, P + P, P + (-P): point.h bv_step_count); R_G /
// R_Q: the stored partial sums (X Y ZZ ZZZ canonical hex, identity flag).
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
  const uint32_t *gt = emu_g_table(nt);
  uint32_t *kt = aligned<uint32_t>(s_kt, (uint64_t)(n_keys ? n_keys : 1) * BV_K12TABLE_U32 * 4);
  emu_build_tables(12, (uint32_t)n_keys, kxy, kst, kt, nt);
  uint32_t *rg = aligned<uint32_t>(s_rg, (n + 1) * RG_WORDS * 4);
  uint32_t *rq = aligned<uint32_t>(s_rq, (n + 1) * RG_WORDS * 4);
  const uint32_t M = 16;
  const uint64_t T = ((n + M - 1) / M + 255) / 256 * 256;
  parallel_for(T, nt, [&](uint64_t t) { sinv_thread(t, T, n, M, s, b.pre, w); });

  printf("knob %d\n", (int)(y_alt(false, 1) && y_alt(false, 2)));
  bv_step_counts &cnt = bv_step_count();
  for (uint64_t i = 0; i < n; i++) {
    const bv_step_counts c = cnt;
    verify_item_g(i, n, b.item_key, r, s, b.pre, kst, b.item_msg, dig, w, u12, gt, rg);
    const uint8_t st2 = verify_item_q<BV_K12W, BV_K12NWIN>(i, n, b.item_key, r, s, b.pre, kst, u12, kt, nullptr, rg);
    verify_item_qfirst<BV_K12W, BV_K12NWIN>(i, n, b.item_key, r, s, b.pre, kst, w, kt, nullptr, rq);
    const uint8_t st6 = verify_item_gfinish(i, n, b.item_key, r, s, b.pre, kst, b.item_msg, dig, w, gt, rq);
    printf("%llu %d %d %d %llu %llu %llu %llu ", (unsigned long long)i, st0[i], st2, st6,
           (unsigned long long)(cnt.skip - c.skip), (unsigned long long)(cnt.set - c.set),
           (unsigned long long)(cnt.dbl - c.dbl), (unsigned long long)(cnt.opp - c.opp));
    put_acc(rg, n, i);
    put_acc(rq, n, i);
    putchar('\n');
  }
  return 0;
}
