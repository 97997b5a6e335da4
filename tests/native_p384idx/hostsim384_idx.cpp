// TEST-ONLY: the P-384 host harness (tests/native/hostsim384.cpp, included
// whole) plus the entries for index-keyed passes (In384::key_idx:
// bh_verify384_compact, bh_batch_verify384_ptrs): the per-key import
// keys384_prep feeding stage384_prep's gather, the grouping by key index of a
// BH_F_BATCH_KEYS pass with its comb route against the ladder, and pack.h's
// packer at key width 96. The atomic additions of the kernels are plain
// additions here. libhostsim384i.so is built from this translation unit; the
// sanitizer program idx384_selftest compiles it with IDX384_SELFTEST_MAIN.
#include "../native/hostsim384.cpp"

#include "../../bdls_amd/csrc/comb384.h"
#include "../../bdls_amd/csrc/pack.h"

namespace {

// Keys384 in host memory, every array exactly its size.
struct KeyMem {
  std::vector<uint32_t> qx, qy, slot;
  std::vector<uint8_t> st;
  Keys384 kt{};
  explicit KeyMem(uint32_t nk) {
    const uint32_t nks = std::max(64u, (nk + 63) & ~63u);
    qx.assign((size_t)14 * nks, 0);
    qy.assign((size_t)14 * nks, 0);
    slot.assign(nk, 0);
    st.assign(nk, 0xff);
    kt.nk = nk;
    kt.nks = nks;
    kt.qx = qx.data();
    kt.qy = qy.data();
    kt.st = st.data();
    kt.slot = slot.data();
  }
};

// Comb384 for an index-keyed pass of n records over nk keys (bdls_hip.cpp
// comb384_hc: the buckets also hold every key index).
struct IdxCombMem {
  std::vector<uint32_t> mem;
  Comb384 cb{};
  IdxCombMem(uint32_t n, uint32_t nk, uint32_t min) {
    const uint32_t ns = std::max(64u, (n + 63) & ~63u);
    uint32_t hc = 128;
    while (hc < 2 * ns || hc < nk) hc <<= 1;
    const uint32_t cap = std::max(1u, ns / min);
    mem.assign(2 + (size_t)3 * hc + (size_t)2 * ns + cap +
                   (size_t)cap * (kComb384BaseWords + 2 * kComb384Words), 0);
    uint32_t* p = mem.data();
    auto take = [&](size_t words) {
      uint32_t* q = p;
      p += words;
      return q;
    };
    cb.hc = hc;
    cb.cap = cap;
    cb.min = min;
    cb.ctr = take(2);
    cb.rep = take(hc);
    cb.cnt = take(hc);
    cb.gslot = take(hc);
    cb.bkt = take(ns);
    cb.list = take(ns);
    cb.slot_rep = take(cap);
    cb.bases = take((size_t)cap * kComb384BaseWords);
    cb.side = take((size_t)cap * kComb384Words);
    cb.tables = take((size_t)cap * kComb384Words);
  }
};

const uint32_t* gcomb_idx() {
  static std::vector<uint32_t> g;
  static std::once_flag once;
  std::call_once(once, [] {
    g.assign(kComb384Words, 0);
    std::vector<uint32_t> bases(kComb384BaseWords), side(kComb384Words);
    uint32_t gx[14], gy[14];
    f384_const(gx, Cv_p384::gx_m);
    f384_const(gy, Cv_p384::gy_m);
    comb384_bases(gx, gy, bases.data());
    comb384_rows(bases.data(), side.data(), g.data());
  });
  return g.data();
}

// Words per record hs384i_prep hands back: e 12, r 12, sm 14, qx 14, qy 14, rm 14, r2m 14.
constexpr uint32_t kPrepWords = 12 + 12 + 14 * 5;

void dump_prep(const Work384& w, uint32_t n, uint8_t* st, uint32_t* words) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t* o = words + (size_t)i * kPrepWords;
    st[i] = w.st[i];
    ldw<12>(o, w.e, i, w.ns);
    ldw<12>(o + 12, w.r, i, w.ns);
    ldw<14>(o + 24, w.sm, i, w.ns);
    ldw<14>(o + 38, w.qx, i, w.ns);
    ldw<14>(o + 52, w.qy, i, w.ns);
    ldw<14>(o + 66, w.rm, i, w.ns);
    ldw<14>(o + 80, w.r2m, i, w.ns);
  }
}

struct SrcPtrs96 {  // bdls_hip.cpp SrcPtrs384
  const uint8_t* const* pub;
  const uint8_t* const* sg;
  const uint32_t* sl;
  const uint8_t* const* mg;
  const uint32_t* ml;
  const uint8_t* zero;
  const uint8_t* key(size_t i) const { return pub[i] ? pub[i] : zero; }
  const uint8_t* sig(size_t i) const { return sg[i]; }
  uint32_t sig_len(size_t i) const { return sg[i] ? sl[i] : 0u; }
  const uint8_t* msg(size_t i) const { return mg[i]; }
  uint32_t msg_len(size_t i) const { return mg[i] ? ml[i] : 0u; }
};

}  // namespace

extern "C" {

uint32_t hs384i_prep_words() { return kPrepWords; }

// stage384_prep over n records. key_idx != NULL: keys holds nk distinct keys,
// keys384_prep runs once per key (kst: its verdicts) and the records gather;
// key_idx == NULL: keys holds one key per record (the expanded layout).
// st: the status bytes (reason | ST384_R2OK); words: kPrepWords per record.
void hs384i_prep(const uint8_t* keys, uint32_t nk, const uint32_t* key_idx, const uint8_t* sig,
                 const uint64_t* so, const uint32_t* sl, const uint8_t* msg, const uint64_t* mo,
                 const uint32_t* ml, uint32_t n, uint32_t flags, uint8_t* st, uint32_t* words,
                 uint8_t* kst) {
  WorkMem m(n);
  In384 in{keys, sig, so, sl, msg, mo, ml, flags};
  KeyMem km(key_idx ? nk : 1);
  if (key_idx) {
    const KeyReg384 none{};
    par_for(nk, [&](uint32_t j) { keys384_prep(keys, km.kt, none, j); });
    if (kst) std::memcpy(kst, km.st.data(), nk);
    in.key_idx = key_idx;
    in.kt = km.kt;
  }
  par_for(n, [&](uint32_t i) { stage384_prep(in, m.w, i); });
  dump_prep(m.w, n, st, words);
}

// An index-keyed BH_F_BATCH_KEYS pass over n records: keys384_prep, prep,
// inverse, k384_comb_group_idx / _assign_idx / _plan record after record, the
// comb build from the key workspace, then the comb route and the ladder.
// cnt[nk]: records counted per key index; route[n]: 0 ladder, 1 comb;
// reason[n]: the pass's verdicts; ladder[n]: the plain ladder's for the same
// records (every record, whatever its route). Returns the combs built.
uint32_t hs384i_comb_pass(const uint8_t* keys, uint32_t nk, const uint32_t* key_idx,
                          const uint8_t* sig, const uint64_t* so, const uint32_t* sl,
                          const uint8_t* msg, const uint64_t* mo, const uint32_t* ml, uint32_t n,
                          uint32_t flags, uint32_t min, uint32_t* cnt, uint8_t* route,
                          uint8_t* reason, uint8_t* ladder) {
  WorkMem m(n);
  KeyMem km(nk);
  IdxCombMem cm(n, nk, min);
  Comb384& cb = cm.cb;
  const KeyReg384 none{};
  par_for(nk, [&](uint32_t j) { keys384_prep(keys, km.kt, none, j); });
  In384 in{keys, sig, so, sl, msg, mo, ml, flags};
  in.key_idx = key_idx;
  in.kt = km.kt;
  par_for(n, [&](uint32_t i) { stage384_prep(in, m.w, i); });
  const uint32_t stride = (n + 15) / 16;
  par_for(stride, [&](uint32_t c) { stage384_inv(m.w, c, stride, n); });
  for (uint32_t i = 0; i < n; i++) {  // k384_comb_group_idx
    uint32_t b = kNoSlot384;
    if ((m.w.st[i] & 0x7fu) == R_OK) {
      b = key_idx[i];
      cb.cnt[b]++;
    }
    cb.bkt[i] = b;
  }
  for (uint32_t j = 0; j < nk; j++) {  // k384_comb_assign_idx
    uint32_t r = comb384_index_route(km.kt, cb, j);
    if (r == 0) {
      r = cb.ctr[0]++;
      if (r < cb.cap) cb.slot_rep[r] = j;
      else r = kNoSlot384;
    }
    cb.gslot[j] = r;
  }
  std::vector<uint32_t> slot(n, kNoSlot384);
  for (uint32_t i = 0; i < n; i++) route[i] = (uint8_t)comb384_record_route(cb, i, &slot[i]);
  std::memcpy(cnt, cb.cnt, (size_t)nk * 4);
  const uint32_t nt = std::min(cb.ctr[0], cb.cap);
  par_for(nt, [&](uint32_t t) {  // k384_comb_bases_idx, k384_comb_rows
    const uint32_t j = cb.slot_rep[t];
    uint32_t qx[14], qy[14];
    ldw<14>(qx, km.kt.qx, j, km.kt.nks);
    ldw<14>(qy, km.kt.qy, j, km.kt.nks);
    comb384_bases(qx, qy, cb.bases + (size_t)t * kComb384BaseWords);
    comb384_rows(cb.bases + (size_t)t * kComb384BaseWords, cb.side + (size_t)t * kComb384Words,
                 cb.tables + (size_t)t * kComb384Words);
  });
  const uint32_t* gt = gtab();
  const uint32_t* gc = gcomb_idx();
  par_for(n, [&](uint32_t i) {
    const uint8_t st = m.w.st[i] & 0x7fu;
    if (route[i] == 1)
      reason[i] = stage384_comb(m.w, cb.tables + (size_t)slot[i] * kComb384Words, gc, i)
                      ? (uint8_t)R_OK : (uint8_t)R_MATH;
    ladder[i] = st != R_OK ? st : (stage384_ladder(m.w, gt, i) ? (uint8_t)R_OK : (uint8_t)R_MATH);
    if (route[i] != 1) reason[i] = ladder[i];
  });
  return nt;
}

// pack.h at key width 96 over per-record pointers (NULL: as bh_pbatch says).
// keys: n * 96 bytes; sig / msg: the sums of the lengths. Returns the keys
// packed (holes of the claim blocks included), -1 if de-duplication was dropped.
int hs384i_pack(const uint8_t* const* pub, const uint8_t* const* sg, const uint32_t* sl,
                const uint8_t* const* mg, const uint32_t* ml, uint32_t n, int threads,
                uint8_t* keys, uint32_t* key_idx, uint32_t* slen, uint32_t* mlen, uint8_t* sig,
                uint8_t* msg) {
  static const uint8_t zero[96] = {0};
  bh::pack::PackerT<96> P(threads);
  const SrcPtrs96 src{pub, sg, sl, mg, ml, zero};
  bh::pack::Out out{keys, key_idx, slen, mlen};
  bh::pack::Result r;
  P.plan(src, 0, n, &r, 1);
  P.fill(src, out, sig, msg, &r, nullptr);
  if (r.dedup_dropped || !r.dedup) return -1;
  return (int)r.nkeys;
}

}  // extern "C"

#ifdef IDX384_SELFTEST_MAIN
// Stand-alone sanitizer run (-fsanitize=address,undefined): 130 records over a
// shuffled key table with duplicate, unused, off-curve and out-of-range
// entries, libcrypto-signed; index-keyed prep against expanded prep word for
// word, and the index-grouped comb pass against the ladder. Every buffer is a
// heap allocation of exactly its size.
#define OPENSSL_SUPPRESS_DEPRECATED
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>

#include <cstdio>

int main() {
  const uint32_t n = 130, nreal = 9;
  const uint32_t uses[nreal] = {1, 3, 4, 5, 60, 20, 20, 10, 7};  // 130
  std::vector<EC_KEY*> ek;
  std::vector<std::vector<uint8_t>> table;  // the key table
  for (uint32_t k = 0; k < nreal; k++) {
    EC_KEY* key = EC_KEY_new_by_curve_name(NID_secp384r1);
    if (!key || EC_KEY_generate_key(key) != 1) abort();
    BIGNUM *x = BN_new(), *y = BN_new();
    if (EC_POINT_get_affine_coordinates(EC_KEY_get0_group(key), EC_KEY_get0_public_key(key), x, y,
                                        nullptr) != 1)
      abort();
    std::vector<uint8_t> pub(96);
    BN_bn2binpad(x, pub.data(), 48);
    BN_bn2binpad(y, pub.data() + 48, 48);
    BN_free(x);
    BN_free(y);
    ek.push_back(key);
    table.push_back(pub);
  }
  // entries 9..12: a duplicate of key 4 (used by half of its records), an unused
  // off-curve key, an unused key with X >= p, a used off-curve key
  table.push_back(table[4]);
  std::vector<uint8_t> off = table[0];
  off[95] ^= 1;
  table.push_back(off);
  table.push_back(std::vector<uint8_t>(96, 0xff));
  off = table[1];
  off[60] ^= 4;
  table.push_back(off);
  const uint32_t nk = (uint32_t)table.size();
  std::vector<uint8_t> keys((size_t)nk * 96), pub((size_t)n * 96), sig, msg((size_t)n * 48);
  for (uint32_t j = 0; j < nk; j++) memcpy(&keys[(size_t)j * 96], table[j].data(), 96);
  std::vector<uint32_t> kidx(n), sl(n), ml(n);
  std::vector<uint64_t> so(n), mo(n);
  uint32_t i = 0;
  for (uint32_t k = 0; k < nreal; k++)
    for (uint32_t u = 0; u < uses[k]; u++, i++) kidx[i] = (k == 4 && (u & 1)) ? 9 : k;
  for (i = 0; i < n; i++) std::swap(kidx[i], kidx[(i * 37 + 11) % n]);
  for (i = 0; i < n; i++) {
    const uint32_t k = kidx[i] == 9 ? 4 : kidx[i];
    for (int j = 0; j < 48; j++) msg[(size_t)i * 48 + j] = (uint8_t)(29 * i + 13 * j + 3);
    mo[i] = (uint64_t)i * 48;
    ml[i] = 48;
    uint8_t der[128];
    unsigned int dl = 0;
    if (ECDSA_sign(0, &msg[(size_t)i * 48], 48, der, &dl, ek[k]) != 1) abort();
    if (i % 16 == 5) kidx[i] = 12;             // off-curve key: BH_R_BAD_KEY unless rejected earlier
    if (i % 32 == 7) dl = 0;                   // BH_R_EMPTY_SIG
    if (i % 32 == 9) msg[(size_t)i * 48] ^= 1;  // BH_R_MATH
    so[i] = sig.size();
    sl[i] = dl;
    sig.insert(sig.end(), der, der + dl);
    memcpy(&pub[(size_t)i * 96], &keys[(size_t)kidx[i] * 96], 96);
  }
  if (sig.empty()) sig.push_back(0);
  int bad = 0;
  for (uint32_t flags : {0u, 2u}) {
    const uint32_t pw = hs384i_prep_words();
    std::vector<uint8_t> st_a(n), st_b(n), kst(nk);
    std::vector<uint32_t> wa((size_t)n * pw), wb((size_t)n * pw);
    hs384i_prep(keys.data(), nk, kidx.data(), sig.data(), so.data(), sl.data(), msg.data(),
                mo.data(), ml.data(), n, flags, st_a.data(), wa.data(), kst.data());
    hs384i_prep(pub.data(), n, nullptr, sig.data(), so.data(), sl.data(), msg.data(), mo.data(),
                ml.data(), n, flags, st_b.data(), wb.data(), nullptr);
    if (st_a != st_b || wa != wb) {
      fprintf(stderr, "prep differs: flags %u\n", flags);
      bad |= 1;
    }
    if (kst[10] != R_BAD_KEY || kst[11] != R_BAD_KEY || kst[12] != R_BAD_KEY || kst[0] != R_OK)
      bad |= 2;
    std::vector<uint32_t> cnt(nk);
    std::vector<uint8_t> route(n), reason(n), ladder(n);
    const uint32_t tables =
        hs384i_comb_pass(keys.data(), nk, kidx.data(), sig.data(), so.data(), sl.data(),
                         msg.data(), mo.data(), ml.data(), n, flags, 4, cnt.data(), route.data(),
                         reason.data(), ladder.data());
    std::vector<uint32_t> want(nk, 0);
    for (i = 0; i < n; i++)
      if ((st_a[i] & 0x7f) == R_OK) want[kidx[i]]++;
    uint32_t want_tables = 0;
    for (uint32_t j = 0; j < nk; j++) want_tables += want[j] >= 4;
    if (cnt != want || tables != want_tables) {
      fprintf(stderr, "counts differ: flags %u tables %u / %u\n", flags, tables, want_tables);
      bad |= 4;
    }
    for (i = 0; i < n; i++) {
      const bool comb = (st_a[i] & 0x7f) == R_OK && want[kidx[i]] >= 4;
      if (route[i] != (comb ? 1 : 0) || reason[i] != ladder[i]) bad |= 8;
    }
  }
  for (EC_KEY* k : ek) EC_KEY_free(k);
  printf("idx384_selftest: %u records, %u table entries, %s\n", n, nk, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
#endif
