// Key registry of BH_CURVE_P384 (bh_keys384_*): per registered key a
// fixed-base table of the same shape as the table of G, a device hash table
// from the 96 key bytes to the table, and the verify stage that walks two
// tables instead of the ladder. What msp/cache/cache.go keeps per identity and
// BDLS's Config.Participants fixes per channel, kept where the kernels are.
//
//   key table   window w (4 bits, 96 windows), digit d in 1..15 -> d 16^w Q,
//               affine Montgomery x || y (28 words) at ((w * 15) + d - 1) * 28:
//               kKTab384Words = 40,320 words = 161,280 bytes per key. Unsigned
//               digits: no carry window, no negation, and the walk of u2 is the
//               walk of u1 over another table.
//   build       keytab384_bases: one chain of 380 doublings per key, the 96
//               window bases 16^w Q kept (Jacobian); keytab384_window: per
//               window 2B..15B from the base (7 doublings, 7 additions) and one
//               inversion for its 15 entries by Montgomery's trick.
//   lookup      open addressing over buckets of slot + 1, linear probing, every
//               hit confirmed by comparing all 24 key words.
//   verify      stage384_keywin: u2 Q from the key's table, then u1 G from the
//               table of G, every step a mixed addition; the ladder's x check.
// Every function is BH_HD: tests/native_p384keys/hostsim384_keys.cpp runs the
// same code.
#pragma once
#include "verify384.h"

namespace bh {

constexpr size_t kKTab384Words = kGTab384Words;
constexpr uint32_t kNoSlot384 = 0xffffffffu;
constexpr uint32_t kBase384Words = 42;  // a window base: Jacobian x, y, z

struct KeyReg384 {
  uint32_t cap;      // tables (0 = registry not allocated)
  uint32_t hc;       // buckets (power of two >= 2 cap: the probe always ends)
  uint32_t* bucket;  // [hc] slot + 1, 0 = empty
  uint32_t* keys;    // [cap][24] the key bytes X || Y, four to a word
  uint32_t* tables;  // [cap][kKTab384Words]
  uint32_t* count;   // [1] slots handed out (<= cap)
};

// Per-pass routing (one chunk): records whose key has a table, and the rest.
struct Plan384 {
  uint32_t* slot;      // [ns] per record: its key's slot (table route only)
  uint32_t* tab_list;  // [ns] records on the table route, cnt[0] of them
  uint32_t* lad_list;  // [ns] records on the ladder, cnt[1] of them
  uint32_t* cnt;       // [2]
};

BH_HD void key384_words(const uint8_t* q, uint32_t k[24]) {
#pragma unroll
  for (int j = 0; j < 24; j++)
    k[j] = (uint32_t)q[4 * j] | ((uint32_t)q[4 * j + 1] << 8) | ((uint32_t)q[4 * j + 2] << 16) |
           ((uint32_t)q[4 * j + 3] << 24);
}

BH_HD uint32_t key384_hash(const uint32_t k[24]) {
  uint32_t h = 0x811c9dc5u;
#pragma unroll
  for (int j = 0; j < 24; j++) {
    h = (h ^ k[j]) * 0x9e3779b1u;
    h ^= h >> 15;
  }
  return h ^ (h >> 16);
}

// The slot of key k, or kNoSlot384.
BH_HD uint32_t keys384_find(const KeyReg384& g, const uint32_t k[24]) {
  uint32_t b = key384_hash(k) & (g.hc - 1);
  for (uint32_t probes = 0; probes < g.hc; probes++, b = (b + 1) & (g.hc - 1)) {
    const uint32_t v = g.bucket[b];
    if (v == 0 || v > g.cap) return kNoSlot384;
    const uint32_t* q = g.keys + (size_t)(v - 1) * 24;
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 24; j++) d |= q[j] ^ k[j];
    if (d == 0) return v - 1;
  }
  return kNoSlot384;
}

// Register keys one after another (one lane: the registry has one writer).
// status[i] comes in as 0 or R_BAD_KEY (key_import384's verdict) and leaves as
// 0 (registered or already present), R_BAD_KEY or 255 (registry full). The
// slots handed out by this call go to fresh[0, *nfresh): their tables are built next.
BH_HD void keys384_insert(const KeyReg384& g, const uint8_t* pub, uint32_t n, uint8_t* status,
                          uint32_t* fresh, uint32_t* nfresh) {
  uint32_t nf = 0;
  uint32_t c = *g.count;
  if (c > g.cap) c = g.cap;
  for (uint32_t i = 0; i < n; i++) {
    if (status[i] != 0) continue;
    uint32_t k[24];
    key384_words(pub + (size_t)i * 96, k);
    if (keys384_find(g, k) != kNoSlot384) continue;
    if (c >= g.cap) {
      status[i] = 255;
      continue;
    }
    uint32_t* q = g.keys + (size_t)c * 24;
#pragma unroll
    for (int j = 0; j < 24; j++) q[j] = k[j];
    uint32_t b = key384_hash(k) & (g.hc - 1);
    while (g.bucket[b] != 0) b = (b + 1) & (g.hc - 1);  // hc >= 2 cap > count: there is one
    g.bucket[b] = c + 1;
    fresh[nf++] = c;
    c++;
  }
  *g.count = c;
  *nfresh = nf;
}

// The chain of a key's table: bases[w] = 16^w Q (Jacobian, 42 words) for the
// 96 windows. 380 doublings, once per key.
BH_HD void keytab384_bases(const KeyReg384& g, uint32_t slot, uint32_t* bases) {
  const uint32_t* k = g.keys + (size_t)slot * 24;
  uint8_t q[96];
#pragma unroll
  for (int j = 0; j < 24; j++) {
    q[4 * j] = (uint8_t)k[j];
    q[4 * j + 1] = (uint8_t)(k[j] >> 8);
    q[4 * j + 2] = (uint8_t)(k[j] >> 16);
    q[4 * j + 3] = (uint8_t)(k[j] >> 24);
  }
  uint32_t qx[14], qy[14];
  (void)key_import384(q, qx, qy);  // a registered key is on the curve
  J384 B;
  j384_set_affine(&B, qx, qy);
#pragma unroll 1
  for (int w = 0; w < kG384Win; w++) {
    uint32_t* o = bases + (size_t)w * kBase384Words;
#pragma unroll
    for (int j = 0; j < 14; j++) {
      o[j] = B.x[j];
      o[14 + j] = B.y[j];
      o[28 + j] = B.z[j];
    }
    if (w + 1 < kG384Win) {
#pragma unroll 1
      for (int j = 0; j < 4; j++) j384_dbl(&B);
    }
  }
}

// One window of a key's table: rows[d - 1] = d B for d in 1..15, B the window's
// base. d 16^w < n, so neither d B nor a sum of two of them below 16 B meets an
// exceptional case; Q has order n (the cofactor is 1), so no entry is infinite
// and no Z is zero. One inversion for the 15 entries.
BH_HD void keytab384_window(const uint32_t* base, uint32_t* rows) {
  J384 E[kG384Ent];
#pragma unroll
  for (int j = 0; j < 14; j++) {
    E[0].x[j] = base[j];
    E[0].y[j] = base[14 + j];
    E[0].z[j] = base[28 + j];
  }
  E[0].inf = 0;
#pragma unroll 1
  for (int k = 1; k < kG384Ent; k++) {  // E[k] = (k + 1) B
    if (k & 1) {
      E[k] = E[k >> 1];
      j384_dbl(&E[k]);
    } else {
      E[k] = E[k - 1];
      j384_add(&E[k], &E[0], 0);
    }
  }
  uint32_t pre[kG384Ent][14], acc[14], inv[14];
  f384_const(acc, P384::r1);
#pragma unroll 1
  for (int k = 0; k < kG384Ent; k++) {
    f384_copy(pre[k], acc);
    f384_mul<P384>(acc, acc, E[k].z);     // 2*20 [2p]
  }
  f384_canon<P384>(acc, acc);
  f384_inv<P384>(inv, acc);               // (prod Z)^-1 [2p]
#pragma unroll 1
  for (int k = kG384Ent - 1; k >= 0; k--) {
    uint32_t zi[14], zi2[14], t[14], c[14];
    f384_mul<P384>(zi, inv, pre[k]);      // Z_k^-1 [2p]
    f384_mul<P384>(inv, inv, E[k].z);     // [2p]
    f384_sqr<P384>(zi2, zi);              // [2p]
    uint32_t* o = rows + (size_t)k * kG384Words;
    f384_mul<P384>(t, E[k].x, zi2);       // 40 [2p]
    f384_canon<P384>(c, t);
#pragma unroll
    for (int j = 0; j < 14; j++) o[j] = c[j];
    f384_mul<P384>(t, zi, zi2);           // [2p]
    f384_mul<P384>(t, E[k].y, t);         // 40 [2p]
    f384_canon<P384>(c, t);
#pragma unroll
    for (int j = 0; j < 14; j++) o[14 + j] = c[j];
  }
}

// Record i's slot in the registry, or kNoSlot384: a record that prep rejected
// stays on the ladder route, which reports its reason.
BH_HD uint32_t stage384_plan(const In384& in, const Work384& w, const KeyReg384& g, uint32_t i) {
  if ((w.st[i] & 0x7fu) != R_OK) return kNoSlot384;
  if (in.key_idx) return in.kt.slot[in.key_idx[i]];  // looked up once per key (keys384_prep)
  uint32_t k[24];
  key384_words(in384_key(in, i), k);
  return keys384_find(g, k);
}

// Key j of an index-keyed shard, once for all its records and chunks:
// key_import384's verdict and coordinates into the key workspace, and the
// key's slot in the registry (g.cap == 0: no registry, no lookup).
BH_HD void keys384_prep(const uint8_t* pub, const Keys384& kt, const KeyReg384& g, uint32_t j) {
  uint32_t qx[14], qy[14];
  const bool ok = key_import384(pub + (size_t)j * 96, qx, qy);
  uint32_t slot = kNoSlot384;
  if (ok) {
    stw<14>(kt.qx, j, kt.nks, qx);
    stw<14>(kt.qy, j, kt.nks, qy);
    if (g.cap) {
      uint32_t k[24];
      key384_words(pub + (size_t)j * 96, k);
      slot = keys384_find(g, k);
    }
  }
  kt.st[j] = ok ? (uint8_t)R_OK : (uint8_t)R_BAD_KEY;
  kt.slot[j] = slot;
}

// Record i on the table route: true iff x(u1 G + u2 Q) mod n == r. qtab is the
// table of the record's key. u2 Q first, windows upwards from an empty
// accumulator, then u1 G windows upwards: 24 scalar words of 8 digits each.
// While Q is walked the accumulator is (u2 mod 16^w) Q with u2 mod 16^w <
// 16^w <= d 16^w, and their sum is below n (for w = 95 it is at most u2 < n), so
// it is neither the entry nor its negative: the exceptional cases of the mixed
// addition can only be met on the walk of G, where the accumulator u2 Q +
// (u1 mod 16^w) G is any point an input cares to make it
// (tests/golden/p384_keywin_vectors.jsonl).
BH_HD bool stage384_keywin(const Work384& w, const uint32_t* qtab, const uint32_t* gtab, uint32_t i) {
  J384 A;
  A.inf = 1;
#pragma unroll 1
  for (int t = 0; t < 24; t++) {
    const int k = t < 12 ? t : t - 12;
    uint32_t word = (t < 12 ? w.r : w.e)[(size_t)k * w.ns + i];
    const uint32_t* tab = (t < 12 ? qtab : gtab) + (size_t)k * 8 * kG384Ent * kG384Words;
#pragma unroll 1
    for (int b = 0; b < 8; b++, word >>= 4, tab += kG384Ent * kG384Words) {
      const uint32_t d = word & 15u;
      if (d == 0) continue;
      const uint32_t* row = tab + (size_t)(d - 1) * kG384Words;
      uint32_t x[14], y[14];
#pragma unroll
      for (int j = 0; j < 14; j++) {
        x[j] = row[j];
        y[j] = row[14 + j];
      }
      j384_madd_inl(&A, x, y, 0);
    }
  }
  return x_check384(w, i, &A);
}

}  // namespace bh
