// Per-pass key combs of BH_CURVE_P384 (BH_F_BATCH_KEYS): a pass groups its
// records by key, builds a comb table for every key that at least `min` of its
// records use (4 unless BH_P384_COMB_MIN says otherwise), and verifies those
// records over the key's comb and an equally shaped comb of G in one walk of 64
// doublings. What k_keycomb does for P-256 (verify.h), for the wider curve;
// nothing outlives the pass.
//
//   comb        6 teeth of 64 bits, unsigned: entry m in 1..63 is
//               sum over the bits j of m of 2^(64 j) Q, affine Montgomery x || y
//               (28 words) at (m - 1) * 28: kComb384Words = 1,764 words = 7,056
//               bytes per key.
//   grouping    open addressing over the records' 96 key bytes (key384_words /
//               key384_hash of keys384.h), buckets a power of two >= 2 ns, linear
//               probing, every hit confirmed on all 24 key words. A bucket holds
//               the index + 1 of the record that claimed it (the group's
//               representative) and the group's count.
//               An index-keyed pass (In384::key_idx) skips all of this: its
//               buckets are the key indices, one atomic addition per record
//               (comb384_index_route below).
//   routing     per group, by its representative: registered keys to the
//               registry's route, groups of >= min records to a comb slot, the
//               rest (and every record prep rejected) to the ladder.
//   build       comb384_bases: one chain of 320 doublings, the six bases
//               2^(64 j) Q kept (Jacobian); comb384_rows: the 63 subset sums,
//               the highest base added last, one inversion by Montgomery's trick.
//   verify      stage384_comb: A = inf; for column c = 63..0: A = 2A, then
//               + TQ[digit of u2], + TG[digit of u1]; the ladder's x check.
// Every function is BH_HD: tests/native_p384comb/hostsim384_comb.cpp runs the
// same code. The compare-and-swap that claims a bucket and the counters'
// atomic additions are the caller's (the kernels' in verify384_kernels.hip,
// plain stores in the sequential harness).
#pragma once
#include "keys384.h"

namespace bh {

constexpr int kComb384Teeth = 6, kComb384Bits = 64, kComb384Ent = 63;
constexpr size_t kComb384Words = (size_t)kComb384Ent * kG384Words;          // a table
constexpr size_t kComb384BaseWords = (size_t)kComb384Teeth * kBase384Words;  // a key's six bases
constexpr uint32_t kComb384MinDefault = 4;
// a group's route (Comb384::gslot): kNoSlot384 = ladder, bit 31 set = the
// registry's slot in the low bits, else the comb slot
constexpr uint32_t kComb384Reg = 0x80000000u;

struct Comb384 {
  uint32_t hc;         // buckets (power of two >= 2 ns: the probe always ends)
  uint32_t cap;        // comb slots (>= ns / min: every qualifying group gets one)
  uint32_t min;        // records of one key in the pass that earn it a comb
  uint32_t* ctr;       // [2] comb slots handed out, records on the comb list (cleared per pass)
  uint32_t* rep;       // [hc] representative record + 1, 0 = empty (cleared per pass)
  uint32_t* cnt;       // [hc] records of the group (cleared per pass)
  uint32_t* gslot;     // [hc] the group's route, written for every claimed bucket
  uint32_t* bkt;       // [ns] per record: its group's bucket, kNoSlot384 if prep rejected it
  uint32_t* list;      // [ns] records on the comb route, ctr[1] of them
  uint32_t* slot_rep;  // [cap] comb slot -> representative record
  uint32_t* bases;     // [cap][kComb384BaseWords] 2^(64 j) Q, Jacobian x, y, z
  uint32_t* side;      // [cap][kComb384Words] per entry Z and the prefix product (build only)
  uint32_t* tables;    // [cap][kComb384Words]
};

BH_HD bool comb384_same_key(const In384& in, uint32_t rec, const uint32_t k[24]) {
  uint32_t q[24];
  key384_words(in384_key(in, rec), q);
  uint32_t d = 0;
#pragma unroll
  for (int j = 0; j < 24; j++) d |= q[j] ^ k[j];
  return d == 0;
}

// The bucket of record i's group, claiming an empty one on the way: cas(p, v)
// stores v at *p if *p is 0 and returns what *p then holds (v, or the earlier
// claim). kNoSlot384 only if every bucket is taken by another key, which
// hc >= 2 ns rules out. The caller counts the record into cnt[bucket].
template <class Cas>
BH_HD uint32_t comb384_claim(const In384& in, const Comb384& cb, uint32_t i, Cas cas) {
  uint32_t k[24];
  key384_words(in384_key(in, i), k);
  uint32_t b = key384_hash(k) & (cb.hc - 1);
  for (uint32_t probes = 0; probes < cb.hc; probes++, b = (b + 1) & (cb.hc - 1)) {
    uint32_t v = cb.rep[b];
    if (v == 0) v = cas(&cb.rep[b], i + 1);
    if (v == i + 1 || comb384_same_key(in, v - 1, k)) return b;
  }
  return kNoSlot384;
}

// What the group of bucket b gets, asked by its representative i once every
// record is counted: its registry slot | kComb384Reg, kNoSlot384 (ladder), or 0
// for "a comb slot", which the caller hands out.
BH_HD uint32_t comb384_group_route(const In384& in, const KeyReg384& g, const Comb384& cb,
                                   uint32_t i, uint32_t b) {
  if (g.cap) {
    uint32_t k[24];
    key384_words(in384_key(in, i), k);
    const uint32_t s = keys384_find(g, k);
    if (s != kNoSlot384) return s | kComb384Reg;
  }
  return cb.cnt[b] >= cb.min ? 0u : kNoSlot384;
}

// The expanded layout by its key bytes alone (key i at pub + 96 i).
template <class Cas>
BH_HD uint32_t comb384_claim(const uint8_t* pub, const Comb384& cb, uint32_t i, Cas cas) {
  return comb384_claim(In384{pub}, cb, i, cas);
}
BH_HD uint32_t comb384_group_route(const uint8_t* pub, const KeyReg384& g, const Comb384& cb,
                                   uint32_t i, uint32_t b) {
  return comb384_group_route(In384{pub}, g, cb, i, b);
}

// Index-keyed passes (In384::key_idx) group by key index instead: bucket j is
// key j (hc >= kt.nk), a record that prep admitted adds one to cnt[key_idx[i]]
// (the caller's atomic addition) and has bkt[i] = key_idx[i]; no fingerprint,
// no claim, no representative. Two indices whose 96 bytes are equal are two
// groups. What key j's group gets, asked once per key when every record is
// counted: as comb384_group_route, the registry slot being the one
// keys384_prep found. A comb slot's slot_rep is then the key index, and its
// bases come from the key workspace.
BH_HD uint32_t comb384_index_route(const Keys384& kt, const Comb384& cb, uint32_t j) {
  if (cb.cnt[j] == 0) return kNoSlot384;  // (no record reads it)
  const uint32_t s = kt.slot[j];
  if (s != kNoSlot384) return s | kComb384Reg;
  return cb.cnt[j] >= cb.min ? 0u : kNoSlot384;
}

// Record i's route from its group's: 0 ladder, 1 comb, 2 registry; *slot is the
// table's slot on the two table routes. Records that prep rejected have no
// group and take the ladder route, which reports their reason.
BH_HD int comb384_record_route(const Comb384& cb, uint32_t i, uint32_t* slot) {
  const uint32_t b = cb.bkt[i];
  if (b == kNoSlot384) return 0;
  const uint32_t r = cb.gslot[b];
  if (r == kNoSlot384) return 0;
  *slot = r & ~kComb384Reg;
  return (r & kComb384Reg) ? 2 : 1;
}

// The chain of a key's comb: bases[j] = 2^(64 j) Q (Jacobian, 42 words) for the
// six teeth, 320 doublings. qx, qy: canonical Montgomery coordinates of a point
// of the curve (prep's, or G's constants). Q has order n and 2^(64 j) < n, so no
// base is infinite.
BH_HD void comb384_bases(const uint32_t qx[14], const uint32_t qy[14], uint32_t* bases) {
  J384 B;
  j384_set_affine(&B, qx, qy);
#pragma unroll 1
  for (int j = 0; j < kComb384Teeth; j++) {
    uint32_t* o = bases + (size_t)j * kBase384Words;
#pragma unroll
    for (int k = 0; k < 14; k++) {
      o[k] = B.x[k];        // [18p] (j = 0: canonical)
      o[14 + k] = B.y[k];   // [18p]
      o[28 + k] = B.z[k];   // [6p]
    }
    if (j + 1 < kComb384Teeth) {
#pragma unroll 1
      for (int k = 0; k < kComb384Bits; k++) j384_dbl_inl(&B);  // in < 20p, out (18, 18, 6)p
    }
  }
}

// The 63 entries of a comb from its bases: E[m] = E[m - 2^t] + B_t, t the
// highest bit of m. E[m - 2^t] is k Q with k < 2^(64 t) (a sum of lower bases)
// and B_t is 2^(64 t) Q, so k differs from 2^(64 t) and k + 2^(64 t) < 2^321 < n:
// the two are neither equal nor opposite, the full addition meets no
// exceptional case, and since Q has order n no entry is infinite and no Z is
// zero. The Jacobian entries wait in memory (X || Y in the entry's own row, Z
// and the running product of the Zs in `side`), never in a private array the
// loops would index at run time; then one inversion for all 63 by Montgomery's
// trick, and each row is overwritten with its canonical affine coordinates.
BH_HD void comb384_rows(const uint32_t* bases, uint32_t* side, uint32_t* rows) {
  uint32_t acc[14];
  f384_const(acc, P384::r1);
#pragma unroll 1
  for (uint32_t m = 1; m <= (uint32_t)kComb384Ent; m++) {
    int t = kComb384Teeth - 1;
    while (!((m >> t) & 1u)) t--;
    const uint32_t rest = m ^ (1u << t);
    const uint32_t* b = bases + (size_t)t * kBase384Words;
    J384 A, T;
#pragma unroll
    for (int k = 0; k < 14; k++) {
      T.x[k] = b[k];        // [18p]
      T.y[k] = b[14 + k];   // [18p]
      T.z[k] = b[28 + k];   // [6p]
    }
    T.inf = 0;
    if (rest) {
      const uint32_t* r = rows + (size_t)(rest - 1) * kG384Words;
      const uint32_t* s = side + (size_t)(rest - 1) * kG384Words;
#pragma unroll
      for (int k = 0; k < 14; k++) {
        A.x[k] = r[k];      // [18p]
        A.y[k] = r[14 + k]; // [18p]
        A.z[k] = s[k];      // [6p]
      }
      A.inf = 0;
      j384_add(&A, &T, 0);  // in < 20p, out (8, 4, 2)p
    } else {
      A = T;                // a base itself (18, 18, 6)p
    }
    uint32_t* o = rows + (size_t)(m - 1) * kG384Words;
    uint32_t* so = side + (size_t)(m - 1) * kG384Words;
#pragma unroll
    for (int k = 0; k < 14; k++) {
      o[k] = A.x[k];
      o[14 + k] = A.y[k];
      so[k] = A.z[k];
      so[14 + k] = acc[k];  // prod of the Zs below m [2p]
    }
    f384_mul<P384>(acc, acc, A.z);          // 2*6 [2p]
  }
  uint32_t inv[14];
  f384_canon<P384>(acc, acc);
  f384_inv<P384>(inv, acc);                 // (prod Z)^-1 [2p]
#pragma unroll 1
  for (int m = kComb384Ent; m >= 1; m--) {
    uint32_t* o = rows + (size_t)(m - 1) * kG384Words;
    const uint32_t* so = side + (size_t)(m - 1) * kG384Words;
    uint32_t x[14], y[14], z[14], pre[14], zi[14], zi2[14], t[14], c[14];
#pragma unroll
    for (int k = 0; k < 14; k++) {
      x[k] = o[k];          // [18p]
      y[k] = o[14 + k];     // [18p]
      z[k] = so[k];         // [6p]
      pre[k] = so[14 + k];  // [2p]
    }
    f384_mul<P384>(zi, inv, pre);           // Z_m^-1, 4 [2p]
    f384_mul<P384>(inv, inv, z);            // 12 [2p]
    f384_sqr<P384>(zi2, zi);                // 4 [2p]
    f384_mul<P384>(t, x, zi2);              // 36 [2p]
    f384_canon<P384>(c, t);
#pragma unroll
    for (int k = 0; k < 14; k++) o[k] = c[k];
    f384_mul<P384>(t, zi, zi2);             // 4 [2p]
    f384_mul<P384>(t, y, t);                // 36 [2p]
    f384_canon<P384>(c, t);
#pragma unroll
    for (int k = 0; k < 14; k++) o[14 + k] = c[k];
  }
}

// Record i on the comb route: true iff x(u1 G + u2 Q) mod n == r. qtab is the
// comb of the record's key, gtab the comb of G. Column c (63..0) takes bit c of
// each 64-bit chunk of a scalar as one digit; the two halves of the walk read
// the chunks' high and low words, selected here so that no array is indexed at
// run time. The accumulator u2' Q + u1' G is whatever an input makes it: every
// mixed addition can meet A == T (it doubles), A == -T (infinity) and
// A == infinity, and the doubling passes infinity through
// (tests/golden/p384_comb_vectors.jsonl drives each of these).
BH_HD bool stage384_comb(const Work384& w, const uint32_t* qtab, const uint32_t* gtab, uint32_t i) {
  uint32_t u1[12], u2[12];
  ldw<12>(u1, w.e, i, w.ns);
  ldw<12>(u2, w.r, i, w.ns);
  J384 A;
  A.inf = 1;
#pragma unroll 1
  for (int h = 1; h >= 0; h--) {
    uint32_t vq[kComb384Teeth], vg[kComb384Teeth];
#pragma unroll
    for (int j = 0; j < kComb384Teeth; j++) {
      vq[j] = h ? u2[2 * j + 1] : u2[2 * j];
      vg[j] = h ? u1[2 * j + 1] : u1[2 * j];
    }
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      j384_dbl_inl(&A);                     // in < 20p (9, 4, 3 or 18, 18, 6), out (18, 18, 6)p
      uint32_t dq = 0, dg = 0;
#pragma unroll
      for (int j = 0; j < kComb384Teeth; j++) {
        dq |= ((vq[j] >> b) & 1u) << j;
        dg |= ((vg[j] >> b) & 1u) << j;
      }
#pragma unroll 1
      for (int t = 0; t < 2; t++) {
        const uint32_t d = t ? dg : dq;
        if (d == 0) continue;
        const uint32_t* row = (t ? gtab : qtab) + (size_t)(d - 1) * kG384Words;
        uint32_t x[14], y[14];
#pragma unroll
        for (int k = 0; k < 14; k++) {
          x[k] = row[k];                    // canonical [p]
          y[k] = row[14 + k];
        }
        j384_madd_inl(&A, x, y, 0);         // in < 20p, out (9, 4, 3)p or a doubling's
      }
    }
  }
  return x_check384(w, i, &A);
}

}  // namespace bh
