// ECDSA P-384 verification stages (BH_CURVE_P384): the sw provider's Verify
// for a P-384 key (bccsp/sw/ecdsa.go:41-57 over crypto/ecdsa verifyNISTEC)
// with the semantics verify.h gives P-256 -- Go-asn1 DER, R, S > 0, Fabric's
// low-S rule with P-384's half order, pointFromAffine key checks, r, s < n,
// hashToNat, x(u1 G + u2 Q) mod n == r -- and the same BH_R_* precedence.
//
// Stages, one record per lane unless noted:
//   stage384_prep    parse + checks + digest -> e, r, s R (mod n), Q, r R (mod p)
//   stage384_inv     s^-1 for a strided chunk of records by Montgomery's trick
//                    (one Fermat inversion per chunk), then u1 = e / s, u2 = r / s
//   stage384_ladder  u2 Q by a signed 4-bit window over a per-record table of
//                    1Q..8Q, then + u1 G from the fixed-base table, x check
//   gtab384_entry    one entry of the fixed-base table of G (built once)
// Every function is BH_HD: tests/native/hostsim384.cpp runs the same code.
#pragma once
#include "bh_common.h"
#include "der.h"
#include "ec384.h"
#include "sha256.h"
#include "sha3.h"

namespace bh {

using N384 = Fn_p384;

constexpr uint32_t F384_HASH_SHA256 = 1u, F384_NO_LOW_S = 2u, F384_HASH_SHA3_256 = 8u;
constexpr uint8_t ST384_R2OK = 0x80;  // r + n < p: the second x candidate is live

// The distinct keys of an index-keyed pass (In384::key_idx), imported once per
// shard by keys384_prep (keys384.h), one lane per key: word k of key j's
// coordinate at qx[k * nks + j], the layout of Work384, so the lanes of the
// import store side by side and a wave whose records share a few keys gathers
// a few cache lines per word.
struct Keys384 {
  uint32_t nk = 0;           // keys
  uint32_t nks = 0;          // nk rounded up to 64
  uint32_t* qx = nullptr;    // 14: Q.x R mod p, canonical
  uint32_t* qy = nullptr;    // 14
  uint8_t* st = nullptr;     // [nk] key_import384's verdict: R_OK or R_BAD_KEY
  uint32_t* slot = nullptr;  // [nk] the key's slot in the registry, or 0xffffffff
};

struct In384 {  // device pointers (include/bdls_hip.h bh_batch, 96-byte keys)
  const uint8_t* pub;  // key_idx == nullptr: record i's key at pub + 96 i; else the kt.nk distinct keys
  const uint8_t* sig;
  const uint64_t* sig_off;
  const uint32_t* sig_len;
  const uint8_t* msg;
  const uint64_t* msg_off;
  const uint32_t* msg_len;
  uint32_t flags;
  // msg[msg_off, +msg_len) || msg[msg2_off, +msg2_len) in the fused modes
  // (digest mode never reads them); nullptr = one span
  const uint64_t* msg2_off = nullptr;
  const uint32_t* msg2_len = nullptr;
  // index-keyed batches (bh_verify384_compact, bh_batch_verify384_ptrs): record
  // i's key is key key_idx[i] (< kt.nk) of pub, already imported into kt
  const uint32_t* key_idx = nullptr;
  Keys384 kt{};
};

// The 96 key bytes of record i: the one place that knows the two key layouts.
BH_HD const uint8_t* in384_key(const In384& in, uint32_t i) {
  return in.pub + (size_t)(in.key_idx ? in.key_idx[i] : i) * 96;
}

// Workspace, structure of arrays: word k of record i at base[k * ns + i].
struct Work384 {
  uint32_t ns;      // records rounded up to 64
  uint32_t* e;      // 12: e, then u1
  uint32_t* r;      // 12: r, then u2
  uint32_t* sm;     // 14: s R mod n
  uint32_t* pre;    // 14: prefix products of the inverse
  uint32_t* qx;     // 14: Q.x R mod p
  uint32_t* qy;     // 14
  uint32_t* rm;     // 14: r R mod p
  uint32_t* r2m;    // 14: (r + n) R mod p when ST384_R2OK
  uint32_t* qtab;   // 8 entries x 3 coordinates x 14 limbs: 1Q..8Q (Jacobian)
  uint8_t* st;      // reason | ST384_R2OK
};
constexpr size_t kWork384Words = 12 + 12 + 14 * 6 + 8 * 3 * 14;  // per record, + 1 byte

// Fixed-base table of G: window w (4 bits, 96 windows), digit d in 1..15 ->
// d 16^w G, affine Montgomery x || y (28 words) at ((w * 15) + d - 1) * 28.
constexpr int kG384Win = 96, kG384Ent = 15, kG384Words = 28;
constexpr size_t kGTab384Words = (size_t)kG384Win * kG384Ent * kG384Words;

template <int NW>
BH_HD void ldw(uint32_t* v, const uint32_t* base, uint32_t i, uint32_t ns) {
#pragma unroll
  for (int k = 0; k < NW; k++) v[k] = base[(size_t)k * ns + i];
}
template <int NW>
BH_HD void stw(uint32_t* base, uint32_t i, uint32_t ns, const uint32_t* v) {
#pragma unroll
  for (int k = 0; k < NW; k++) base[(size_t)k * ns + i] = v[k];
}

// Key bytes X || Y (48 B big-endian each) -> canonical Montgomery coordinates;
// false unless X, Y < p and the point is on the curve (Go pointFromAffine;
// (0, 0) is not on the curve since b != 0).
BH_HD bool key_import384(const uint8_t* q, uint32_t qx[14], uint32_t qy[14]) {
  uint32_t wx[12], wy[12], pp[12];
  w12_const(pp, Cv_p384::p);
  w12_from_be48(wx, q);
  w12_from_be48(wy, q + 48);
  if (w12_geq(wx, pp) || w12_geq(wy, pp)) return false;
  f384_from_w12(qx, wx);
  f384_from_w12(qy, wy);
  f384_to_mont<P384>(qx, qx);
  f384_to_mont<P384>(qy, qy);
  f384_cond_sub<P384>(qx, qx);
  f384_cond_sub<P384>(qy, qy);
  return j384_on_curve(qx, qy);
}

// e = hashToNat(digest) for record i: the leftmost 48 bytes of the given
// digest (a shorter one whole), or the fused 32-byte hash of the record's one
// or two spans; one reduction mod n.
BH_HD void digest_e384(const In384& in, uint32_t i, uint32_t e[12]) {
  const uint32_t mlen = in.msg_len[i];
  const uint32_t mlen2 = in.msg2_len ? in.msg2_len[i] : 0u;  // fused modes only
  const uint8_t* m = in.msg + in.msg_off[i];
#pragma unroll
  for (int k = 0; k < 12; k++) e[k] = 0;
  if (in.flags & F384_HASH_SHA3_256) {
    uint8_t hb[32];
    if (mlen2) sha3_256_msg2(hb, m, mlen, in.msg + in.msg2_off[i], mlen2);
    else sha3_256_msg(hb, m, mlen);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint8_t* q = hb + 28 - 4 * k;
      e[k] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
  } else if (in.flags & F384_HASH_SHA256) {
    uint32_t h[8];
    if (mlen2) sha256_msg2(h, m, mlen, in.msg + in.msg2_off[i], mlen2);
    else sha256_msg(h, m, mlen);
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = h[7 - k];
  } else {
    const uint32_t L = mlen < 48 ? mlen : 48;
#pragma unroll
    for (int j = 0; j < 48; j++) {  // j = byte index from the least significant end
      uint32_t v = 0;
      if ((uint32_t)j < L) v = m[L - 1 - j];
      e[j >> 2] |= v << (8 * (j & 3));
    }
  }
  uint32_t nn[12], t[12];
  w12_const(nn, Cv_p384::n);
  if (!w12_sub(t, e, nn)) {  // e < 2^384 < 2n: one conditional subtraction
#pragma unroll
    for (int k = 0; k < 12; k++) e[k] = t[k];
  }
}

BH_HD void stage384_prep(const In384& in, const Work384& w, uint32_t i) {
  uint8_t reason = R_OK;
  uint32_t r[12], s[12], e[12];
  uint32_t qx[14], qy[14], sm[14];
  const uint32_t slen = in.sig_len[i];
  const uint32_t mlen = in.msg_len[i];
  const bool fused = (in.flags & (F384_HASH_SHA256 | F384_HASH_SHA3_256)) != 0;
  // impl.go:249-257: empty signature, then empty digest
  if (slen == 0) reason = R_EMPTY_SIG;
  else if (!fused && mlen == 0) reason = R_EMPTY_DIGEST;
  DerSigT<12> ds;
  if (reason == R_OK) reason = der_parse_sig(in.sig + in.sig_off[i], slen, &ds);
  uint32_t half[12], nn[12];
  w12_const(half, Cv_p384::half_n);
  w12_const(nn, Cv_p384::n);
  if (reason == R_OK) {
#pragma unroll
    for (int k = 0; k < 12; k++) { r[k] = ds.r[k]; s[k] = ds.s[k]; }
    // sw/ecdsa.go:48-54 IsLowS with P-384's half order: S <= floor(n/2)
    if (!(in.flags & F384_NO_LOW_S) && (ds.s_big || !w12_geq(half, s))) reason = R_HIGH_S;
  }
  // ---- inside crypto/ecdsa.Verify (verifyNISTEC): Q first, then r, s ranges
  if (reason == R_OK) {
    if (in.key_idx) {  // imported once per key: gather the verdict and the coordinates
      const uint32_t k = in.key_idx[i];
      if (in.kt.st[k] != R_OK) {
        reason = R_BAD_KEY;
      } else {
        ldw<14>(qx, in.kt.qx, k, in.kt.nks);
        ldw<14>(qy, in.kt.qy, k, in.kt.nks);
      }
    } else if (!key_import384(in384_key(in, i), qx, qy)) {
      reason = R_BAD_KEY;
    }
  }
  if (reason == R_OK && (ds.r_big || w12_geq(r, nn))) reason = R_R_RANGE;
  if (reason == R_OK && (ds.s_big || w12_geq(s, nn))) reason = R_S_RANGE;
  if (reason == R_OK) digest_e384(in, i, e);
  uint8_t st = reason;
  if (reason == R_OK) {
    // r R mod p and, when r + n < p, (r + n) R mod p for the x-mod-n check
    uint32_t pmn[12], rn[12], rm[14], r2m[14];
    w12_const(pmn, Cv_p384::p_minus_n);
    f384_from_w12(rm, r);
    f384_to_mont<P384>(rm, rm);   // [2p]
    if (!w12_geq(r, pmn)) {
      st |= ST384_R2OK;
      w12_add(rn, r, nn);         // < p
      f384_from_w12(r2m, rn);
      f384_to_mont<P384>(r2m, r2m);
    } else {
      f384_copy(r2m, rm);
    }
    stw<14>(w.rm, i, w.ns, rm);
    stw<14>(w.r2m, i, w.ns, r2m);
    f384_from_w12(sm, s);
    f384_to_mont<N384>(sm, sm);   // s R mod n [2n]
  } else {
    // a rejected record contributes 1 to its chunk's product and keeps the
    // arithmetic of its lane well defined: e = r = 1, s = 1 (Montgomery), Q = G
#pragma unroll
    for (int k = 0; k < 12; k++) e[k] = r[k] = 0;
    e[0] = r[0] = 1;
    f384_const(sm, N384::r1);
    f384_const(qx, Cv_p384::gx_m);
    f384_const(qy, Cv_p384::gy_m);
  }
  stw<12>(w.e, i, w.ns, e);
  stw<12>(w.r, i, w.ns, r);
  stw<14>(w.sm, i, w.ns, sm);
  stw<14>(w.qx, i, w.ns, qx);
  stw<14>(w.qy, i, w.ns, qy);
  w.st[i] = st;
}

// Lane c owns records c, c + stride, ... (< n): Montgomery's trick, one
// inversion per lane, then u1 = e / s and u2 = r / s as plain integers < n.
BH_HD void stage384_inv(const Work384& w, uint32_t c, uint32_t stride, uint32_t n) {
  if (c >= n) return;
  uint32_t acc[14], x[14];
  f384_const(acc, N384::r1);
  uint32_t last = c;
  for (uint32_t i = c; i < n; i += stride) {
    stw<14>(w.pre, i, w.ns, acc);
    ldw<14>(x, w.sm, i, w.ns);
    f384_mul<N384>(acc, acc, x);  // 4 [2n]
    last = i;
  }
  uint32_t inv[14];
  f384_inv<N384>(inv, acc);       // (prod s_i)^-1 R [2n]
  for (uint32_t i = last;; i -= stride) {
    uint32_t pre[14], wi[14], t[14], tw[12];
    ldw<14>(pre, w.pre, i, w.ns);
    f384_mul<N384>(wi, inv, pre);  // s_i^-1 R [2n]
    ldw<14>(x, w.sm, i, w.ns);
    f384_mul<N384>(inv, inv, x);
    ldw<12>(tw, w.e, i, w.ns);
    f384_from_w12(t, tw);
    f384_mul<N384>(t, t, wi);      // u1 = e w, plain [2n]
    f384_cond_sub<N384>(t, t);
    f384_to_w12(tw, t);
    stw<12>(w.e, i, w.ns, tw);
    ldw<12>(tw, w.r, i, w.ns);
    f384_from_w12(t, tw);
    f384_mul<N384>(t, t, wi);      // u2 = r w, plain
    f384_cond_sub<N384>(t, t);
    f384_to_w12(tw, t);
    stw<12>(w.r, i, w.ns, tw);
    if (i < c + stride) break;
  }
}

// ---- per-record table of 1Q..8Q, [entry][coordinate][limb][record] ----
BH_HD void qtab384_store(const Work384& w, uint32_t i, uint32_t entry, const J384* P) {
  uint32_t* b = w.qtab + (size_t)entry * 42 * w.ns;
  stw<14>(b, i, w.ns, P->x);
  stw<14>(b + (size_t)14 * w.ns, i, w.ns, P->y);
  stw<14>(b + (size_t)28 * w.ns, i, w.ns, P->z);
}
BH_HD void qtab384_load(J384* P, const Work384& w, uint32_t i, uint32_t entry) {
  const uint32_t* b = w.qtab + (size_t)entry * 42 * w.ns;
  ldw<14>(P->x, b, i, w.ns);
  ldw<14>(P->y, b + (size_t)14 * w.ns, i, w.ns);
  ldw<14>(P->z, b + (size_t)28 * w.ns, i, w.ns);
  P->inf = 0;
}

// One entry of the fixed-base table: t = w * 15 + d - 1 -> d 16^w G, affine.
BH_HD void gtab384_entry(uint32_t t, uint32_t* gtab) {
  const uint32_t win = t / kG384Ent, d = t % kG384Ent + 1;
  uint32_t gx[14], gy[14];
  f384_const(gx, Cv_p384::gx_m);
  f384_const(gy, Cv_p384::gy_m);
  J384 B, A;
  j384_set_affine(&B, gx, gy);
#pragma unroll 1
  for (uint32_t k = 0; k < 4 * win; k++) j384_dbl(&B);  // 16^w G
  A.inf = 1;
#pragma unroll 1
  for (int bit = 3; bit >= 0; bit--) {  // d B, d < 16 <<< n: no exceptional case but A = inf
    j384_dbl(&A);
    if ((d >> bit) & 1u) j384_add(&A, &B, 0);
  }
  uint32_t x[14], y[14];
  j384_to_affine(x, y, &A);
  uint32_t* o = gtab + (size_t)t * kG384Words;
#pragma unroll
  for (int k = 0; k < 14; k++) { o[k] = x[k]; o[14 + k] = y[k]; }
}

// Bits [4j, 4j + 4) of a 13-word integer.
BH_HD uint32_t nib13(const uint32_t v[13], int j) { return (v[j >> 3] >> (4 * (j & 7))) & 15u; }

// x(A) mod n == r for record i: x = r, or x = r + n when that is below p.
// False at infinity.
BH_HD bool x_check384(const Work384& w, uint32_t i, const J384* A) {
  if (A->inf) return false;
  uint32_t rm[14];
  ldw<14>(rm, w.rm, i, w.ns);
  if (j384_x_equals(A, rm)) return true;
  if (w.st[i] & ST384_R2OK) {  // x in [n, p): r + n
    ldw<14>(rm, w.r2m, i, w.ns);
    return j384_x_equals(A, rm);
  }
  return false;
}

// Record i: true iff x(u1 G + u2 Q) mod n == r (false at infinity).
BH_HD bool stage384_ladder(const Work384& w, const uint32_t* gtab, uint32_t i) {
  uint32_t qx[14], qy[14];
  ldw<14>(qx, w.qx, i, w.ns);
  ldw<14>(qy, w.qy, i, w.ns);
  J384 A, T;
  // table: 1Q, 2Q = dbl, kQ = (k-1)Q + Q
  j384_set_affine(&T, qx, qy);
  qtab384_store(w, i, 0, &T);
  j384_dbl(&T);
  qtab384_store(w, i, 1, &T);
#pragma unroll 1
  for (uint32_t k = 2; k < 8; k++) {
    j384_madd(&T, qx, qy, 0);
    qtab384_store(w, i, k, &T);
  }
  // u2 + 0x88..8 (96 nibbles): digit j = nibble j - 8 in [-8, 7], j < 96, and
  // the carry out is digit 96 in {0, 1}
  uint32_t v[13];
  {
    uint32_t u2[12];
    ldw<12>(u2, w.r, i, w.ns);
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      c += (uint64_t)u2[k] + 0x88888888u;
      v[k] = (uint32_t)c;
      c >>= 32;
    }
    v[12] = (uint32_t)c;
  }
  A.inf = 1;
  if (v[12] & 1u) qtab384_load(&A, w, i, 0);  // digit 96 = 1
#pragma unroll 1
  for (int j = 95; j >= 0; j--) {
#pragma unroll 1
    for (int k = 0; k < 4; k++) j384_dbl(&A);
    const int d = (int)nib13(v, j) - 8;
    if (d != 0) {  // digit 0: nothing to add
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
      qtab384_load(&T, w, i, mag - 1);
      j384_add(&A, &T, d < 0 ? 1u : 0u);
    }
  }
  // + u1 G from the fixed-base table: no doubling
  uint32_t u1[12];
  ldw<12>(u1, w.e, i, w.ns);
#pragma unroll 1
  for (int j = 0; j < kG384Win; j++) {
    const uint32_t d = (u1[j >> 3] >> (4 * (j & 7))) & 15u;
    if (d == 0) continue;
    const uint32_t* g = gtab + ((size_t)j * kG384Ent + d - 1) * kG384Words;
    uint32_t gx[14], gy[14];
#pragma unroll
    for (int k = 0; k < 14; k++) { gx[k] = g[k]; gy[k] = g[14 + k]; }
    j384_madd(&A, gx, gy, 0);
  }
  return x_check384(w, i, &A);
}

}  // namespace bh
