// SHA-384 / SHA-512 (FIPS 180-4), one message per lane, message bytes read
// straight from HBM. Replaces bccsp/sw/hash.go:29-33 with the hashers of
// bccsp/sw/new.go:69-73 (SHA384Opts, security level 384: bccsp/sw/conf.go:43-46)
// and the hashes of crypto/x509 checkSignature for ecdsa-with-SHA384 / -SHA512.
//
// CDNA4 has no 64-bit rotate or logic instruction, so a word is a pair of
// 32-bit halves on the device: a rotation is two v_alignbit_b32 (the halves
// swap roles for a rotation of 32 or more), the three-way xors one
// v_bitop3_b32 per half, Ch and Maj one expression per half. Only the adds
// stay 64-bit (v_add_co / v_addc pairs from the compiler). Host builds (the
// CPU harness) take the plain 64-bit expressions.
#pragma once
#include "bh_common.h"
#include "sha256.h"

namespace bh {

#if defined(__HIPCC__)
__device__ __constant__ static const uint64_t kSha512K[80] = {
#else
static const uint64_t kSha512K[80] = {
#endif
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

BH_HD uint64_t sha512_join(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

// x rotated right by N (0 < N < 64, N != 32)
template <int N>
BH_HD uint64_t sha512_rotr(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if constexpr (N < 32)
    return sha512_join(__builtin_amdgcn_alignbit(lo, hi, N), __builtin_amdgcn_alignbit(hi, lo, N));
  else
    return sha512_join(__builtin_amdgcn_alignbit(hi, lo, N - 32),
                       __builtin_amdgcn_alignbit(lo, hi, N - 32));
#else
  return (x >> N) | (x << (64 - N));
#endif
}

BH_HD uint64_t sha512_xor3(uint64_t a, uint64_t b, uint64_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sha512_join(sha_xor3((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32)),
                     sha_xor3((uint32_t)a, (uint32_t)b, (uint32_t)c));
#else
  return a ^ b ^ c;
#endif
}

BH_HD uint32_t sha512_ch32(uint32_t e, uint32_t f, uint32_t g) { return g ^ (e & (f ^ g)); }
BH_HD uint32_t sha512_maj32(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }

BH_HD uint64_t sha512_ch(uint64_t e, uint64_t f, uint64_t g) {
  return sha512_join(sha512_ch32((uint32_t)(e >> 32), (uint32_t)(f >> 32), (uint32_t)(g >> 32)),
                     sha512_ch32((uint32_t)e, (uint32_t)f, (uint32_t)g));
}
BH_HD uint64_t sha512_maj(uint64_t a, uint64_t b, uint64_t c) {
  return sha512_join(sha512_maj32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32)),
                     sha512_maj32((uint32_t)a, (uint32_t)b, (uint32_t)c));
}

// one round; wk = W[t] + K[t]
BH_HD void sha512_round(uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d, uint64_t& e,
                        uint64_t& f, uint64_t& g, uint64_t& hh, uint64_t wk) {
  const uint64_t S1 = sha512_xor3(sha512_rotr<14>(e), sha512_rotr<18>(e), sha512_rotr<41>(e));
  const uint64_t t1 = (hh + wk) + S1 + sha512_ch(e, f, g);
  const uint64_t S0 = sha512_xor3(sha512_rotr<28>(a), sha512_rotr<34>(a), sha512_rotr<39>(a));
  const uint64_t mj = sha512_maj(a, b, c);
  hh = g;
  g = f;
  f = e;
  e = d + t1;
  d = c;
  c = b;
  b = a;
  a = t1 + S0 + mj;
}

// schedule word T >= 16 into the 16-word ring (every index a constant)
template <int T>
BH_HD uint64_t sha512_sched(uint64_t w[16]) {
  const uint64_t w15 = w[(T - 15) & 15], w2 = w[(T - 2) & 15];
  const uint64_t s0 = sha512_xor3(sha512_rotr<1>(w15), sha512_rotr<8>(w15), w15 >> 7);
  const uint64_t s1 = sha512_xor3(sha512_rotr<19>(w2), sha512_rotr<61>(w2), w2 >> 6);
  const uint64_t wi = w[T & 15] + s0 + w[(T - 7) & 15] + s1;
  w[T & 15] = wi;
  return wi;
}

// rounds T .. 79 by template recursion: the ring is indexed by constants only
// (a runtime index would put it in scratch)
template <int T>
BH_HD void sha512_rounds_from(uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d, uint64_t& e,
                              uint64_t& f, uint64_t& g, uint64_t& hh, uint64_t w[16]) {
  if constexpr (T < 80) {
    uint64_t wi;
    if constexpr (T < 16) wi = w[T];
    else wi = sha512_sched<T>(w);
    sha512_round(a, b, c, d, e, f, g, hh, wi + kSha512K[T]);
    sha512_rounds_from<T + 1>(a, b, c, d, e, f, g, hh, w);
  }
}

// The compression function: h = h + rounds(h, w); w (16 big-endian message
// words, already as integers) is consumed.
BH_HD void sha512_block(uint64_t h[8], uint64_t w[16]) {
  uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
  sha512_rounds_from<0>(a, b, c, d, e, f, g, hh, w);
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// Every load of message bytes in this file goes through these two (a byte at
// an address, an aligned dword at a pointer). The sanitizer self-test
// (tests/native_sha512/sha512_selftest.cpp) defines them itself to check each
// address against the message's bounds before it loads.
#ifndef BH_SHA512_LD_U8
#define BH_SHA512_LD_U8(a) (*reinterpret_cast<const uint8_t*>(a))
#define BH_SHA512_LD_U32(p) ld_aligned_u32(p)
#endif

// The bytes of the aligned dword at address q that lie in [lo, hi), in their
// little-endian places, zero elsewhere. Reads those bytes only.
BH_HD uint32_t sha512_partial_dword(uintptr_t q, uintptr_t lo, uintptr_t hi) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uintptr_t a = q + k;
    if (a >= lo && a < hi) v |= (uint32_t)BH_SHA512_LD_U8(a) << (8 * k);
  }
  return v;
}

// The 16 big-endian words of block blk (byte offset) of the padded stream:
// bytes [0, len) are the message at address lo, then 0x80, zeros, and the
// 128-bit big-endian bit length in the last 16 bytes (its upper 64 bits zero).
// One path for every block, any alignment: the aligned dwords that lie wholly
// inside the message load whole; the two that can straddle its ends (headv at
// the dword holding the first byte, tailv at the one holding the byte after
// the last, both from sha512_partial_dword) were read byte by byte; every other
// dword is zero without a load. So no byte outside [lo, lo + len) is read.
BH_HD void sha512_load_block(uint64_t w[16], uintptr_t lo, uint64_t len, uint64_t total,
                             uint64_t blk, uint32_t headv, uint32_t tailv) {
  const uint32_t a = (uint32_t)(lo & 3u);
  // dword j of the block is at base + 4 j, stream position blk + 4 j - a
  const uint8_t* base = reinterpret_cast<const uint8_t*>(lo - a + (uintptr_t)blk);
  // message bytes from base on (capped: 33 dwords are looked at), and the
  // index of the dword holding the byte after the last (99: not in this block)
  const uint64_t end = a + len;
  const uint32_t rem = end <= blk ? 0u : (end - blk > 200 ? 200u : (uint32_t)(end - blk));
  const uint32_t tj = (end >= blk && end - blk < 132) ? (uint32_t)(end - blk) >> 2 : 99u;
  const bool first = blk == 0;
  uint32_t d[33];
#pragma unroll
  for (int j = 0; j < 33; j++) {
    const bool whole = 4u * j + 4u <= rem && (j > 0 || !first || a == 0u);
    if (whole) d[j] = BH_SHA512_LD_U32(base + 4 * j);
    else d[j] = (uint32_t)j == tj ? tailv : ((j == 0 && first) ? headv : 0u);
  }
  // the 0x80 after the last byte: word pj of this block (99: another block)
  const uint32_t pj = (len >= blk && len - blk < 128) ? (uint32_t)(len - blk) >> 2 : 99u;
  const uint32_t pbit = 0x80u << (8 * (3 - (uint32_t)(len & 3u)));
  uint32_t t[32];
#pragma unroll
  for (int j = 0; j < 32; j++) {
    t[j] = bswap32(funnel_bytes(d[j], d[j + 1], a));
    if ((uint32_t)j == pj) t[j] |= pbit;
  }
  if (blk + 128 == total) {
    t[30] |= (uint32_t)((len * 8) >> 32);
    t[31] |= (uint32_t)(len * 8);
  }
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = sha512_join(t[2 * i], t[2 * i + 1]);
}

// h = the chaining value after all of m[0, len) and its padding. With
// len == 0, m is not dereferenced.
BH_HD void sha512_absorb(uint64_t h[8], const uint8_t* m, uint64_t len) {
  const uint64_t total = ((len + 17 + 127) / 128) * 128;
  const uintptr_t lo = (uintptr_t)m, hi = lo + (uintptr_t)len;
  const uint32_t headv = sha512_partial_dword(lo & ~(uintptr_t)3, lo, hi);
  const uint32_t tailv = sha512_partial_dword(hi & ~(uintptr_t)3, lo, hi);
  for (uint64_t blk = 0; blk < total; blk += 128) {
    uint64_t w[16];
    sha512_load_block(w, lo, len, total, blk, headv, tailv);
    sha512_block(h, w);
  }
}

// out = SHA-512(m[0, len)) as 8 big-endian 64-bit words (out[0] most significant).
BH_HD void sha512_msg(uint64_t out[8], const uint8_t* m, uint64_t len) {
  uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                   0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                   0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  sha512_absorb(h, m, len);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = h[i];
}

// out = SHA-384(m[0, len)): the first 6 words of the SHA-512 chain from its own IV.
BH_HD void sha384_msg(uint64_t out[6], const uint8_t* m, uint64_t len) {
  uint64_t h[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull,
                   0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
                   0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
  sha512_absorb(h, m, len);
#pragma unroll
  for (int i = 0; i < 6; i++) out[i] = h[i];
}

// OUT_BYTES 48: SHA-384, 64: SHA-512; the digest as bytes, big-endian.
template <int OUT_BYTES>
BH_HD void sha512_family_bytes(uint8_t* out, const uint8_t* m, uint64_t len) {
  static_assert(OUT_BYTES == 48 || OUT_BYTES == 64, "SHA-384 or SHA-512");
  uint64_t h[8];
  if constexpr (OUT_BYTES == 48) sha384_msg(h, m, len);
  else sha512_msg(h, m, len);
#pragma unroll
  for (int i = 0; i < OUT_BYTES / 8; i++) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[8 * i + k] = (uint8_t)(h[i] >> (56 - 8 * k));
  }
}

}  // namespace bh
