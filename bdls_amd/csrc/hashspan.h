// Span records of bh_hash / bh_fabric_block_prevalidate: a record is up to
// three byte spans (off, len) of one data buffer hashed as one message
// (protoutil.ComputeTxID's nonce || creator, protoutil/proputils.go:351-370;
// GetProposalHash2's channel_header || action header || chaincode proposal
// payload, protoutil/txutils.go:449-466 -- without a host-side concatenation),
// and an optional expected span the digest is compared with. A zero-length
// span contributes nothing. The N-span forms of sha256.h's and sha3.h's
// two-span loaders: blocks wholly inside one span load by dwords, the blocks
// straddling a seam and the padding go byte by byte. BH_HD: the same code runs
// in hash_kernels.hip and in the test-only host harness.
#pragma once
#include "sha256.h"
#include "sha3.h"

namespace bh {

// identical to include/bdls_hip.h (BH_HASH_*)
enum : uint8_t { HS_MATCH = 0, HS_MISMATCH = 1, HS_RANGE = 2 };
enum : uint8_t { HS_WANT_RAW = 0, HS_WANT_HEX = 1 };
constexpr uint32_t kHashMaxSpans = 3;

// A hash batch as the kernels see it (device pointers; the harness: host).
struct HashIn {
  const uint8_t* data;
  uint64_t data_len;
  const uint64_t* off;  // n * nspan, record-major
  const uint32_t* len;
  uint32_t nspan;  // 1..3
  const uint64_t* want_off;  // all three NULL: nothing to compare
  const uint32_t* want_len;
  const uint8_t* want_kind;
};

// One record's spans in message order. end[k]: message length up to and
// including span k (end[2] is the message length); absent spans are empty.
struct HSpans {
  const uint8_t* p[kHashMaxSpans];
  uint64_t end[kHashMaxSpans];
};

// [off, off + len) inside [0, data_len), with no sum that can wrap
BH_HD bool hs_in_range(uint64_t off, uint32_t len, uint64_t data_len) {
  return off <= data_len && (uint64_t)len <= data_len - off;
}

// Record i of `in`. False: a span or the expected span ends beyond data_len
// (HS_RANGE) -- sp is then the empty message and nothing of data is read.
BH_HD bool hs_record(const HashIn& in, uint32_t i, HSpans& sp) {
  bool ok = true;
  uint64_t off[kHashMaxSpans];
  uint32_t len[kHashMaxSpans];
#pragma unroll
  for (uint32_t k = 0; k < kHashMaxSpans; k++) {
    const bool have = k < in.nspan;
    off[k] = have ? in.off[(uint64_t)i * in.nspan + k] : 0u;
    len[k] = have ? in.len[(uint64_t)i * in.nspan + k] : 0u;
    ok = ok && hs_in_range(off[k], len[k], in.data_len);
  }
  if (in.want_off) ok = ok && hs_in_range(in.want_off[i], in.want_len[i], in.data_len);
  uint64_t acc = 0;
#pragma unroll
  for (uint32_t k = 0; k < kHashMaxSpans; k++) {
    // an empty span's pointer is never dereferenced: keep it at the buffer
    sp.p[k] = (ok && len[k]) ? in.data + off[k] : in.data;
    acc += ok ? len[k] : 0u;
    sp.end[k] = acc;
  }
  return ok;
}

BH_HD uint32_t hs_byte(const HSpans& sp, uint64_t p) {
  return p < sp.end[0] ? sp.p[0][p] : p < sp.end[1] ? sp.p[1][p - sp.end[0]] : sp.p[2][p - sp.end[1]];
}

// where [blk, blk + nbytes) lies wholly inside one span: its address there
BH_HD const uint8_t* hs_block_src(const HSpans& sp, uint64_t blk, uint64_t nbytes) {
  if (blk + nbytes <= sp.end[0]) return sp.p[0] + blk;
  if (blk >= sp.end[0] && blk + nbytes <= sp.end[1]) return sp.p[1] + (blk - sp.end[0]);
  if (blk >= sp.end[1] && blk + nbytes <= sp.end[2]) return sp.p[2] + (blk - sp.end[1]);
  return nullptr;
}

// ---- SHA-256 -----------------------------------------------------------------
BH_HD uint64_t sha256_padded_len(uint64_t len) { return ((len + 9 + 63) / 64) * 64; }

// big-endian word at byte pos of the padded stream (sha256_word2 over N spans)
BH_HD uint32_t sha256_word_n(const HSpans& sp, uint64_t total, uint64_t pos) {
  const uint64_t len = sp.end[kHashMaxSpans - 1];
  uint32_t w = 0;
  const uint64_t bits = len * 8;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint64_t p = pos + k;
    uint32_t byte;
    if (p < len) byte = hs_byte(sp, p);
    else if (p == len) byte = 0x80u;
    else if (p >= total - 8) byte = (uint32_t)(bits >> (8 * (total - 1 - p))) & 0xffu;
    else byte = 0;
    w = (w << 8) | byte;
  }
  return w;
}

// The 16 big-endian words of padded block blk (byte offset) of the record.
BH_HD void sha256_load_block_n(uint32_t w[16], const HSpans& sp, uint64_t total, uint64_t blk) {
  const uint8_t* src = hs_block_src(sp, blk, 64);
  if (src) {
    load_le_words<16>(w, src);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = bswap32(w[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = sha256_word_n(sp, total, blk + 4 * i);
  }
}

// The digest as 8 words whose little-endian bytes are the digest bytes.
BH_HD void sha256_spans(uint32_t d[8], const HSpans& sp) {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  const uint64_t total = sha256_padded_len(sp.end[kHashMaxSpans - 1]);
  for (uint64_t blk = 0; blk < total; blk += 64) {
    uint32_t w[16], wk[64];
    sha256_load_block_n(w, sp, total, blk);
    sha256_sched_wk(wk, w);
    sha256_rounds_wk(h, wk);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = bswap32(h[k]);
}

// ---- SHA3-256 ----------------------------------------------------------------
// little-endian word at byte pos of the padded stream (sha3_word2 over 3 spans)
BH_HD uint32_t sha3_word3(const HSpans& sp, uint64_t total, uint64_t pos) {
  const uint64_t len = sp.end[kHashMaxSpans - 1];
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint64_t p = pos + k;
    uint32_t byte = 0;
    if (p < len) byte = hs_byte(sp, p);
    else if (p == len) byte = 0x06u;
    if (p == total - 1) byte |= 0x80u;
    v |= byte << (8 * k);
  }
  return v;
}

BH_HD void sha3_256_spans(uint32_t d[8], const HSpans& sp) {
  K64 a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = K64{0u, 0u};
  const uint64_t len = sp.end[kHashMaxSpans - 1];
  const uint64_t total = (len / kSha3Rate + 1) * kSha3Rate;
  for (uint64_t blk = 0; blk < total; blk += kSha3Rate) {  // one permutation call site
    uint32_t w[34];
    const uint8_t* src = hs_block_src(sp, blk, kSha3Rate);
    if (src) {
      load_le_words<34>(w, src);
    } else {
#pragma unroll
      for (int i = 0; i < 34; i++) w[i] = sha3_word3(sp, total, blk + 4 * i);
    }
#pragma unroll
    for (int i = 0; i < 17; i++) {
      a[i].lo ^= w[2 * i];
      a[i].hi ^= w[2 * i + 1];
    }
    keccak_f1600(a);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    d[2 * i] = a[i].lo;
    d[2 * i + 1] = a[i].hi;
  }
}

// ---- the compare step --------------------------------------------------------
BH_HD uint32_t hs_digest_byte(const uint32_t d[8], uint32_t j) {
  return (d[j >> 2] >> (8 * (j & 3u))) & 0xffu;
}

// lowercase hex digit, as Go's hex.EncodeToString writes it
BH_HD uint32_t hs_hex(uint32_t nib) { return nib < 10u ? 0x30u + nib : 0x61u + (nib - 10u); }

// HS_MATCH iff the expected span equals the digest under `kind`:
//   HS_WANT_RAW  want_len == 32 and the bytes match (bytes.Equal,
//                core/common/validation/msgvalidation.go:238)
//   HS_WANT_HEX  want_len == 64 and the bytes are the lowercase hex of the
//                digest (hex.EncodeToString and a string compare,
//                protoutil/proputils.go:351-370: upper case does not match)
// Any other kind is HS_MISMATCH. A wrong length reads nothing.
BH_HD uint8_t hs_compare(const uint32_t d[8], const uint8_t* want, uint32_t want_len,
                         uint8_t kind) {
  uint32_t diff = 0;
  if (kind == HS_WANT_RAW) {
    if (want_len != 32u) return HS_MISMATCH;
    for (uint32_t j = 0; j < 32u; j++) diff |= hs_digest_byte(d, j) ^ want[j];
  } else if (kind == HS_WANT_HEX) {
    if (want_len != 64u) return HS_MISMATCH;
    for (uint32_t j = 0; j < 32u; j++) {
      const uint32_t b = hs_digest_byte(d, j);
      diff |= (hs_hex(b >> 4) ^ want[2 * j]) | (hs_hex(b & 15u) ^ want[2 * j + 1]);
    }
  } else {
    return HS_MISMATCH;
  }
  return diff ? HS_MISMATCH : HS_MATCH;
}

// record i's result byte (the record is in range: hs_record returned true)
BH_HD uint8_t hs_result(const HashIn& in, uint32_t i, const uint32_t d[8]) {
  return hs_compare(d, in.data + in.want_off[i], in.want_len[i], in.want_kind[i]);
}

}  // namespace bh
