// TEST-ONLY host build of bdls_amd/csrc/hashspan.h (the BH_HD loaders and the
// compare step that k_hash256_grp / k_hash3 run), so span records can be
// checked against hashlib without a GPU. Never linked into the product.
//
// Each entry point hashes ONE record the way a kernel lane does: spans
// (off, len) of `data`, an optional expected span, digest and result out.
// Returns the result byte (BH_HASH_MATCH / _MISMATCH / _RANGE); with no
// expected span (want_kind < 0) it returns MATCH or RANGE.
#include <cstdint>
#include <cstring>

#include "../../bdls_amd/csrc/hashspan.h"

namespace {

int one(int alg, const uint8_t* data, uint64_t data_len, const uint64_t* off, const uint32_t* len,
        uint32_t nspan, uint64_t want_off, uint32_t want_len, int want_kind, uint8_t* digest) {
  const uint8_t kind = (uint8_t)want_kind;
  bh::HashIn in{data, data_len, off, len, nspan, nullptr, nullptr, nullptr};
  if (want_kind >= 0) {
    in.want_off = &want_off;
    in.want_len = &want_len;
    in.want_kind = &kind;
  }
  bh::HSpans sp;
  const bool ok = bh::hs_record(in, 0, sp);
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) {
    if (alg == 1) {
      // block by block through the kernel's loader, schedule and rounds
      bh::sha256_spans(d, sp);
    } else {
      bh::sha3_256_spans(d, sp);
    }
  }
  if (digest)
    for (uint32_t j = 0; j < 32; j++) digest[j] = ok ? (uint8_t)bh::hs_digest_byte(d, j) : 0;
  if (!ok) return bh::HS_RANGE;
  return want_kind >= 0 ? bh::hs_result(in, 0, d) : bh::HS_MATCH;
}

}  // namespace

extern "C" {

int hs_hash256_record(const uint8_t* data, uint64_t data_len, const uint64_t* off,
                      const uint32_t* len, uint32_t nspan, uint64_t want_off, uint32_t want_len,
                      int want_kind, uint8_t* digest) {
  return one(1, data, data_len, off, len, nspan, want_off, want_len, want_kind, digest);
}

int hs_hash3_record(const uint8_t* data, uint64_t data_len, const uint64_t* off,
                    const uint32_t* len, uint32_t nspan, uint64_t want_off, uint32_t want_len,
                    int want_kind, uint8_t* digest) {
  return one(2, data, data_len, off, len, nspan, want_off, want_len, want_kind, digest);
}

}  // extern "C"
