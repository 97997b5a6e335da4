// TEST-ONLY host build of bdls_amd/csrc/sha512.h (the BH_HD code the
// k_sha512 kernel runs), so SHA-384 / SHA-512 can be checked against hashlib
// and libcrypto without a GPU. Never linked into the product.
#include <cstdint>

#include "../../bdls_amd/csrc/sha512.h"

extern "C" {

// out: 48 bytes, big-endian
void hs_sha384(const uint8_t* m, uint64_t len, uint8_t* out) {
  bh::sha512_family_bytes<48>(out, m, len);
}

// out: 64 bytes, big-endian
void hs_sha512(const uint8_t* m, uint64_t len, uint8_t* out) {
  bh::sha512_family_bytes<64>(out, m, len);
}

// One compression: h (8 words, in place) over the 16 big-endian words of a
// block, given as integers.
void hs_sha512_block(uint64_t h[8], const uint64_t w[16]) {
  uint64_t ring[16];
  for (int i = 0; i < 16; i++) ring[i] = w[i];
  bh::sha512_block(h, ring);
}

}  // extern "C"
