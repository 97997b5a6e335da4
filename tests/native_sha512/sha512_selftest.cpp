// Stand-alone check of bdls_amd/csrc/sha512.h on the CPU, built with
// -fsanitize=address,undefined: SHA-384 and SHA-512 of every length 0..300 at
// every start alignment 0..7 against libcrypto. That no byte outside
// [m, m + len) is read is shown twice:
//   * every load sha512.h makes of message bytes goes through its two load
//     macros, which this program defines: each address range is compared with
//     the bounds of the message being hashed, at both ends, before the load,
//     and a load outside them ends the program;
//   * each message lies in a heap allocation that ends exactly at its last
//     byte, so a read past it is an AddressSanitizer error as well. Alignment
//     0: the allocation is exactly the message (malloc(len)). Alignment a > 0:
//     malloc(len + a) with the message at offset a (the sanitizer's shadow
//     describes 8-byte granules by "the first k bytes are addressable", so it
//     cannot fence bytes below a misaligned start; the first check does), and
//     the bytes below the message differ between two runs (0x00 / 0xff) while
//     the digests must not.
// With len == 0 the pointer handed over is null.
#include <openssl/sha.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../bdls_amd/csrc/bh_common.h"

// bounds of the message being hashed, and the checked loads
static uintptr_t g_lo, g_hi;
static size_t g_loads;
static inline void in_bounds(uintptr_t a, size_t n) {
  if (a < g_lo || a + n > g_hi) {
    fprintf(stderr, "load of %zu bytes at message offset %td outside [0, %zu)\n", n,
            (ptrdiff_t)(a - g_lo), (size_t)(g_hi - g_lo));
    abort();
  }
  g_loads++;
}
static inline uint32_t checked_u8(uintptr_t a) {
  in_bounds(a, 1);
  return *reinterpret_cast<const uint8_t*>(a);
}
static inline uint32_t checked_u32(const uint8_t* p) {
  in_bounds((uintptr_t)p, 4);
  return bh::ld_aligned_u32(p);
}
#define BH_SHA512_LD_U8(a) checked_u8(a)
#define BH_SHA512_LD_U32(p) checked_u32(p)

#include "../../bdls_amd/csrc/sha512.h"

static int check(const uint8_t* m, size_t len, unsigned a, const uint8_t* ref_src) {
  uint8_t got48[48], got64[64], want48[48], want64[64];
  g_lo = (uintptr_t)m;
  g_hi = g_lo + len;
  bh::sha512_family_bytes<48>(got48, m, len);
  bh::sha512_family_bytes<64>(got64, m, len);
  SHA384(ref_src, len, want48);
  SHA512(ref_src, len, want64);
  int bad = 0;
  if (memcmp(got48, want48, 48)) {
    fprintf(stderr, "SHA-384 mismatch: len %zu alignment %u\n", len, a);
    bad = 1;
  }
  if (memcmp(got64, want64, 64)) {
    fprintf(stderr, "SHA-512 mismatch: len %zu alignment %u\n", len, a);
    bad = 1;
  }
  return bad;
}

int main() {
  int bad = 0;
  size_t cases = 0;
  uint8_t ref[301];  // libcrypto reads its own copy
  for (size_t len = 0; len <= 300; len++) {
    for (unsigned a = 0; a < 8; a++) {
      for (size_t i = 0; i < len; i++) ref[i] = (uint8_t)(131 * i + 7 * len + a + 1);
      if (len == 0) {
        bad |= check(nullptr, 0, a, ref);
        cases++;
        continue;
      }
      for (int fill = 0; fill < (a ? 2 : 1); fill++) {
        uint8_t* base = (uint8_t*)malloc(len + a);  // 16-byte aligned: start alignment is a
        if (!base) return 2;
        memset(base, fill ? 0xff : 0x00, a);
        memcpy(base + a, ref, len);
        bad |= check(base + a, len, a, ref);
        free(base);
        cases++;
      }
    }
    if (bad) break;  // one length's report is enough
  }
  // the compression function alone: one hand-fed block ("abc" padded)
  uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                   0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                   0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  uint64_t w[16] = {0x6162638000000000ull};
  w[15] = 24;
  bh::sha512_block(h, w);
  if (h[0] != 0xddaf35a193617abaull || h[7] != 0x2a9ac94fa54ca49full) {
    fprintf(stderr, "sha512_block mismatch on the abc block\n");
    bad = 1;
  }
  if (!g_loads) bad = 1;  // the checked loads are the ones the hash makes
  printf("sha512_selftest: %zu messages, %zu checked loads, %s\n", cases, g_loads,
         bad ? "MISMATCH" : "ok");
  return bad;
}
