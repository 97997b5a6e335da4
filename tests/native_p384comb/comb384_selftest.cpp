// Stand-alone check of bdls_amd/csrc/comb384.h on the CPU, built with
// -fsanitize=address,undefined: the harness's flagged pass (grouping, comb
// build, the three routes) over a few dozen libcrypto-signed P-384 records,
// every buffer a heap allocation of exactly its size, so a read or write
// outside the grouping tables, the comb slots or the lists is an
// AddressSanitizer error. The reasons must equal the plain ladder pass's, with
// and without the low-S rule, whole and in chunks, with and without one key in
// a registry; the routes and the number of combs must be what the rule says.
#define OPENSSL_SUPPRESS_DEPRECATED
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>

#include <cstdio>

#include "hostsim384_comb.cpp"

namespace {

struct Key {
  EC_KEY* k;
  uint8_t pub[96];
};

Key make_key() {
  Key key{};
  key.k = EC_KEY_new_by_curve_name(NID_secp384r1);
  if (!key.k || EC_KEY_generate_key(key.k) != 1) abort();
  BIGNUM *x = BN_new(), *y = BN_new();
  if (EC_POINT_get_affine_coordinates(EC_KEY_get0_group(key.k), EC_KEY_get0_public_key(key.k), x, y,
                                      nullptr) != 1)
    abort();
  BN_bn2binpad(x, key.pub, 48);
  BN_bn2binpad(y, key.pub + 48, 48);
  BN_free(x);
  BN_free(y);
  return key;
}

}  // namespace

int main() {
  // uses per key: 20, 10, 4, 3, 1 (+ 10 spoiled records of key 0)
  const int uses[5] = {20, 10, 4, 3, 1};
  std::vector<Key> keys;
  for (int k = 0; k < 5; k++) keys.push_back(make_key());
  std::vector<int> owner;
  for (int round = 0; round < 20; round++)
    for (int k = 0; k < 5; k++)
      if (round < uses[k]) owner.push_back(k);  // interleaved
  for (int i = 0; i < 10; i++) owner.push_back(0);
  const uint32_t n = (uint32_t)owner.size();  // 48
  std::vector<uint8_t> pub((size_t)n * 96), sig, msg((size_t)n * 48);
  std::vector<uint64_t> so(n), mo(n);
  std::vector<uint32_t> sl(n), ml(n);
  for (uint32_t i = 0; i < n; i++) {
    const Key& key = keys[owner[i]];
    memcpy(&pub[(size_t)i * 96], key.pub, 96);
    for (int j = 0; j < 48; j++) msg[(size_t)i * 48 + j] = (uint8_t)(37 * i + 11 * j + 5);
    mo[i] = (uint64_t)i * 48;
    ml[i] = 48;
    uint8_t der[128];
    unsigned int dl = 0;
    if (ECDSA_sign(0, &msg[(size_t)i * 48], 48, der, &dl, key.k) != 1) abort();
    const uint32_t spoil = i >= n - 10 ? (i - (n - 10)) % 5 : 99;
    if (spoil == 0) msg[(size_t)i * 48 + 7] ^= 1;        // BH_R_MATH
    if (spoil == 1) pub[(size_t)i * 96 + 95] ^= 1;       // off the curve: BH_R_BAD_KEY
    if (spoil == 2) dl = 0;                              // BH_R_EMPTY_SIG
    if (spoil == 3) ml[i] = 0;                           // BH_R_EMPTY_DIGEST
    so[i] = sig.size();
    sl[i] = dl;
    sig.insert(sig.end(), der, der + dl);
  }
  int bad = 0;
  for (uint32_t flags : {0u, 2u}) {
    std::vector<uint8_t> want(n, 255);
    hs384_verify(pub.data(), sig.data(), so.data(), sl.data(), msg.data(), mo.data(), ml.data(), n,
                 flags, 5, want.data());
    std::vector<int> okc(5, 0);
    uint32_t n_ok = 0;
    for (uint32_t i = 0; i < n; i++) {
      const bool passed = want[i] == R_OK || want[i] == R_MATH;
      // the spoiled key bytes are a key of their own
      if (passed) okc[owner[i]]++;
      n_ok += want[i] == R_OK;
    }
    if (flags == 2u && n_ok < 38) bad |= 1;  // without the low-S rule only the spoiled records fail
    uint32_t want_tables = 0;
    for (int k = 0; k < 5; k++) want_tables += okc[k] >= 4;
    for (uint32_t nreg : {0u, 1u}) {
      for (uint32_t pass_chunk : {0u, 64u}) {
        std::vector<uint8_t> got(n, 254), route(n, 253);
        const uint32_t tables =
            hs384c_verify(pub.data(), sig.data(), so.data(), sl.data(), msg.data(), mo.data(),
                          ml.data(), n, flags, pass_chunk, 5, 4, keys[1].pub, nreg, got.data(),
                          route.data());
        if (memcmp(got.data(), want.data(), n)) {
          fprintf(stderr, "reasons differ: flags %u nreg %u\n", flags, nreg);
          bad |= 2;
        }
        const bool reg1 = nreg && okc[1] > 0;
        if (tables != want_tables - (reg1 && okc[1] >= 4 ? 1 : 0)) {
          fprintf(stderr, "tables %u, expected %u\n", tables, want_tables);
          bad |= 4;
        }
        for (uint32_t i = 0; i < n; i++) {
          const bool passed = want[i] == R_OK || want[i] == R_MATH;
          const int k = owner[i];
          const int r = !passed ? 0 : (reg1 && k == 1) ? 2 : okc[k] >= 4 ? 1 : 0;
          if (route[i] != r) {
            fprintf(stderr, "record %u: route %u, expected %d\n", i, route[i], r);
            bad |= 8;
          }
        }
      }
    }
  }
  for (Key& key : keys) EC_KEY_free(key.k);
  printf("comb384_selftest: %u records, %s\n", n, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
