// HIP kernels (gfx950) of bh_hash: SHA-256 / SHA3-256 over records of up to
// three spans of one buffer, digests and / or comparisons out (hashspan.h has
// the loaders and the compare step, shared with the test-only host harness).
// A translation unit of its own: the verify passes do not change.
//
//   k_hash256_grp   kDigG lanes/record   k_digest_grp's split compression
//                                        (verify_kernels.hip) over N spans
//   k_hash3         1 lane/record        SHA3-256
#include "hashspan.h"

using namespace bh;

namespace {

// digest[i] (32 bytes) and result[i], by lane 0 of a record. Plain vector
// stores: 16-byte stores where the caller's buffer allows, bytes otherwise.
__device__ __forceinline__ void hash_out(const HashIn& in, uint32_t i, bool ok,
                                         const uint32_t d[8], uint8_t* digest, uint8_t* result) {
  if (digest) {
    uint8_t* o = digest + (size_t)i * 32;
    if (((uintptr_t)digest & 15u) == 0) {
      uint4* o16 = reinterpret_cast<uint4*>(o);
      o16[0] = ok ? make_uint4(d[0], d[1], d[2], d[3]) : make_uint4(0u, 0u, 0u, 0u);
      o16[1] = ok ? make_uint4(d[4], d[5], d[6], d[7]) : make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (uint32_t j = 0; j < 32u; j++) o[j] = ok ? (uint8_t)hs_digest_byte(d, j) : (uint8_t)0;
    }
  }
  if (result) result[i] = ok ? hs_result(in, i, d) : (uint8_t)HS_RANGE;
}

// As k_digest_grp: lane l of a record's group expands the schedule of padded
// block base + l into its LDS slot, then the whole group runs the rounds of
// the group's blocks from the slots (every lane the same chain; lane 0
// stores). A record out of range has no blocks: its group only passes the
// barriers.
constexpr uint32_t kDigG = 16, kHashBlock = 128, kDigSlot = 68;  // slot: 64 words + pad (b128)
__global__ __launch_bounds__(kHashBlock) void k_hash256_grp(HashIn in, uint32_t n,
                                                            uint8_t* __restrict__ digest,
                                                            uint8_t* __restrict__ result) {
  __shared__ uint4 s_wk[kHashBlock * kDigSlot / 4];
  const uint32_t i = blockIdx.x * (kHashBlock / kDigG) + threadIdx.x / kDigG;
  const uint32_t l = threadIdx.x % kDigG;
  if (i >= n) return;  // whole groups (kDigG divides the wave)
  HSpans sp;
  const bool ok = hs_record(in, i, sp);
  const uint64_t total = sha256_padded_len(sp.end[kHashMaxSpans - 1]);
  const uint32_t nblk = ok ? (uint32_t)(total / 64) : 0u;
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint4* mine = s_wk + threadIdx.x * (kDigSlot / 4);
  const uint4* grp = s_wk + (threadIdx.x - l) * (kDigSlot / 4);
  for (uint32_t base = 0; base < nblk; base += kDigG) {
    if (base + l < nblk) {
      uint32_t wv[16], wk[64];
      sha256_load_block_n(wv, sp, total, (uint64_t)(base + l) * 64u);
      sha256_sched_wk(wk, wv);
#pragma unroll
      for (int q = 0; q < 16; q++) mine[q] = uint4{wk[4 * q], wk[4 * q + 1], wk[4 * q + 2], wk[4 * q + 3]};
    }
    // the group's slots, written by its other lanes of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t cnt = nblk - base < kDigG ? nblk - base : kDigG;
    for (uint32_t q = 0; q < cnt; q++) {
      uint32_t wk[64];
      const uint4* s = grp + q * (kDigSlot / 4);
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const uint4 v = s[k];
        wk[4 * k] = v.x; wk[4 * k + 1] = v.y; wk[4 * k + 2] = v.z; wk[4 * k + 3] = v.w;
      }
      sha256_rounds_wk(h, wk);
    }
    // every lane's reads of this round of slots precede the next writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (l != 0) return;
  uint32_t d[8];
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = bswap32(h[k]);
  hash_out(in, i, ok, d, digest, result);
}

__global__ __launch_bounds__(256) void k_hash3(HashIn in, uint32_t n, uint8_t* __restrict__ digest,
                                               uint8_t* __restrict__ result) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  HSpans sp;
  const bool ok = hs_record(in, i, sp);
  uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (ok) sha3_256_spans(d, sp);
  hash_out(in, i, ok, d, digest, result);
}

}  // namespace

namespace bh {

// alg: 1 SHA-256, 2 SHA3-256 (BH_HASH_*). digest (n * 32) and result (n) may
// each be NULL; result needs in.want_*.
hipError_t launch_hash(int alg, const HashIn& in, uint32_t n, uint8_t* digest, uint8_t* result,
                       hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (in.nspan < 1 || in.nspan > kHashMaxSpans || (result && !in.want_off))
    return hipErrorInvalidValue;
  if (alg == 1) {
    constexpr uint32_t per = kHashBlock / kDigG;
    hipLaunchKernelGGL(k_hash256_grp, dim3((n + per - 1) / per), dim3(kHashBlock), 0, s, in, n,
                       digest, result);
  } else if (alg == 2) {
    hipLaunchKernelGGL(k_hash3, dim3((n + 255) / 256), dim3(256), 0, s, in, n, digest, result);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bh
