// HIP kernel (gfx950) of the SHA-384 / SHA-512 digest pre-pass
// (BH_F_HASH_SHA384, BH_F_HASH_SHA512). The hash lives in sha512.h (shared
// with the test-only host harness); this file only maps lanes to records. A
// translation unit of its own: the curve passes (verify_kernels.hip,
// verify384_kernels.hip) do not change and then run in digest mode over the
// buffer written here.
//
//   k_sha512<48|64>  1 lane/record   digest, and the digest batch's off / len
#include "sha512.h"

using namespace bh;

template <int OUT_BYTES>
__global__ __launch_bounds__(256) void k_sha512(const uint8_t* __restrict__ msg,
                                                const uint64_t* __restrict__ msg_off,
                                                const uint32_t* __restrict__ msg_len, uint32_t n,
                                                uint8_t* __restrict__ dig,
                                                uint64_t* __restrict__ off,
                                                uint32_t* __restrict__ len) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t mlen = msg_len[i];
  uint64_t h[8];
  // an empty message's offset is not used: its pointer is never formed
  const uint8_t* m = mlen ? msg + msg_off[i] : nullptr;
  if constexpr (OUT_BYTES == 48) sha384_msg(h, m, mlen);
  else sha512_msg(h, m, mlen);
  // dig is 256-byte aligned and OUT_BYTES a multiple of 16: 16-byte stores
  uint4* o = reinterpret_cast<uint4*>(dig + (size_t)i * OUT_BYTES);
#pragma unroll
  for (int k = 0; k < OUT_BYTES / 16; k++) {
    const uint64_t a = h[2 * k], b = h[2 * k + 1];
    o[k] = make_uint4(bswap32((uint32_t)(a >> 32)), bswap32((uint32_t)a),
                      bswap32((uint32_t)(b >> 32)), bswap32((uint32_t)b));
  }
  off[i] = (uint64_t)i * OUT_BYTES;
  len[i] = OUT_BYTES;
}

namespace bh {

// out_bytes 48: SHA-384, 64: SHA-512. dig: n * out_bytes bytes, 16-byte aligned.
hipError_t launch_sha512(int out_bytes, const uint8_t* msg, const uint64_t* msg_off,
                         const uint32_t* msg_len, uint32_t n, uint8_t* dig, uint64_t* off,
                         uint32_t* len, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (out_bytes != 48 && out_bytes != 64) return hipErrorInvalidValue;
  const dim3 blk(256), grd((n + 255) / 256);
  if (out_bytes == 48)
    hipLaunchKernelGGL(k_sha512<48>, grd, blk, 0, s, msg, msg_off, msg_len, n, dig, off, len);
  else
    hipLaunchKernelGGL(k_sha512<64>, grd, blk, 0, s, msg, msg_off, msg_len, n, dig, off, len);
  return hipGetLastError();
}

}  // namespace bh
