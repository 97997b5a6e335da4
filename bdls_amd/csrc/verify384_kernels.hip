// HIP kernels (gfx950) of the P-384 verify pass (BH_CURVE_P384). The stage
// logic lives in verify384.h (shared with the test-only host harness); this
// file only maps lanes to records. A translation unit of its own:
// verify_kernels.hip and the code generated from it do not change.
//
//   k384_gtab    1 lane/entry    fixed-base table of G, once per device
//   k384_prep    1 lane/record   parse + checks + digest + Montgomery inputs
//   k384_inv     1 lane/chunk    s^-1 by Montgomery's trick, u1, u2
//   k384_ladder  1 lane/record   u2 Q (signed window) + u1 G (table), x check
//   k384_bitmap  1 lane/record   validity bitmap from the reason bytes
#include "verify384.h"

using namespace bh;

constexpr uint32_t kInvChunk384 = 16;  // records per inversion

__global__ __launch_bounds__(64) void k384_gtab(uint32_t* __restrict__ gtab) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)(kG384Win * kG384Ent)) return;
  gtab384_entry(t, gtab);
}

__global__ __launch_bounds__(64) void k384_prep(In384 in, Work384 w, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  stage384_prep(in, w, i);
}

__global__ __launch_bounds__(64) void k384_inv(Work384 w, uint32_t stride, uint32_t n) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= stride) return;
  stage384_inv(w, c, stride, n);
}

__global__ __launch_bounds__(64) void k384_ladder(Work384 w, const uint32_t* __restrict__ gtab,
                                                  uint32_t n, uint8_t* __restrict__ reason) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = w.st[i] & 0x7fu;
  if (st != R_OK) {
    reason[i] = st;
    return;
  }
  reason[i] = stage384_ladder(w, gtab, i) ? (uint8_t)R_OK : (uint8_t)R_MATH;
}

__global__ __launch_bounds__(256) void k384_bitmap(const uint8_t* __restrict__ reason, uint32_t n,
                                                   uint64_t* __restrict__ bitmap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ((i & ~63u) >= n) return;
  const bool ok = i < n && reason[i] == R_OK;
  const uint64_t m = __ballot(ok);
  if ((threadIdx.x & 63u) == 0) bitmap[i >> 6] = m;
}

namespace bh {

hipError_t launch_gtab384_build(uint32_t* gtab, hipStream_t s) {
  const uint32_t t = (uint32_t)(kG384Win * kG384Ent);
  hipLaunchKernelGGL(k384_gtab, dim3((t + 63) / 64), dim3(64), 0, s, gtab);
  return hipGetLastError();
}

// ev (optional): 4 events around prep, inverse, ladder + bitmap.
hipError_t launch_verify384(const In384& in, const Work384& w, const uint32_t* gtab, uint32_t n,
                            uint64_t* bitmap, uint8_t* reason, hipStream_t s, hipEvent_t* ev) {
  if (n == 0) return hipSuccess;
  hipError_t e;
  const dim3 blk(64), grd((n + 63) / 64);
  if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k384_prep, grd, blk, 0, s, in, w, n);
  if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
  const uint32_t stride = (n + kInvChunk384 - 1) / kInvChunk384;
  hipLaunchKernelGGL(k384_inv, dim3((stride + 63) / 64), blk, 0, s, w, stride, n);
  if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k384_ladder, grd, blk, 0, s, w, gtab, n, reason);
  hipLaunchKernelGGL(k384_bitmap, dim3((n + 255) / 256), dim3(256), 0, s, reason, n, bitmap);
  if (ev && (e = hipEventRecord(ev[3], s)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace bh
