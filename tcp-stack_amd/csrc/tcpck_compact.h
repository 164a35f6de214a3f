// tcpck_compact.h -- the device pieces every stable stream compaction here
// shares (tcpck_reply.hip, tcpck_resend_queue.hip): one image per lane, a wave
// ballot per chunk of 64 images, a block total per kImagesPerBlock images, ONE
// block that turns the block totals into exclusive offsets, and a survivor's
// index = its block's offset + the waves before it in the block + the chunks
// before it in the wave + the lanes below it in the chunk's ballot.  Order comes
// from the scan alone: no atomic orders anything and no block waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include "tcpck_device.h"
#include "tcpck_reply.h"

namespace tcpck {
namespace compact {

constexpr uint32_t kBlock = 256;                                   // threads of a count / mark / emit block
constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kChunks = reply::kImagesPerBlock / kBlock;      // chunks of 64 images per wave
constexpr uint32_t kScanBlock = 1024;
constexpr uint32_t kScanWaves = kScanBlock / 64;
static_assert(reply::kImagesPerBlock == kBlock * kChunks, "a block is whole chunks");

// Image of chunk 0 of this lane; chunk i is 64 i further on.
__device__ __forceinline__ uint32_t first_image() {
  return blockIdx.x * reply::kImagesPerBlock + (threadIdx.x >> 6) * (64u * kChunks) + (threadIdx.x & 63u);
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(ballot >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(ballot), 0u));
}

// Every wave's survivor count `n` (uniform in the wave) through LDS: the sum of
// the waves before this one.  wave_total: kWaves words of LDS.
__device__ __forceinline__ uint32_t waves_before(uint32_t *wave_total, uint32_t n) {
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) wave_total[w] = n;
  __syncthreads();
  uint32_t at = 0;
#pragma unroll
  for (uint32_t i = 0; i < kWaves; ++i) at += i < w ? wave_total[i] : 0u;
  return at;
}

// The block's total to totals[blockIdx.x].  wave_total as above.
__device__ __forceinline__ void store_block_total(uint32_t *wave_total, uint32_t n, uint32_t *__restrict__ totals) {
  if ((threadIdx.x & 63u) == 0) wave_total[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t i = 0; i < kWaves; ++i) t += wave_total[i];
    totals[blockIdx.x] = t;
  }
}

namespace {

// One block.  totals[0, nblocks) -> exclusive prefix sums in place; *total = the sum.
__global__ void __launch_bounds__(kScanBlock) scan_totals_kernel(uint32_t *__restrict__ totals, uint32_t nblocks,
                                                                 uint64_t *__restrict__ total) {
  __shared__ uint32_t wave_sum[kScanWaves];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t carry = 0;  // (at most 2^31 survivors: u32 holds every offset)
  for (uint32_t base = 0; base < nblocks; base += kScanBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nblocks ? totals[i] : 0u;
    const uint32_t incl = dev::wave_inclusive_scan(v);
    if (lane == 63) wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = 0, step = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanWaves; ++j) {
      const uint32_t s = wave_sum[j];
      before += j < w ? s : 0u;
      step += s;
    }
    if (i < nblocks) totals[i] = carry + before + incl - v;
    carry += step;
    __syncthreads();  // wave_sum is rewritten by the next step
  }
  if (threadIdx.x == 0) *total = carry;
}

}  // namespace

inline hipError_t launch_scan_totals(uint32_t *d_totals, uint32_t blocks, uint64_t *d_total, hipStream_t stream) {
  hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kScanBlock), 0, stream, d_totals, blocks, d_total);
  return hipGetLastError();
}

}  // namespace compact
}  // namespace tcpck
