// scan_util.h -- wave64 / workgroup prefix-sum and reduction primitives (device only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bce {

// inclusive sum scan across the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o);
    if (lane >= (uint32_t)o) v += t;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_incl_sum64(uint64_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(v, o);
    if (lane >= (uint32_t)o) v += t;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o);
    if (lane >= (uint32_t)o) v = v > t ? v : t;
  }
  return v;
}

// Exclusive sum scan over the NT threads of a block; *total = block sum.  Two barriers.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan_sum(uint32_t v, uint32_t *total) {
  __shared__ uint32_t ws[NT / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_sum(v);
  if (lane == 63) ws[wid] = inc;
  __syncthreads();
  uint32_t wbase = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const uint32_t t = ws[i];
    if ((uint32_t)i < wid) wbase += t;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return wbase + inc - v;
}
template <int NT>
__device__ __forceinline__ uint64_t block_excl_scan_sum64(uint64_t v, uint64_t *total) {
  __shared__ uint64_t ws[NT / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint64_t inc = wave_incl_sum64(v);
  if (lane == 63) ws[wid] = inc;
  __syncthreads();
  uint64_t wbase = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const uint64_t t = ws[i];
    if ((uint32_t)i < wid) wbase += t;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return wbase + inc - v;
}

// Inclusive max scan over the NT threads of a block; *total = block max.
template <int NT>
__device__ __forceinline__ uint32_t block_incl_scan_max(uint32_t v, uint32_t *total) {
  __shared__ uint32_t ws[NT / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_max(v);
  if (lane == 63) ws[wid] = inc;
  __syncthreads();
  uint32_t wbase = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const uint32_t t = ws[i];
    if ((uint32_t)i < wid) wbase = wbase > t ? wbase : t;
    tot = tot > t ? tot : t;
  }
  __syncthreads();
  *total = tot;
  return wbase > inc ? wbase : inc;
}

template <int NT>
__device__ __forceinline__ uint32_t block_reduce_sum(uint32_t v) {
  uint32_t tot;
  (void)block_excl_scan_sum<NT>(v, &tot);
  return tot;
}
template <int NT>
__device__ __forceinline__ uint32_t block_reduce_max(uint32_t v) {
  uint32_t tot;
  (void)block_incl_scan_max<NT>(v, &tot);
  return tot;
}

// Exclusive max scan over the NT threads of a block (0, the identity, for thread 0); *total = block max.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan_max(uint32_t v, uint32_t *total) {
  __shared__ uint32_t ws[NT / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_max(v);
  if (lane == 63) ws[wid] = inc;
  __syncthreads();
  const uint32_t prev = __shfl_up(inc, 1);
  uint32_t ex = lane ? prev : 0u, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const uint32_t t = ws[i];
    if ((uint32_t)i < wid) ex = ex > t ? ex : t;
    tot = tot > t ? tot : t;
  }
  __syncthreads();
  *total = tot;
  return ex;
}

// The sum / the maximum of v over the block, in every thread.
template <int NT>
__device__ __forceinline__ uint64_t block_reduce_sum64(uint64_t v) {
  uint64_t tot;
  (void)block_excl_scan_sum64<NT>(v, &tot);
  return tot;
}
template <int NT>
__device__ __forceinline__ uint64_t block_reduce_max64(uint64_t v) {
  __shared__ uint64_t ws[NT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t t = __shfl_xor(v, o);
    v = v > t ? v : t;
  }
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) m = m > ws[i] ? m : ws[i];
  __syncthreads();
  return m;
}

// ---- the carried pass over per-block results: ONE workgroup of NT threads scans a[0, nb) in place, NT words at a time, and carries
// what the words already done add up to into the next NT.  The carry accumulates: with a carry that is replaced, three passes
// (nb > 2 NT) are the first to come out wrong.
// Exclusive sum scan; returns the grand total, in every thread.
template <int NT>
__device__ __forceinline__ uint64_t block_carried_scan_sum64(uint64_t *a, uint32_t nb) {
  uint64_t carry = 0;
  for (uint32_t at = 0; at < nb; at += NT) {
    const uint32_t i = at + threadIdx.x;
    const uint64_t v = i < nb ? a[i] : 0ull;
    uint64_t tot;
    const uint64_t ex = block_excl_scan_sum64<NT>(v, &tot);
    if (i < nb) a[i] = carry + ex;
    carry += tot;
  }
  return carry;
}
// Exclusive max scan: a[b] = the maximum of the words in front of b, or, Backward, of the words behind it (0 where there is none).
template <int NT, bool Backward>
__device__ __forceinline__ void block_carried_scan_max(uint32_t *a, uint32_t nb) {
  uint32_t carry = 0;
  for (uint32_t at = 0; at < nb; at += NT) {
    const uint32_t r = at + threadIdx.x, i = Backward ? nb - 1u - r : r;
    const uint32_t v = r < nb ? a[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan_max<NT>(v, &tot);
    if (r < nb) a[i] = carry > ex ? carry : ex;
    carry = carry > tot ? carry : tot;
  }
}

}  // namespace bce
