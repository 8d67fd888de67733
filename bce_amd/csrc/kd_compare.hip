// kd_compare.hip -- first differing byte of two device buffers (bce_hip_verify_device / _host, `bce -t`; alone: bce_hip_compare_device).
//
// The decoder leaves the text in HBM (kd_decode.hip); "does this archive decode to these bytes" is then one pass over
// 2 m bytes that never leaves the device.  Memory-bound: every byte of both buffers is read once, nothing is written but
// one 64-bit result word.
//   - Neither pointer needs any alignment (the original may be a slice of a tensor).  `a` decides the split: its first
//     (-a mod 16) bytes and the last (m - head) mod 16 bytes are compared bytewise by workgroup 0, the 16-byte units in
//     between by a grid-stride loop, four units per lane and pass (eight loads in flight per lane).  `b` is read at the
//     same offsets whatever its alignment (global memory takes unaligned 16-byte vector loads; the load is a memcpy in
//     the source, no pointer of a stricter type is ever formed).
//   - A 16-byte pair differs where its xor is not zero: the first non-zero word, and its lowest set bit / 8 (little endian).
//   - A wave that has found a difference stops -- its later units lie higher --, and a workgroup stops when its next chunk
//     lies above the result word, which only ever holds the index of a real difference: whatever is skipped is above one.
//     So the word ends as the exact minimum.  The lanes' minima are reduced by shuffles, the waves' through LDS, and a
//     workgroup that found something issues ONE atomicMin.
#include "common.h"

namespace bce {

namespace {

constexpr int CMP_T = 256;                   // lanes per workgroup (4 waves)
constexpr int CMP_U = 4;                     // 16-byte units per lane and pass
constexpr uint64_t kNoDiff = ~0ull;

struct Vec16 { uint32_t w[4]; };

__device__ inline Vec16 load16(const uint8_t *p) {
  Vec16 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// offset of the first differing byte of a 16-byte pair, 16 if there is none
__device__ inline uint32_t first_diff16(const Vec16 &x, const Vec16 &y) {
  #pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t d = x.w[k] ^ y.w[k];
    if (d) return 4u * k + ((uint32_t)__ffs(d) - 1u) / 8u;
  }
  return 16u;
}

// a + head is 16-byte aligned; units 16-byte pairs follow it, then tail < 16 bytes: head + 16 units + tail = the m bytes compared
__global__ __launch_bounds__(CMP_T) void compare_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t head,
                                                        uint64_t units, uint32_t tail, unsigned long long *result) {
  __shared__ unsigned long long wave_min[CMP_T / 64];
  const uint32_t tid = threadIdx.x;
  uint64_t mine = kNoDiff, ends = kNoDiff;
  if (blockIdx.x == 0) {                                          // the two ragged ends, a byte per lane (kept apart from `mine`: the tail lies above every unit)
    const uint64_t tail_at = head + units * 16;
    if (tid < head) { if (a[tid] != b[tid]) ends = tid; }
    else if (tid >= 16 && tid - 16 < tail) { if (a[tail_at + tid - 16] != b[tail_at + tid - 16]) ends = tail_at + tid - 16; }
  }
  const uint8_t *av = a + head, *bv = b + head;
  const uint64_t chunk = (uint64_t)CMP_T * CMP_U;
  for (uint64_t base = blockIdx.x * chunk; base < units; base += gridDim.x * chunk) {
    if (head + base * 16 > __atomic_load_n(result, __ATOMIC_RELAXED)) break;   // (block-uniform: everything from here on lies above a difference)
    Vec16 x[CMP_U], y[CMP_U];
    #pragma unroll
    for (int k = 0; k < CMP_U; ++k) {
      const uint64_t u = base + (uint64_t)k * CMP_T + tid;
      if (u < units) { x[k] = load16(av + u * 16); y[k] = load16(bv + u * 16); }
      else { x[k] = Vec16{{0, 0, 0, 0}}; y[k] = x[k]; }
    }
    #pragma unroll
    for (int k = CMP_U - 1; k >= 0; --k) {                        // (downwards: the lowest unit's answer is the one that stays)
      const uint32_t f = first_diff16(x[k], y[k]);
      if (f < 16) mine = head + (base + (uint64_t)k * CMP_T + tid) * 16 + f;
    }
    if (__any(mine != kNoDiff)) break;                            // (wave-uniform: this wave's later units lie above it)
  }
  mine = ends < mine ? ends : mine;
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor((unsigned long long)mine, d, 64);
    mine = o < mine ? o : mine;
  }
  if ((tid & 63) == 0) wave_min[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    unsigned long long m = wave_min[0];
    for (int w = 1; w < CMP_T / 64; ++w) m = wave_min[w] < m ? wave_min[w] : m;
    if (m != kNoDiff) atomicMin(result, m);
  }
}

}  // namespace

// *first_diff = the smallest i < m with a[i] != b[i], UINT64_MAX if there is none.  a, b: device memory of the context's device, any
// alignment.  Queued on the context's stream behind whatever wrote the two buffers; returns when the answer is on the host.
int kd_compare(bce_hip_ctx *c, const uint8_t *a, const uint8_t *b, uint64_t m, uint64_t *first_diff) {
  *first_diff = kNoDiff;
  if (m == 0) return BCE_HIP_OK;
  // (the result word lies in a buffer of its own: a call between two stages of a compression or between two model flushes --
  //  bce_hip_compare_device is valid there -- must not touch the words other stages keep in c->stat, K4's model counters among them)
  BCE_TRY(ensure(c, c->cmp_res, 8));
  unsigned long long *d_res = c->cmp_res.as<unsigned long long>();
  BCE_HIP_TRY(c, hipMemsetAsync(d_res, 0xFF, 8, c->stream));
  const uint32_t head = (uint32_t)std::min<uint64_t>(m, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(a) & 15u)) & 15u);
  const uint64_t units = (m - head) / 16;
  const uint32_t tail = (uint32_t)(m - head - units * 16);
  const uint64_t chunk = (uint64_t)CMP_T * CMP_U, chunks = (units + chunk - 1) / chunk;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunks, 2048));
  hipLaunchKernelGGL(compare_kernel, dim3(grid), dim3(CMP_T), 0, c->stream, a, b, head, units, tail, d_res);
  BCE_HIP_TRY(c, hipGetLastError());
  uint64_t res = kNoDiff;
  BCE_TRY(read_back(c, &res, d_res, 8));
  BCE_HIP_TRY(c, hipGetLastError());
  *first_diff = res;
  return BCE_HIP_OK;
}

}  // namespace bce
