// wave_walk.h -- what a wave that walks a backward-search tree needs besides the step: the rank on the context's granules, the
// wave-uniform reads, and the rows of 64 intervals handed out in the order of the lanes.  Device only; kd_near.hip's helpers, moved
// here when kd_classes.hip came to walk its trees the same way (the code unchanged; WAVE_SERIAL was kd_near.hip's NEAR_SERIAL).
#pragma once
#include "common.h"
#include "fm_step.h"
#include "scan_util.h"

namespace bce {

constexpr uint32_t WAVE_SERIAL = 8;          // rows of an interval that its own lane reads

struct Zeros8 { uint32_t v[8]; };

// rank2 of fm_step on the context's granules: both loads of a level go out before either rank (count_kernel's lambda)
struct PlaneRank {
  const Granule *gran;
  uint32_t ngran;
  __device__ __forceinline__ void operator()(int j, uint32_t ia, uint32_t ib, uint32_t &ra, uint32_t &rb) const {
    const Granule *G = gran + (size_t)j * ngran;                    // (64-bit, as count_kernel)
    const uint32_t ga = div96(ia), gb = div96(ib);
    const Granule qa = G[ga], qb = G[gb];
    ra = granule_rank1(qa, ia - ga * 96u);
    rb = granule_rank1(qb, ib - gb * 96u);
  }
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int l) { return (uint32_t)__shfl((int)v, l); }
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// All 64 lanes together: lane l brings the rows [lo, lo + rows).  f(o, row) once for every row of every lane, o = its index in
// the order of the lanes.  Returns the rows of all lanes (below 2^31: the intervals of one pattern are disjoint).
template <class F>
__device__ __forceinline__ uint32_t wave_rows(uint32_t lo, uint32_t rows, uint32_t lane, F &&f) {
  const uint32_t incl = wave_incl_sum(rows);
  const uint32_t total = from_lane(incl, 63);
  if (total == 0) return 0;
  const uint32_t off = incl - rows;
  const bool wide = rows > WAVE_SERIAL;
  if (!wide) for (uint32_t i = 0; i < rows; ++i) f(off + i, lo + i);
  for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    const uint32_t L = from_lane(lo, l), S = from_lane(rows, l), O = from_lane(off, l);
    for (uint32_t i = lane; i < S; i += 64u) f(O + i, L + i);
  }
  return total;
}

}  // namespace bce
