// fm_step.h -- backward search on the K2 planes: the step kd_count.hip runs per pattern byte, shared with the host
// (tests/count_emul.cpp runs the same lines on planes it builds naively), the way bce_cost.h and bce_core.h are shared.
//
// K2 partitions the BWT stably by bit 0, then bit 1, ... bit 7, zeros first (k2_planes.hip): an LSD radix sort, so after the
// eight levels the bytes stand sorted by value, equal bytes in BWT order.  Following a position i in [0, n] down the levels for
// a byte c -- a one-bit goes to zeros[j] + rank1_j(i), a zero-bit to i - rank1_j(i) -- therefore ends at C[c] + rank_c(BWT, i),
// the last-to-first mapping, with no histogram and no C[] array.  Both ends of an interval take the step together: their two
// ranks of a level are independent (one fetch), the levels are a dependent chain.
#pragma once
#include "bce_core.h"

namespace bce {

// (lo, hi) -> (LF(c, lo), LF(c, hi)).  rank2(j, a, b, ra, rb): ra = rank1_j(a), rb = rank1_j(b) on plane j, 0 <= a <= b <= n.
template <class Rank2>
BCE_HD void fm_step(uint32_t c, const uint32_t zeros[8], uint32_t &lo, uint32_t &hi, Rank2 &&rank2) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 8; ++j) {
    uint32_t rl, rh;
    rank2(j, lo, hi, rl, rh);
    const bool one = (c >> j) & 1u;
    lo = one ? zeros[j] + rl : lo - rl;
    hi = one ? zeros[j] + rh : hi - rh;
  }
}

// Occurrences of pat[0, m) in the circular text of n bytes whose planes rank2 serves: the i in [0, n) with
// pat[k] == T[(i + k) mod n] for all k.  Any m: the empty pattern occurs n times, m > n wraps around.
template <class Rank2>
BCE_HD uint32_t fm_count(const uint8_t *pat, uint64_t m, uint32_t n, const uint32_t zeros[8], Rank2 &&rank2) {
  uint32_t lo = 0, hi = n;
  for (uint64_t k = m; k > 0 && lo < hi; --k) fm_step(pat[k - 1], zeros, lo, hi, rank2);
  return hi - lo;
}

}  // namespace bce
