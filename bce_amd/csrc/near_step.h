// near_step.h -- backward search that branches: the rows of the sorted rotations whose rotation starts within k mismatches of a
// pattern (kd_near.hip: bce_hip_count_near / _locate_near, `bce -gn` / `-gnl`), shared with the host (tests/near_emul.cpp runs the
// same lines on planes it builds naively), the way fm_step.h is shared.
//
// T: the circular text of n bytes, P: a pattern of m bytes, d(i) = #{ j < m : P[j] != T[(i + j) mod n] }.  Two different strings of
// one length own disjoint row intervals, so the i with d(i) <= k are the disjoint union of the intervals of the strings within k
// mismatches of P that occur: counts add, no position is found twice.  The search enumerates those strings from right to left.  A
// node is (the interval of the suffix chosen so far, the bytes still to the left, the mismatches so far):
//   - with budget left, every byte c != P[pos - 1] whose step from the node's interval is not empty opens a child with one more
//     mismatch (near_child), then the node itself takes the exact step and moves one byte to the left; an empty interval ends it;
//   - with the budget spent, the rest of the pattern is plain backward search from the node's interval (near_finish);
//   - pos == 0 with rows left: the interval is an answer, at the node's number of mismatches.
// The last byte is a position like any other: a pattern byte the text lacks ends the exact child, not the others.  m == 0: the
// root is the answer (all n rows, distance 0); k >= m needs no special case, every row is reached at its own distance.
#pragma once
#include "fm_step.h"

#define BCE_NEAR_MAX_K 2u                    // = BCE_HIP_NEAR_MAX_K (include/bce_hip.h)

namespace bce {

// The candidate step: the rows of [lo, hi) whose rotation is preceded by c, as an interval of their own.  False: there are none.
template <class Rank2>
BCE_HD bool near_child(uint32_t c, const uint32_t zeros[8], uint32_t lo, uint32_t hi, uint32_t &a, uint32_t &b, Rank2 &&rank2) {
  a = lo; b = hi;
  fm_step(c, zeros, a, b, rank2);
  return a < b;
}

// The exact finish: pat[0, pos) to the left of the interval [lo, hi), fm_range's loop from where a node stands.  An empty interval
// stops it; lo is then whatever the last step left.
template <class Rank2>
BCE_HD void near_finish(const uint8_t *pat, uint64_t pos, const uint32_t zeros[8], uint32_t &lo, uint32_t &hi, Rank2 &&rank2) {
  uint32_t c = pos ? pat[pos - 1] : 0u;
  for (uint64_t k = pos; k > 0 && lo < hi; --k) {
    const uint32_t next = k > 1 ? pat[k - 2] : 0u;
    fm_step(c, zeros, lo, hi, rank2);
    c = next;
  }
}

// The distance bookkeeping: per[d] += rows, d <= BCE_NEAR_MAX_K (a chain of compares, so that per[] can live in registers).
BCE_HD void near_tally(uint64_t per[BCE_NEAR_MAX_K + 1], uint32_t d, uint32_t rows) {
  static_assert(BCE_NEAR_MAX_K == 2u, "near_tally names every distance");
  per[0] += d == 0 ? rows : 0u;
  per[1] += d == 1 ? rows : 0u;
  per[2] += d == 2 ? rows : 0u;
}

// A node with budget left.  cand: the next byte to try at pos as a mismatch; 256: all tried, the exact step is next.
struct NearFrame {
  uint32_t lo, hi;
  uint64_t pos;
  uint32_t cand;
};

// The whole search by one thread: emit(lo, hi, d) for every answer, lo < hi, in the order of the walk.  At most k frames with
// budget are open at a time, and the node below them whose budget is spent: k + 1 frames, nothing grows with n or m.
// kd_near.hip walks the same tree with a wave: its lanes share a frame's candidates, the frames are these.
template <class Rank2, class Emit>
BCE_HD void near_search(const uint8_t *pat, uint64_t m, uint32_t n, uint32_t k, const uint32_t zeros[8], Rank2 &&rank2, Emit &&emit) {
  NearFrame f[BCE_NEAR_MAX_K + 1];
  int d = 0;                                 // the open frame; its mismatches
  f[0] = NearFrame{0u, n, m, 0u};
  while (d >= 0) {
    NearFrame &F = f[d];
    if (F.lo >= F.hi) { --d; continue; }
    if (F.pos == 0) { emit(F.lo, F.hi, (uint32_t)d); --d; continue; }
    if ((uint32_t)d == k) {
      near_finish(pat, F.pos, zeros, F.lo, F.hi, rank2);
      if (F.lo < F.hi) emit(F.lo, F.hi, (uint32_t)d);
      --d;
      continue;
    }
    const uint32_t own = pat[F.pos - 1];
    if (F.cand < 256u) {
      const uint32_t c = F.cand++;
      uint32_t a, b;
      if (c != own && near_child(c, zeros, F.lo, F.hi, a, b, rank2)) { f[d + 1] = NearFrame{a, b, F.pos - 1, 0u}; ++d; }
      continue;
    }
    fm_step(own, zeros, F.lo, F.hi, rank2);
    F.pos -= 1; F.cand = 0;
  }
}

}  // namespace bce
