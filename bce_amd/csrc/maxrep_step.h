// maxrep_step.h -- the per-element rules of bce_hip_maximal_repeats (kd_maxrep.hip): what one row of the LCP array decides about the
// LCP interval it lies in, the weight a maximal repeat is ordered by, and the host's share of the selection: which repeats can still
// be among the `limit` heaviest, judged from the 64 counters the histogram pass brings back.  Shared with tests/maxrep_emul.cpp,
// which runs the same lines under AddressSanitizer with blocks of 4 and 8 rows, the way lpf_step.h and top_step.h are shared.
//
// vals[0, n) is the capped LCP array (vals[0] == 0), D[r] the number of rows 1 .. r whose preceding byte differs from the row's
// above.  Row r >= 1 with l = vals[r] >= 1 lies in the interval [p, q): p the nearest row above with vals[p] < l, q the nearest row
// below with vals[q] < l, or n.  Many rows may carry l inside one interval; exactly one of them -- the lowest -- finds p as the
// nearest row above with a value <= l, and that row REPRESENTS the interval.  The first search therefore runs with the bound
// l + 1 and costs the other rows one load.
#pragma once
#include <stdint.h>

#include "bce_core.h"
#include "lpf_step.h"

namespace bce {

constexpr int kMxrBins = 64;
constexpr uint32_t kMxrByLen = 0, kMxrByCount = 1, kMxrByGain = 2;   // BCE_HIP_MAXREP_BY_*

// The weight of a repeat of `len` bytes that occurs `count` >= 2 times: always >= 1, below 2^44 for len <= 4096 and count < 2^31.
BCE_HD uint64_t mxr_weight(uint32_t order, uint32_t len, uint32_t count) {
  if (order == kMxrByLen) return ((uint64_t)len << 31) | count;
  if (order == kMxrByCount) return ((uint64_t)count << 13) | len;
  return (uint64_t)len * (count - 1u);
}
// ... and the count back from the weight and the length
BCE_HD uint32_t mxr_count_of(uint32_t order, uint64_t w, uint32_t len) {
  if (order == kMxrByLen) return (uint32_t)(w & 0x7FFFFFFFu);
  if (order == kMxrByCount) return (uint32_t)(w >> 13);
  return (uint32_t)(w / len) + 1u;
}

// floor(log2 w), w >= 1
BCE_HD uint32_t mxr_bin(uint64_t w) { return 63u - (uint32_t)__builtin_clzll(w); }

// Row i of block b (global row r = b * B + i) against the block's tree t[1, 2B) (leaves included) and, for answers outside the
// block, the top tree and the blocks' trees in global memory.  Returns the weight of the maximal repeat the row represents and its
// first row through *first, or 0: the row represents no interval, or one that is not left-maximal or shorter than min_len.
BCE_HD uint64_t mxr_row(const uint32_t *t, uint32_t B, uint32_t i, uint32_t b, const uint32_t *top, uint32_t NB, const uint32_t *inner,
                        const uint32_t *vals, uint32_t n, const uint32_t *D, uint32_t min_len, uint32_t order, uint32_t *first) {
  const uint32_t base = b * B, l = t[B + i];
  if (base + i == 0u || l == 0u || l == 0xFFFFFFFFu) return 0;         // (row 0 names no interval; l + 1 must not wrap)
  uint32_t p = nsv_tree_prev(t, B, i, l + 1u), pv;
  if (p != NSV_NONE) { pv = t[B + p]; p += base; }
  else {
    p = nsv_far_prev(top, NB, inner, vals, n, B, b, l + 1u);
    if (p == NSV_NONE) return 0;                                       // (only where vals[0] != 0: not an LCP array)
    pv = vals[p];
  }
  if (pv == l) return 0;                                               // a row above carries l inside the same interval: it represents it
  uint32_t q = nsv_tree_next(t, B, i, l);
  q = q != NSV_NONE ? base + q : nsv_far_next(top, NB, inner, vals, n, B, b, l);
  if (q == NSV_NONE) q = n;
  if (D[q - 1u] == D[p]) return 0;                                     // one preceding byte throughout: extends to the left
  if (l < min_len) return 0;
  *first = p;
  return mxr_weight(order, l, q - p);
}

// ---- the selection (top_step.h's rule with 64 bins of a 64-bit weight) ----
BCE_HD uint64_t mxr_total(const uint64_t H[kMxrBins]) {
  uint64_t d = 0;
  for (int b = 0; b < kMxrBins; ++b) d += H[b];
  return d;
}
// The threshold bin t for a list of want = min(limit, total) >= 1 repeats: the LARGEST bin with sum_{b >= t} H[b] >= want.  The
// repeats of weight >= 2^t are the candidates, *candidates of them; at least `want` of them exist, so the want-th heaviest is among
// them and so is everything in front of it, and equal weights share a bin, so ties are whole.  *top: the largest bin in use.
BCE_HD int mxr_threshold(const uint64_t H[kMxrBins], uint64_t want, uint64_t *candidates, int *top) {
  int hi = 0;
  for (int b = 0; b < kMxrBins; ++b) if (H[b]) hi = b;
  uint64_t above = 0;
  int t = 0;
  for (int b = kMxrBins - 1; b >= 0; --b) {
    above += H[b];
    if (above >= want) { t = b; break; }
  }
  if (above < want) above = mxr_total(H);
  *candidates = above;
  *top = hi;
  return t;
}
// The sort key of a candidate: the complement of its weight within the largest bin in use, so ascending keys are descending weights.
BCE_HD uint64_t mxr_key_max(int top) { return top >= 63 ? ~0ull : (2ull << top) - 1ull; }
BCE_HD uint64_t mxr_key(int top, uint64_t w) { return mxr_key_max(top) - w; }
// the bits of the largest key there can be, mxr_key(top, 2^t): what the sorter looks at (0: one weight only)
BCE_HD uint32_t mxr_key_bits(int t, int top) {
  const uint64_t m = mxr_key_max(top) - (1ull << t);
  return m ? 64u - (uint32_t)__builtin_clzll(m) : 0u;
}

}  // namespace bce
