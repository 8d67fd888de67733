// fm_step.h -- backward search on the K2 planes: the step kd_count.hip, kd_locate.hip and kd_match.hip run per byte, and the row
// arithmetic of a located batch, shared with the host (tests/count_emul.cpp and tests/locate_emul.cpp run the same lines on planes
// they build naively), the way bce_cost.h and bce_core.h are shared.
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

// The rows [lo, hi) of the sorted rotations that start with pat[0, m), in the circular text of n bytes whose planes rank2
// serves.  Any m: the empty pattern owns all n rows, m > n wraps around.  The next byte is fetched before the current byte's
// eight levels, off their chain.  An empty interval stops the search; lo is then whatever the last step left.
template <class Rank2>
BCE_HD void fm_range(const uint8_t *pat, uint64_t m, uint32_t n, const uint32_t zeros[8], uint32_t &lo, uint32_t &hi, Rank2 &&rank2) {
  lo = 0; hi = n;
  uint32_t c = m ? pat[m - 1] : 0u;
  for (uint64_t k = m; k > 0 && lo < hi; --k) {
    const uint32_t next = k > 1 ? pat[k - 2] : 0u;
    fm_step(c, zeros, lo, hi, rank2);
    c = next;
  }
}

// Occurrences of pat[0, m) in that text: the i in [0, n) with pat[k] == T[(i + k) mod n] for all k.
template <class Rank2>
BCE_HD uint32_t fm_count(const uint8_t *pat, uint64_t m, uint32_t n, const uint32_t zeros[8], Rank2 &&rank2) {
  uint32_t lo, hi;
  fm_range(pat, m, n, zeros, lo, hi, rank2);
  return hi - lo;
}

// ---- locating (kd_locate.hip): the occurrences are the suffix array's entries sa[lo, hi) ---------------------------------------
// A batch's rows stand pattern after pattern: pattern p owns rows [start[p], start[p + 1]), start[0] = 0, non-decreasing,
// npat + 1 words.  The pattern that owns row r < start[npat]: the last p with start[p] <= r (empty patterns between are skipped).
BCE_HD uint32_t fm_row_pattern(const uint64_t *start, uint32_t npat, uint64_t r) {
  uint32_t a = 0, b = npat;                          // start[a] <= r < start[b]
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (start[mid] <= r) a = mid; else b = mid;
  }
  return a;
}

// Does the cyclic hit at pos < n lie inside the text, pos + m <= n?  (A pattern longer than the text never does.)
BCE_HD bool fm_linear_hit(uint32_t pos, uint64_t m, uint32_t n) { return m <= n && pos <= n - (uint32_t)m; }

// ---- matching statistics (kd_match.hip): the longest string that ends at q[i] and occurs in the text ------------------------------
// len = the largest l <= min(L, i + 1) for which q[i - l + 1 .. i] occurs, found by extending to the left one byte at a time from
// the empty match: the strings that end at i are suffixes of one another, so the first length that fails ends the search.  row = a
// row of the sorted rotations whose rotation starts with that match (0 when len == 0): the caller reads the position from it.
// The byte to the left is fetched before the current byte's eight levels, off their chain, as in fm_range.
//   Cyclic: "occurs" as in fm_count; the search goes on while the interval [lo, hi) is not empty, and row = lo.
//   Linear: an occurrence must start at a p with p + l <= n.  At length l only the l - 1 rotations that start at n - l + 1 .. n - 1
//     run across the end of the text, so an interval of l rows or more holds a row inside the text and nothing is read.  A
//     narrower one has fewer than l entries of the suffix array, neighbouring words: sa(r) reads them in turn until one passes
//     fm_linear_hit -- the witness; if none does, the previous length stands.  An interval of one row whose start w is known needs
//     no read: the step leaves the rotation that starts one byte earlier, at w - 1 (w == 0: it would start at the text's last
//     byte and run across the end).  l > n never matches.  With want_row, a final length whose witness is not known (its interval
//     was wide) looks for it among the interval's first len rows, where there must be one.
// sa(r) is called with lo <= r < hi <= n only, and never for a text of one byte (which has no array: its rotation starts at 0).
template <bool Linear, class Rank2, class Sa>
BCE_HD void fm_match_end(const uint8_t *q, uint64_t i, uint32_t L, uint32_t n, const uint32_t zeros[8], bool want_row, uint32_t &len,
                         uint32_t &row, Rank2 &&rank2, Sa &&sa) {
  uint32_t maxl = i + 1 < (uint64_t)L ? (uint32_t)(i + 1) : L;
  if (Linear && maxl > n) maxl = n;
  uint32_t lo = 0, hi = n;                             // the rotations that start with the match of len bytes
  uint32_t w = 0;                                      // Linear, known: the rotation of `row` starts at w, w + len <= n
  bool known = false;
  len = 0; row = 0;
  uint32_t c = q[i];
  while (len < maxl) {
    const uint32_t l = len + 1;
    const uint32_t next = l < maxl ? q[i - l] : 0u;
    const bool single = Linear && known && hi - lo == 1u;
    if (single && w == 0) break;
    uint32_t a = lo, b = hi;
    fm_step(c, zeros, a, b, rank2);
    if (a >= b) break;
    if (Linear) {
      if (single) { w -= 1u; row = a; }
      else if (b - a >= l) known = false;
      else {
        uint32_t r = a, p = sa(r);
        while (!fm_linear_hit(p, l, n) && ++r < b) p = sa(r);
        if (r == b) break;
        known = true; w = p; row = r;
      }
    }
    lo = a; hi = b; len = l; c = next;
  }
  if (!Linear) row = lo;
  else if (!known) {
    row = lo;
    if (want_row && len) while (row + 1u < hi && !fm_linear_hit(sa(row), len, n)) ++row;
  }
}

}  // namespace bce
