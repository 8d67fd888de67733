// top_step.h -- the host's share of bce_hip_top_kgrams (kd_lcp.hip): which classes of one k can still be among the `limit` largest,
// judged from the 32 counters the histogram pass brings back, and the way `bce -gf` prints a k-gram's bytes.  Shared with
// tests/top_emul.cpp, which runs the same lines under AddressSanitizer, the way lcp_step.h and parse_step.h are shared.
//
// H[b], b < 32: the classes whose size N has floor(log2 N) = b (N >= 1, so every class is in exactly one bin; N < 2^31).
#pragma once
#include <stdint.h>

#include "bce_core.h"

namespace bce {

constexpr int kTopBins = 32;

// floor(log2 size), size >= 1
BCE_HD uint32_t top_bin(uint32_t size) { return 31u - (uint32_t)__builtin_clz(size); }

BCE_HD uint64_t top_classes(const uint64_t H[kTopBins]) {
  uint64_t d = 0;
  for (int b = 0; b < kTopBins; ++b) d += H[b];
  return d;
}

// The threshold bin t for a list of want = min(limit, distinct) >= 1 classes: the LARGEST bin with sum_{b >= t} H[b] >= want.
// The classes of size >= 2^t are the candidates.  Nothing of the answer is lost: at least `want` classes have a size of 2^t or
// more, so the want-th largest has, and so has every class in front of it; a class of equal size is in the same bin, so ties are
// whole.  *candidates = that sum, exact, so the candidate buffers are sized by it and never by n; *top = the largest bin that is
// not empty.  Worst case: every class in one bin (all singletons, or one class) -- then t is that bin and every class a candidate.
BCE_HD int top_threshold(const uint64_t H[kTopBins], uint64_t want, uint64_t *candidates, int *top) {
  int hi = 0;
  for (int b = 0; b < kTopBins; ++b) if (H[b]) hi = b;
  uint64_t above = 0;
  int t = 0;
  for (int b = kTopBins - 1; b >= 0; --b) {
    above += H[b];
    if (above >= want) { t = b; break; }
  }
  if (above < want) above = top_classes(H);                           // (want > distinct: the caller's mistake; everything is a candidate)
  *candidates = above;
  *top = hi;
  return t;
}

// The sort key of a candidate of `size` in [2^t, 2^(top + 1)): ascending keys are descending sizes.
BCE_HD uint32_t top_key_max(int top) { return top >= 31 ? 0xFFFFFFFFu : (1u << (top + 1)) - 1u; }
BCE_HD uint32_t top_key(int top, uint32_t size) { return top_key_max(top) - size; }
// the bits of the largest key there can be, top_key(top, 2^t): what the sorter has to look at (0: one size only, nothing to sort)
BCE_HD uint32_t top_key_bits(int t, int top) {
  const uint32_t m = top_key_max(top) - (1u << t);
  return m ? 32u - (uint32_t)__builtin_clz(m) : 0u;
}

// One byte of a k-gram as `bce -gf` prints it: printable ASCII other than backslash and space as it is, everything else as \xHH
// (two upper-case hex digits).  out: room for 5 chars, 0-terminated; returns the characters written (1 or 4).
BCE_HD int top_escape(uint8_t byte, char out[5]) {
  if (byte > 0x20 && byte < 0x7F && byte != '\\') { out[0] = (char)byte; out[1] = 0; return 1; }
  const char *hex = "0123456789ABCDEF";
  out[0] = '\\'; out[1] = 'x'; out[2] = hex[byte >> 4]; out[3] = hex[byte & 15]; out[4] = 0;
  return 4;
}

}  // namespace bce
