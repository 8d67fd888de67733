// lcp_step.h -- the longest common prefix of two rotations of the circular text: the compare kd_lcp.hip runs per row of the
// sorted rotations, shared with the host (tests/lcp_emul.cpp runs the same lines under AddressSanitizer on a text in a heap block
// of exactly n bytes), the way fm_step.h, bce_cost.h and bce_core.h are shared.
//
// Rotation a of the text T of n bytes is T[(a + j) mod n], j = 0, 1, ...  It has no end, so the common prefix of two rotations is
// not capped at n: two equal rotations of a periodic text agree for ever and give max_len, the work bound of the compare.
#pragma once
#include <stdint.h>

#include "bce_core.h"

namespace bce {

// eight bytes from p, any alignment, the byte at p in the low bits (host and device are little-endian)
BCE_HD uint64_t lcp_load8(const uint8_t *p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// The largest l <= max_len with T[(a + j) mod n] == T[(b + j) mod n] for all j < l; a, b < n, n >= 1.
// Eight bytes at a time while neither rotation is within eight bytes of the text's end -- the first difference is the lowest set
// bit of the words' xor -- and byte by byte across the seam, where a position wraps to 0.  With n < 8 the seam is inside every
// word and all steps are single bytes; with n far below max_len the compare goes round the text many times.  A word that ends
// past max_len is still compared whole (the result is cut afterwards): what is read is bounded by the text, not by max_len, and
// nothing at or beyond text + n is ever read.
BCE_HD uint32_t rot_lcp(const uint8_t *text, uint32_t n, uint32_t a, uint32_t b, uint32_t max_len) {
  uint32_t l = 0;
  while (l < max_len) {
    if (n - a >= 8u && n - b >= 8u) {
      const uint64_t x = lcp_load8(text + a) ^ lcp_load8(text + b);
      if (x) { l += (uint32_t)__builtin_ctzll(x) >> 3; break; }
      l += 8u; a += 8u; b += 8u;
      if (a == n) a = 0;
      if (b == n) b = 0;
    } else {
      if (text[a] != text[b]) break;
      l += 1u;
      if (++a == n) a = 0;
      if (++b == n) b = 0;
    }
  }
  return l < max_len ? l : max_len;
}

}  // namespace bce
