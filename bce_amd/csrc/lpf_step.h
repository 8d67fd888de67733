// lpf_step.h -- the per-element rules of the self-index queries: all nearest smaller values over the suffix array, the longest
// previous factor of a text position, and the mirror that turns the self-parse's left-to-right chain into kd_parse's right-to-left
// one.  What kd_self.hip decides per row, shared with the host (tests/lpf_emul.cpp runs the same lines under AddressSanitizer
// with blocks of 4 and 8 rows), the way lcp_step.h and parse_step.h are shared.
//
// The structure is an implicit binary min-tree in two storeys.  Every block of B rows (B a power of two) has a tree of its own:
// node 1 is the block's minimum, node k the minimum of nodes 2k and 2k + 1, the leaves B .. 2B - 1 are the rows (NSV_PAD beyond
// the last row).  The blocks' minima are the leaves of one more tree of the same shape.  A search climbs from a leaf until a
// sibling on the wanted side holds a smaller value and descends into it: at most log2(L) loads up and log2(L) down in a tree of L
// leaves, whatever the values are.
#pragma once
#include <stdint.h>

#include "bce_core.h"
#include "lcp_step.h"

namespace bce {

constexpr uint32_t NSV_NONE = 0xFFFFFFFFu;   // psv / nsv of a row without a smaller value on that side; src of a position without a factor
constexpr uint32_t NSV_PAD = 0xFFFFFFFFu;    // a leaf beyond the rows: smaller than nothing

// strictly: equal values are never "smaller"
BCE_HD bool nsv_less(uint32_t a, uint32_t v) { return a < v; }
BCE_HD uint32_t nsv_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// t[1, 2L): a tree of L leaves, L a power of two, with its leaves in the same array.  The nearest leaf in front of leaf p (behind
// it) whose value is smaller than v, or NSV_NONE.
BCE_HD uint32_t nsv_tree_prev(const uint32_t *t, uint32_t L, uint32_t p, uint32_t v) {
  for (uint32_t k = L + p; k > 1u; k >>= 1) {
    if (!(k & 1u) || !nsv_less(t[k - 1u], v)) continue;               // a right child whose left sibling holds a smaller value
    k -= 1u;
    while (k < L) { k = 2u * k + 1u; if (!nsv_less(t[k], v)) k -= 1u; }   // the right half wherever it has one
    return k - L;
  }
  return NSV_NONE;
}
BCE_HD uint32_t nsv_tree_next(const uint32_t *t, uint32_t L, uint32_t p, uint32_t v) {
  for (uint32_t k = L + p; k > 1u; k >>= 1) {
    if ((k & 1u) || !nsv_less(t[k + 1u], v)) continue;
    k += 1u;
    while (k < L) { k = 2u * k; if (!nsv_less(t[k], v)) k += 1u; }
    return k - L;
  }
  return NSV_NONE;
}

// A block's tree as it lies in global memory: inner[1, B) and the rows themselves as leaves, `cnt` of them (1 <= cnt <= B).
BCE_HD uint32_t nsv_block_node(const uint32_t *inner, const uint32_t *leaf, uint32_t B, uint32_t cnt, uint32_t k) {
  if (k < B) return inner[k];
  return k - B < cnt ? leaf[k - B] : NSV_PAD;
}
// The last (first) row of a block whose minimum is smaller than v that is smaller than v itself: log2(B) loads from the root down.
BCE_HD uint32_t nsv_block_last(const uint32_t *inner, const uint32_t *leaf, uint32_t B, uint32_t cnt, uint32_t v) {
  uint32_t k = 1u;
  while (k < B) { k = 2u * k + 1u; if (!nsv_less(nsv_block_node(inner, leaf, B, cnt, k), v)) k -= 1u; }
  return k - B;
}
BCE_HD uint32_t nsv_block_first(const uint32_t *inner, const uint32_t *leaf, uint32_t B, uint32_t cnt, uint32_t v) {
  uint32_t k = 1u;
  while (k < B) { k = 2u * k; if (!nsv_less(nsv_block_node(inner, leaf, B, cnt, k), v)) k += 1u; }
  return k - B;
}

// The answer of a row whose own block holds none: the nearest block in front of block b (behind it) with a smaller minimum, from
// the tree `top` over the NB >= blocks minima, then the row inside it.  vals[0, n) are the rows, inner the blocks' trees, B words each.
BCE_HD uint32_t nsv_far_prev(const uint32_t *top, uint32_t NB, const uint32_t *inner, const uint32_t *vals, uint32_t n, uint32_t B, uint32_t b,
                             uint32_t v) {
  const uint32_t f = nsv_tree_prev(top, NB, b, v);
  if (f == NSV_NONE) return NSV_NONE;
  const uint32_t base = f * B;
  return base + nsv_block_last(inner + base, vals + base, B, n - base < B ? n - base : B, v);
}
BCE_HD uint32_t nsv_far_next(const uint32_t *top, uint32_t NB, const uint32_t *inner, const uint32_t *vals, uint32_t n, uint32_t B, uint32_t b,
                             uint32_t v) {
  const uint32_t f = nsv_tree_next(top, NB, b, v);
  if (f == NSV_NONE) return NSV_NONE;
  const uint32_t base = f * B;
  return base + nsv_block_first(inner + base, vals + base, B, n - base < B ? n - base : B, v);
}

// ---- the longest previous factor ----
// The compare's bound for text position i: with it neither i + l nor j + l (j < i) reaches n, so rot_lcp never wraps.
BCE_HD uint32_t lpf_cap(uint32_t n, uint32_t i, uint32_t max_len) { return n - i < max_len ? n - i : max_len; }

// lpf[i] and, through *src, src[i], from the text positions a and b of the nearest rows above and below i's row that start earlier
// in the text (NSV_NONE: there is none).  The longer one wins, the upper one where both are as long.
BCE_HD uint32_t lpf_pick(const uint8_t *text, uint32_t n, uint32_t i, uint32_t a, uint32_t b, uint32_t max_len, uint32_t *src) {
  const uint32_t cap = lpf_cap(n, i, max_len);
  const uint32_t la = a != NSV_NONE ? rot_lcp(text, n, i, a, cap) : 0u;
  const uint32_t lb = b != NSV_NONE ? rot_lcp(text, n, i, b, cap) : 0u;
  const uint32_t l = la >= lb ? la : lb;
  *src = l == 0u ? NSV_NONE : la >= lb ? a : b;
  return l;
}

// ---- the chain ----
// The self-parse walks s = 0, s += jump(lpf[s]) ...; kd_parse walks e = q - 1, e -= jump(len[e]) ...  They are the same walk once
// position s is written at n - 1 - s: a copy of l bytes that BEGINS at s ends at its mirror.  Ops and literal bytes come out in
// mirrored order and are turned round once, element k against element count - 1 - k.
BCE_HD uint32_t self_mirror(uint32_t n, uint32_t i) { return n - 1u - i; }

}  // namespace bce
