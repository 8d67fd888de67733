// parse_step.h -- the per-element rules of the delta parse and of the patch that undoes it: what kd_parse.hip decides per query
// position and per op, shared with the host (tests/parse_emul.cpp runs the same lines under AddressSanitizer with blocks of 4 and 8
// positions), the way fm_step.h and lcp_step.h are shared.
//
// The parse walks the query from its last byte to its first along the chain e -> e - jump(e): a copy of len[e] bytes where the
// longest match that ends at e has min_len bytes or more, else one literal byte.  The chain's nodes carry a flag byte; an op is
// a copy, or a maximal run of literal nodes, named by its LAST position (its head).  Everything here is a function of one
// element and its right neighbour, so blocks of positions can be judged side by side.
#pragma once
#include <stdint.h>

#include "bce_core.h"

namespace bce {

constexpr uint32_t PARSE_LITERAL = 0xFFFFFFFFu;   // bce_hip_op::src of a literal run (BCE_HIP_OP_LITERAL)
constexpr uint8_t PARSE_NONE = 0, PARSE_LIT = 1, PARSE_COPY = 2;   // the flag byte of a position: no chain node, a literal byte, the last byte of a copy
constexpr uint32_t PARSE_NO_ENTRY = 0xFFFFFFFFu;  // entry[b] of a block the chain never enters
constexpr uint64_t PATCH_MAX_TOTAL = 0x7FFFFFFFull;   // a patched result has fewer than 2^31 bytes

// how far the chain moves to the left from a node at a position whose longest match has `len` bytes (len <= position + 1)
BCE_HD uint32_t parse_jump(uint32_t len, uint32_t min_len) { return len >= min_len ? len : 1u; }
BCE_HD uint8_t parse_kind(uint32_t len, uint32_t min_len) { return len >= min_len ? PARSE_COPY : PARSE_LIT; }

// The first hop of the exit search of position e in the block that begins at `base` (base <= e): the chain's next node plus one,
// so that "the chain ends in front of position 0" is the word 0.  A word <= base is final: the node lies below the block.
// A jump that would start in front of the query (no length of a search does) ends the chain like one that starts at position 0.
BCE_HD uint32_t parse_next1(uint32_t e, uint32_t jump) { return jump <= e ? e + 1u - jump : 0u; }
BCE_HD bool parse_left_block(uint32_t next1, uint32_t base) { return next1 <= base; }

// An op head: a copy's last byte, or a literal node whose right neighbour is no literal node (`right`: its flag, PARSE_NONE past
// the end of the query).  Literal nodes that are neighbours belong to one run: the chain goes from a literal node to the position
// in front of it.
BCE_HD bool parse_is_head(uint8_t flag, uint8_t right) { return flag == PARSE_COPY || (flag == PARSE_LIT && right != PARSE_LIT); }

// ---- the patch ----
// What is wrong with one op by itself, as bits (0: nothing): a length of zero; a copy that does not lie inside the n bytes of the text.
constexpr uint32_t PATCH_BAD_ZERO = 1u, PATCH_BAD_RANGE = 2u;
BCE_HD uint32_t patch_op_bad(uint32_t len, uint32_t src, uint32_t n) {
  if (len == 0u) return PATCH_BAD_ZERO;
  if (src != PARSE_LITERAL && (uint64_t)src + len > n) return PATCH_BAD_RANGE;
  return 0u;
}
BCE_HD uint64_t patch_lit_len(uint32_t len, uint32_t src) { return src == PARSE_LITERAL ? len : 0u; }

// What is wrong with a whole list, from its sums (after no single op was): the words of the refusal, or nullptr.
inline const char *patch_list_bad(uint32_t op_bits, uint64_t total, uint64_t lit_total, uint64_t nlits) {
  if (op_bits & PATCH_BAD_ZERO) return "patch: an op of length 0";
  if (op_bits & PATCH_BAD_RANGE) return "patch: a copy runs past the end of the text";
  if (lit_total != nlits) return "patch: the literal runs do not add up to the literal bytes given";
  if (total > PATCH_MAX_TOTAL) return "patch: a result of 2^31 bytes or more";
  return nullptr;
}

// The op that holds output byte o: the largest k < nops with off[k] <= o (off: the ops' exclusive output offsets, ascending, off[0] == 0).
BCE_HD uint32_t patch_op_of(const uint32_t *off, uint32_t nops, uint32_t o) {
  uint32_t lo = 0, hi = nops;                                           // off[lo] <= o < off[hi] (off[nops] = the total)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= o) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace bce
