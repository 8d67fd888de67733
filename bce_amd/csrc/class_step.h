// class_step.h -- backward search for patterns whose every position is a SET of bytes: the rows of the sorted rotations whose
// rotation starts with a string of the pattern's language (kd_classes.hip: bce_hip_count_classes / _locate_classes, `bce -ge` /
// `-gel`), shared with the host (tests/class_emul.cpp runs the same lines on planes it builds naively), the way near_step.h is.
//
// T: the circular text of n bytes.  P: m classes S_0 .. S_(m-1); a class is 256 bits in 8 words, byte c is a member iff bit c & 31
// of word c >> 5 is set.  i in [0, n) is a hit iff T[(i + j) mod n] is in S_j for all j < m.  Two different strings of one length
// own disjoint row intervals, so the hits are the disjoint union of the intervals of the strings of S_0 x .. x S_(m-1) that occur:
// counts add, no position is found twice.  The search enumerates those strings from right to left.  A node is (the interval of the
// suffix chosen so far, the classes still to the left):
//   - a class with ONE member is a plain exact step (fm_step) and needs no memory;
//   - an EMPTY class ends the node: nothing matches;
//   - a WIDE class (two members or more) opens a frame: every member byte whose step from the node's interval has rows is a child;
//   - no class left and rows: the interval is an answer.
// The work of a pattern is the number of non-root nodes that have rows -- every step that does not come back empty:
//   nodes(P) = #{ (j, s) : 1 <= j <= m, s a string of j bytes with s[t] in S_(m-j+t) for all t, s occurs in the circular text },
// a property of text and pattern, not of the order of the walk.  A walk counts it and gives up once the count has passed its budget.
#pragma once
#include "fm_step.h"

#define BCE_CLASS_MAX_WIDE 64u               // = BCE_HIP_CLASS_MAX_WIDE (include/bce_hip.h): the frames of a walk

namespace bce {

constexpr uint32_t CLASS_ONE = 0x100u, CLASS_WIDE = 0x200u;             // class_summary: below CLASS_ONE empty, from CLASS_WIDE on wide
constexpr uint32_t CLASS_OK = 0u, CLASS_OVER = 1u, CLASS_DEEP = 2u;     // class_search's verdicts; the first two are the ABI's status

// the mask test
BCE_HD bool class_has(const uint32_t *mask, uint32_t c) { return (mask[c >> 5] >> (c & 31u)) & 1u; }

// What a walk needs to know of a class: how many members (none, one, more) and, if one, which -- the member in the low byte.
BCE_HD uint32_t class_summary(const uint32_t *mask) {
  uint32_t size = 0, only = 0;
  for (uint32_t w = 0; w < 8u; ++w) {
    size += (uint32_t)__builtin_popcount(mask[w]);
    if (mask[w]) only = 32u * w + (uint32_t)__builtin_ctz(mask[w]);
  }
  return size == 0 ? 0u : size == 1 ? CLASS_ONE | only : CLASS_WIDE;
}

// the smallest member >= from; 256: there is none
BCE_HD uint32_t class_next(const uint32_t *mask, uint32_t from) {
  for (uint32_t c = from; c < 256u;) {
    const uint32_t rest = mask[c >> 5] >> (c & 31u);
    if (rest) return c + (uint32_t)__builtin_ctz(rest);
    c = (c | 31u) + 1u;
  }
  return 256u;
}

// The exact steps from a node: the one-member classes to the left of pos, until a wide class, the pattern's start or the node's
// end.  summary(j): class_summary of S_j.  False: the node has ended (an empty interval or an empty class).  Counts its nodes.
template <class Summary, class Rank2>
BCE_HD bool class_run(Summary &&summary, uint32_t &pos, const uint32_t zeros[8], uint32_t &lo, uint32_t &hi, uint64_t &nodes, Rank2 &&rank2) {
  while (pos > 0) {
    const uint32_t s = summary(pos - 1);
    if (s >= CLASS_WIDE) return true;
    if (s < CLASS_ONE) return false;
    fm_step(s & 0xFFu, zeros, lo, hi, rank2);
    if (lo >= hi) return false;
    ++nodes;
    --pos;
  }
  return true;
}

// A node at a wide class.  cand: the next byte to try at pos.
struct ClassFrame {
  uint32_t lo, hi, pos, cand;
};

// The whole search by one thread: emit(lo, hi) for every answer, lo < hi, in the order of the walk; nodes = the steps that had
// rows.  One frame per wide class at most, BCE_CLASS_MAX_WIDE of them: nothing grows with n, m, the answers or the budget.
// CLASS_DEEP: more wide classes than that, nothing searched.  CLASS_OVER: nodes has passed max_nodes and the walk has stopped --
// what it has emitted by then is a part of the answer and to be dropped.  CLASS_OK: the answer is complete, nodes = nodes(P).
// kd_classes.hip walks the same tree with a wave: its lanes share a frame's candidates.
template <class Rank2, class Emit>
BCE_HD uint32_t class_search(const uint32_t *masks, uint32_t m, uint32_t n, uint64_t max_nodes, const uint32_t zeros[8], uint64_t &nodes,
                             Rank2 &&rank2, Emit &&emit) {
  nodes = 0;
  uint32_t wide = 0;
  for (uint32_t j = 0; j < m; ++j) wide += class_summary(masks + 8 * (size_t)j) >= CLASS_WIDE;
  if (wide > BCE_CLASS_MAX_WIDE) return CLASS_DEEP;
  auto summary = [&](uint32_t j) { return class_summary(masks + 8 * (size_t)j); };
  ClassFrame f[BCE_CLASS_MAX_WIDE];
  int d = -1;                                // the open frame
  auto open = [&](uint32_t lo, uint32_t hi, uint32_t pos) {
    if (!class_run(summary, pos, zeros, lo, hi, nodes, rank2)) return;
    if (pos == 0) emit(lo, hi);
    else f[++d] = ClassFrame{lo, hi, pos, 0u};
  };
  open(0u, n, m);
  while (d >= 0 && nodes <= max_nodes) {
    const uint32_t c = class_next(masks + 8 * (size_t)(f[d].pos - 1), f[d].cand);
    if (c >= 256u) { --d; continue; }
    f[d].cand = c + 1;
    uint32_t a = f[d].lo, b = f[d].hi;
    fm_step(c, zeros, a, b, rank2);
    if (a < b) { ++nodes; open(a, b, f[d].pos - 1); }
  }
  return nodes > max_nodes ? CLASS_OVER : CLASS_OK;
}

}  // namespace bce
