// edit_step.h -- backward search that branches three ways: the rows of the sorted rotations whose rotation starts with a string
// within k edits (substitutions, insertions, deletions) of a pattern (kd_edit.hip: bce_hip_count_edit / _locate_edit, `bce -gw` /
// `-gwl`), shared with the host (tests/edit_emul.cpp runs the same lines on planes it builds naively), the way near_step.h is.
//
// T: the circular text of n bytes, P: a pattern of m bytes.  e(P, S), the ANCHORED edit distance to a string S of l bytes: the
// fewest edits that turn P into S among the alignments in which P's first byte stands against S's first and P's last against S's
// last, each of the two a match or a substitution (include/bce_hip.h has the definition in full).  The search enumerates edit
// scripts from right to left.  A node is (the interval of the suffix chosen so far, pos = the bytes of P still to the left, the
// edits so far, the length of the string so far less the bytes of P used: loff = l - (m - k) at the end, in [0, 2 k]):
//   - with budget left at pos > 0, own = P[pos - 1]:
//       substitution  every byte c != own whose step from the node's interval has rows -> (that step, pos - 1), one more edit;
//       insertion     (the text has a byte P lacks) every byte c whose step has rows, when 0 < pos < m -> (the same step, pos),
//                     one more edit, one byte longer.  The two children of one c share the rank step;
//       deletion      (P has a byte the text lacks) when 2 <= pos <= m - 1 -> (the same interval, pos - 1), one more edit, one
//                     byte shorter;
//     then the node takes the exact step and moves one byte to the left; an empty interval ends it;
//   - with the budget spent, the rest of P is near_finish;
//   - pos == 0 with rows left: the interval is a CANDIDATE, at the node's edits and length.
// The bounds on pos are the anchors: nothing is inserted outside P's two ends, and neither end is deleted.
// Different scripts reach one string and strings of different lengths nest, so a position is a candidate many times: the answer
// is the minimum (edits, length) per position, kd_edit.hip's reduce.  One pruning: an insertion directly followed by a deletion at
// the same node, or the reverse, spells the string a substitution (or the exact step) spells with fewer edits and the same length,
// and the anchors allow that substitution wherever they allow the pair, so a child opened by one never opens the other before it
// has taken a step.  No minimum changes.
#pragma once
#include "near_step.h"

#define BCE_EDIT_MAX_K 2u                    // = BCE_HIP_EDIT_MAX_K (include/bce_hip.h)
#define BCE_EDIT_CODE_BITS 4u                // a candidate's (edits, loff) in one code: they order as the pair does
#define BCE_EDIT_DEAD 15u                    // the code of a candidate that linear mode drops: after every live one

namespace bce {

static_assert((BCE_EDIT_MAX_K + 1u) * (2u * BCE_EDIT_MAX_K + 1u) <= BCE_EDIT_DEAD, "every live code is below the dead one");

BCE_HD uint32_t edit_code(uint32_t d, uint32_t loff) { return d * (2u * BCE_EDIT_MAX_K + 1u) + loff; }
BCE_HD uint32_t edit_code_dist(uint32_t code) { return code / (2u * BCE_EDIT_MAX_K + 1u); }
BCE_HD uint32_t edit_code_loff(uint32_t code) { return code % (2u * BCE_EDIT_MAX_K + 1u); }
// the length of a candidate: loff - k bytes more than the pattern (never negative: a deletion needs two bytes of P beside it)
BCE_HD uint64_t edit_length(uint64_t m, uint32_t k, uint32_t loff) { return m + loff - k; }

// the anchors
BCE_HD bool edit_may_insert(uint64_t pos, uint64_t m) { return pos > 0 && pos < m; }
BCE_HD bool edit_may_delete(uint64_t pos, uint64_t m) { return pos >= 2 && pos + 1 <= m; }

enum EditCame : uint32_t { EDIT_BY_STEP = 0, EDIT_BY_INS = 1, EDIT_BY_DEL = 2 };   // what brought a node to its pos (the pruning)

// A node with budget left.  cand: 2 c: the step of byte c is next, and its substitution child; 2 c + 1: its insertion child, from
// the step kept in (a, b); 512: the deletion; 513: all tried, the exact step is next.
struct EditFrame {
  uint32_t lo, hi;
  uint64_t pos;
  uint32_t loff, cand, came;
  uint32_t a, b;
};

// The whole search by one thread: emit(lo, hi, d, loff) for every candidate, lo < hi, in the order of the walk.  At most k + 1
// frames are open, as in near_search.  kd_edit.hip walks the same tree with a wave.
template <class Rank2, class Emit>
BCE_HD void edit_search(const uint8_t *pat, uint64_t m, uint32_t n, uint32_t k, const uint32_t zeros[8], Rank2 &&rank2, Emit &&emit) {
  EditFrame f[BCE_EDIT_MAX_K + 1];
  int d = 0;                                 // the open frame; its edits
  f[0] = EditFrame{0u, n, m, k, 0u, EDIT_BY_STEP, 0u, 0u};
  while (d >= 0) {
    EditFrame &F = f[d];
    if (F.lo >= F.hi) { --d; continue; }
    if (F.pos == 0) { emit(F.lo, F.hi, (uint32_t)d, F.loff); --d; continue; }
    if ((uint32_t)d == k) {
      near_finish(pat, F.pos, zeros, F.lo, F.hi, rank2);
      if (F.lo < F.hi) emit(F.lo, F.hi, (uint32_t)d, F.loff);
      --d;
      continue;
    }
    const uint32_t own = pat[F.pos - 1];
    if (F.cand < 512u) {
      const uint32_t c = F.cand >> 1;
      const bool ins = F.cand & 1u;
      ++F.cand;
      if (!ins) {
        if (!near_child(c, zeros, F.lo, F.hi, F.a, F.b, rank2)) { ++F.cand; continue; }
        if (c != own) { f[d + 1] = EditFrame{F.a, F.b, F.pos - 1, F.loff, 0u, EDIT_BY_STEP, 0u, 0u}; ++d; }
      } else if (edit_may_insert(F.pos, m) && F.came != EDIT_BY_DEL) {
        f[d + 1] = EditFrame{F.a, F.b, F.pos, F.loff + 1u, 0u, EDIT_BY_INS, 0u, 0u};
        ++d;
      }
      continue;
    }
    if (F.cand == 512u) {
      ++F.cand;
      if (edit_may_delete(F.pos, m) && F.came != EDIT_BY_INS) { f[d + 1] = EditFrame{F.lo, F.hi, F.pos - 1, F.loff - 1u, 0u, EDIT_BY_DEL, 0u, 0u}; ++d; }
      continue;
    }
    fm_step(own, zeros, F.lo, F.hi, rank2);
    F.pos -= 1; F.cand = 0; F.came = EDIT_BY_STEP;
  }
}

}  // namespace bce
