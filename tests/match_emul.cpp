// match_emul.cpp -- TEST-ONLY: the lines kd_match.hip shares with the host (fm_step.h: fm_match_end) over planes and ranks built
// naively from a BWT and a suffix array made in Python (tests/test_match_cpu.py compares the lengths with a brute-force scan of the
// text and checks every position).  A stand-alone program, so that it can run under ASan + UBSan.  Every end position of a query
// is searched as a lane of match_kernel searches it, in both modes and for each length bound; the coverage is reduced as the
// coverage kernels reduce it: the running maximum of ~(i - len[i] + 1) from the last element to the first, 0 where the match is
// too short, then the j whose maximum says that a start at or before j lies behind them.
//   input (a file, or stdin): cases of lines "n nq", "<BWT, 2 n hex digits>", "<n suffix-array entries>", then nq lines
//                             "<query hex or ->"
//   output: per case one line "case n nq", then per query, mode (c cyclic, l linear) and bound L in 1, 2, 7, 4096 one line
//           "m <mode> <L> <lengths or -> <positions or ->" (joined by commas), and per mode and min_len in 1, 3, 8 one line
//           "v <mode> <min_len> <covered>"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../bce_amd/csrc/fm_step.h"

namespace {

bool from_hex(const std::string &s, std::vector<uint8_t> &out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    unsigned v = 0;
    if (sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
    out.push_back((uint8_t)v);
  }
  return true;
}

bool read_word(FILE *f, std::string &w) {
  w.clear();
  int ch = fgetc(f);
  while (ch == ' ' || ch == '\n' || ch == '\r' || ch == '\t') ch = fgetc(f);
  while (ch != EOF && ch != ' ' && ch != '\n' && ch != '\r' && ch != '\t') { w.push_back((char)ch); ch = fgetc(f); }
  return !w.empty();
}

// K2 as k2_planes.hip defines it, one bit at a time (as tests/count_emul.cpp)
struct Planes {
  uint32_t n = 0;
  uint32_t zeros[8] = {0};
  std::vector<uint32_t> pre[8];
  explicit Planes(const std::vector<uint8_t> &bwt) : n((uint32_t)bwt.size()) {
    std::vector<uint8_t> cur = bwt, nxt(n);
    for (int j = 0; j < 8; ++j) {
      pre[j].assign((size_t)n + 1, 0);
      for (uint32_t i = 0; i < n; ++i) pre[j][i + 1] = pre[j][i] + ((cur[i] >> j) & 1u);
      zeros[j] = n - pre[j][n];
      uint32_t z = 0, o = zeros[j];
      for (uint32_t i = 0; i < n; ++i) { if ((cur[i] >> j) & 1u) nxt[o++] = cur[i]; else nxt[z++] = cur[i]; }
      cur.swap(nxt);
    }
  }
};

void print_words(const std::vector<uint32_t> &h) {
  if (h.empty()) { printf("-"); return; }
  for (size_t i = 0; i < h.size(); ++i) printf(i ? ",%u" : "%u", h[i]);
}

bool array_read_for_one_byte = false;                 // a text of one byte has no suffix array: fm_match_end must not ask for it

template <bool Linear>
void match_all(const Planes &pl, const std::vector<uint32_t> &sa, const std::vector<uint8_t> &q, uint32_t L, bool want_pos,
               std::vector<uint32_t> &len, std::vector<uint32_t> &pos) {
  len.assign(q.size(), 0);
  pos.assign(want_pos ? q.size() : 0, 0);
  for (size_t i = 0; i < q.size(); ++i) {
    uint32_t l, row;
    bce::fm_match_end<Linear>(
        q.data(), i, L, pl.n, pl.zeros, want_pos, l, row,
        [&](int j, uint32_t a, uint32_t b, uint32_t &ra, uint32_t &rb) {
          ra = pl.pre[j].at(a);
          rb = pl.pre[j].at(b);
        },
        [&](uint32_t r) {
          if (pl.n == 1) array_read_for_one_byte = true;
          return sa.at(r);
        });
    len[i] = l;
    if (want_pos) pos[i] = l ? (pl.n == 1 ? 0u : sa.at(row)) : 0xFFFFFFFFu;
  }
}

uint64_t covered(const std::vector<uint32_t> &len, uint32_t min_len) {
  uint64_t count = 0;
  uint32_t run = 0;
  for (size_t j = len.size(); j-- > 0;) {
    const uint32_t v = len[j] >= min_len ? ~((uint32_t)j - len[j] + 1u) : 0u;
    run = run > v ? run : v;
    count += run != 0u && ~run <= (uint32_t)j;
  }
  return count;
}

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w;
  while (read_word(f, w)) {
    const unsigned long n = strtoul(w.c_str(), nullptr, 10);
    if (!read_word(f, w)) return 3;
    const unsigned long nq = strtoul(w.c_str(), nullptr, 10);
    std::vector<uint8_t> bwt;
    if (!read_word(f, w) || !from_hex(w, bwt) || bwt.size() != n || n == 0) return 3;
    std::vector<uint32_t> sa(n);
    std::vector<bool> seen(n, false);
    for (unsigned long i = 0; i < n; ++i) {                         // a permutation of [0, n)
      if (!read_word(f, w)) return 3;
      const unsigned long v = strtoul(w.c_str(), nullptr, 10);
      if (v >= n || seen[v]) return 3;
      seen[v] = true;
      sa[i] = (uint32_t)v;
    }
    const Planes pl(bwt);
    std::vector<std::vector<uint8_t>> qs(nq);
    for (unsigned long k = 0; k < nq; ++k)
      if (!read_word(f, w) || !from_hex(w, qs[k])) return 3;
    printf("case %lu %lu\n", n, nq);
    std::vector<uint32_t> len, pos, none;
    for (unsigned long k = 0; k < nq; ++k) {
      for (int linear = 0; linear < 2; ++linear) {
        for (uint32_t L : {1u, 2u, 7u, 4096u}) {
          if (linear) match_all<true>(pl, sa, qs[k], L, true, len, pos); else match_all<false>(pl, sa, qs[k], L, true, len, pos);
          printf("m %c %u ", linear ? 'l' : 'c', L);
          print_words(len);
          printf(" ");
          print_words(pos);
          printf("\n");
        }
        for (uint32_t min_len : {1u, 3u, 8u}) {                     // as bce_hip_coverage: the search with L = min_len, no positions
          if (linear) match_all<true>(pl, sa, qs[k], min_len, false, len, none); else match_all<false>(pl, sa, qs[k], min_len, false, len, none);
          printf("v %c %u %llu\n", linear ? 'l' : 'c', min_len, (unsigned long long)covered(len, min_len));
        }
      }
    }
  }
  if (f != stdin) fclose(f);
  return array_read_for_one_byte ? 4 : 0;
}
