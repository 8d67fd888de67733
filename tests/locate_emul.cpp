// locate_emul.cpp -- TEST-ONLY: the lines kd_locate.hip shares with the host (fm_step.h: fm_range, fm_row_pattern, fm_linear_hit)
// over planes and ranks built naively from a BWT and a suffix array made in Python (tests/test_locate_cpu.py compares the hits
// with a brute-force scan of the text).  A stand-alone program, so that it can run under ASan + UBSan.  The batch is walked as the
// kernels walk it: ranges, an exclusive scan of the row counts, then row by row -- pattern by binary search, position from the
// suffix array, the linear filter; each pattern's rows are then put in ascending order (the device sorts; here std::sort).
//   input (a file, or stdin): cases of lines "n npat", "<BWT, 2 n hex digits>", "<n suffix-array entries>", then npat lines
//                             "<pattern hex or ->"
//   output: per case one line "case n npat", then per pattern "c <cyclic hits or -> l <linear hits or ->", hits joined by commas
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
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

void print_hits(const std::vector<uint32_t> &h) {
  if (h.empty()) { printf("-"); return; }
  for (size_t i = 0; i < h.size(); ++i) printf(i ? ",%u" : "%u", h[i]);
}

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w;
  while (read_word(f, w)) {
    const unsigned long n = strtoul(w.c_str(), nullptr, 10);
    if (!read_word(f, w)) return 3;
    const unsigned long npat = strtoul(w.c_str(), nullptr, 10);
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
    std::vector<std::vector<uint8_t>> pats(npat);
    std::vector<uint32_t> lo(npat);
    std::vector<uint64_t> start(npat + 1, 0);
    for (unsigned long p = 0; p < npat; ++p) {
      if (!read_word(f, w) || !from_hex(w, pats[p])) return 3;
      uint32_t hi;
      bce::fm_range(pats[p].data(), pats[p].size(), pl.n, pl.zeros, lo[p], hi, [&](int j, uint32_t a, uint32_t b, uint32_t &ra, uint32_t &rb) {
        ra = pl.pre[j].at(a);
        rb = pl.pre[j].at(b);
      });
      start[p + 1] = start[p] + (hi - lo[p]);
    }
    std::vector<std::vector<uint32_t>> cyc(npat), lin(npat);
    for (uint64_t r = 0; r < start[npat]; ++r) {
      const uint32_t p = bce::fm_row_pattern(start.data(), (uint32_t)npat, r);
      if (p >= npat || r < start[p] || r >= start[p + 1]) return 4;
      const uint32_t pos = sa.at(lo[p] + (r - start[p]));
      cyc[p].push_back(pos);
      if (bce::fm_linear_hit(pos, pats[p].size(), pl.n)) lin[p].push_back(pos);
    }
    printf("case %lu %lu\n", n, npat);
    for (unsigned long p = 0; p < npat; ++p) {
      std::sort(cyc[p].begin(), cyc[p].end());
      std::sort(lin[p].begin(), lin[p].end());
      printf("c ");
      print_hits(cyc[p]);
      printf(" l ");
      print_hits(lin[p]);
      printf("\n");
    }
  }
  if (f != stdin) fclose(f);
  return 0;
}
