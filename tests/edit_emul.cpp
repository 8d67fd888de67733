// edit_emul.cpp -- TEST-ONLY: edit_step.h (the three-way branching backward search kd_edit.hip runs) on the host, over planes and
// ranks built naively from a BWT, the way near_emul.cpp runs near_step.h (tests/test_edit_cpu.py expands its candidates through a
// naive suffix array, reduces them per position and compares with tests/edit_ref.py).  A stand-alone program, so that it can run
// under ASan + UBSan.
//   input (a file, or stdin): cases of lines "n offset npat", "<BWT, 2 n hex digits>", then npat lines "<pattern hex or ->"
//   output: for every pattern three lines, k = 0, 1, 2: the number of candidates, then " | lo hi d l" for every candidate
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../bce_amd/csrc/edit_step.h"

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

// K2 as k2_planes.hip defines it, one bit at a time (count_emul.cpp's)
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

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w;
  while (read_word(f, w)) {
    const unsigned long n = strtoul(w.c_str(), nullptr, 10);
    if (!read_word(f, w)) return 3;                                 // (the offset: the rows do not depend on it)
    if (!read_word(f, w)) return 3;
    const unsigned long npat = strtoul(w.c_str(), nullptr, 10);
    std::vector<uint8_t> bwt, pat;
    if (!read_word(f, w) || !from_hex(w, bwt) || bwt.size() != n || n == 0) return 3;
    const Planes pl(bwt);
    auto rank2 = [&](int j, uint32_t a, uint32_t b, uint32_t &ra, uint32_t &rb) {
      ra = pl.pre[j].at(a);
      rb = pl.pre[j].at(b);
    };
    for (unsigned long p = 0; p < npat; ++p) {
      if (!read_word(f, w) || !from_hex(w, pat)) return 3;
      for (uint32_t k = 0; k <= BCE_EDIT_MAX_K; ++k) {
        uint64_t cands = 0;
        std::string rows;
        bce::edit_search(pat.data(), pat.size(), pl.n, k, pl.zeros, rank2, [&](uint32_t lo, uint32_t hi, uint32_t d, uint32_t loff) {
          if (lo >= hi || hi > pl.n || d > k || loff > 2 * k || bce::edit_code(d, loff) >= BCE_EDIT_DEAD) abort();
          if (bce::edit_code_dist(bce::edit_code(d, loff)) != d || bce::edit_code_loff(bce::edit_code(d, loff)) != loff) abort();
          ++cands;
          rows += " | " + std::to_string(lo) + " " + std::to_string(hi) + " " + std::to_string(d) + " " +
                  std::to_string(bce::edit_length(pat.size(), k, loff));
        });
        printf("%llu%s\n", (unsigned long long)cands, rows.c_str());
      }
    }
  }
  if (f != stdin) fclose(f);
  return 0;
}
