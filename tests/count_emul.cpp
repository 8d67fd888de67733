// count_emul.cpp -- TEST-ONLY: fm_step.h (the backward-search step kd_count.hip runs) on the host, over planes and ranks built
// naively from a BWT (tests/test_count_cpu.py compares its counts with a brute-force count of the circular text).  A stand-alone
// program, so that it can run under ASan + UBSan.
//   input (a file, or stdin): cases of lines "n offset npat", "<BWT, 2 n hex digits or ->", then npat lines "<pattern hex or ->"
//   output: one line per case, its npat cyclic counts separated by blanks
#include <stdint.h>
#include <stdio.h>

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

// K2 as k2_planes.hip defines it, one bit at a time: plane j = bit j of the bytes in the current order, the next order their
// stable partition by that bit, zeros first; pre[j][i] = ones of plane j below position i, i in [0, n]
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
    if (!read_word(f, w)) return 3;                                 // (the offset: the count does not depend on it)
    if (!read_word(f, w)) return 3;
    const unsigned long npat = strtoul(w.c_str(), nullptr, 10);
    std::vector<uint8_t> bwt, pat;
    if (!read_word(f, w) || !from_hex(w, bwt) || bwt.size() != n || n == 0) return 3;
    const Planes pl(bwt);
    for (unsigned long p = 0; p < npat; ++p) {
      if (!read_word(f, w) || !from_hex(w, pat)) return 3;
      const uint32_t c = bce::fm_count(pat.data(), pat.size(), pl.n, pl.zeros, [&](int j, uint32_t a, uint32_t b, uint32_t &ra, uint32_t &rb) {
        ra = pl.pre[j].at(a);
        rb = pl.pre[j].at(b);
      });
      printf(p + 1 < npat ? "%u " : "%u", c);
    }
    printf("\n");
  }
  if (f != stdin) fclose(f);
  return 0;
}
