// lcp_emul.cpp -- TEST-ONLY: the lines kd_lcp.hip shares with the host (lcp_step.h: rot_lcp) over every adjacent pair of a suffix
// array made in Python (tests/test_repeat_cpu.py compares the output with a sort of capped windows of the text).  A stand-alone
// program, so that it can run under ASan + UBSan: the text lies in a heap block of EXACTLY n bytes, so a read at or beyond
// text + n is a sanitizer report.  Every row is compared as a lane of lcp_kernel compares it, for each bound.
//   input (a file, or stdin): cases of lines "n", "<text, 2 n hex digits>", "<n suffix-array entries>"
//   output: per case one line "case n", then per bound L in 1, 2, 7, 8, 9, 4096 one line "l <L> <n words joined by commas>"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../bce_amd/csrc/lcp_step.h"

namespace {

bool from_hex(const std::string &s, std::vector<uint8_t> &out) {
  out.clear();
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

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w;
  while (read_word(f, w)) {
    const unsigned long n = strtoul(w.c_str(), nullptr, 10);
    std::vector<uint8_t> bytes;
    if (!read_word(f, w) || !from_hex(w, bytes) || bytes.size() != n || n == 0) return 3;
    std::vector<uint32_t> sa(n);
    std::vector<bool> seen(n, false);
    for (unsigned long i = 0; i < n; ++i) {                           // a permutation of [0, n)
      if (!read_word(f, w)) return 3;
      const unsigned long v = strtoul(w.c_str(), nullptr, 10);
      if (v >= n || seen[v]) return 3;
      seen[v] = true;
      sa[i] = (uint32_t)v;
    }
    uint8_t *text = static_cast<uint8_t *>(malloc(n));                // exactly n bytes: the redzone starts at text + n
    if (!text) return 2;
    memcpy(text, bytes.data(), n);
    printf("case %lu\n", n);
    for (uint32_t L : {1u, 2u, 7u, 8u, 9u, 4096u}) {
      printf("l %u ", L);
      for (unsigned long r = 0; r < n; ++r)
        printf(r ? ",%u" : "%u", r ? bce::rot_lcp(text, (uint32_t)n, sa[r - 1], sa[r], L) : 0u);
      printf("\n");
    }
    free(text);
  }
  if (f != stdin) fclose(f);
  return 0;
}
