// top_emul.cpp -- TEST-ONLY: the lines bce_hip_top_kgrams shares with the host (bce_amd/csrc/top_step.h): the bin of a class, the
// threshold bin, the sort key and its significant bits, and the escape of `bce -gf`.  A stand-alone program, so that it can run
// under ASan + UBSan (tests/test_top_cpu.py); the 32 counters lie in a heap block of exactly 32 words.
//   input (a file, or stdin), one case per line:
//     "s <limit> <m> <m class sizes in row order>"   the selection as the device runs it, on the host: the histogram of top_bin, the
//          threshold, the candidates in row order with their keys, a STABLE sort on the keys' low top_key_bits bits, the first
//          min(limit, m).  Output: "s <t> <candidates> <top> <bits> <found> <found pairs size:index>"
//     "e"   output: "e" and the escapes of the bytes 0 .. 255, separated by blanks
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../bce_amd/csrc/top_step.h"

namespace {

bool read_word(FILE *f, std::string &w, bool *eol) {
  w.clear();
  *eol = false;
  int ch = fgetc(f);
  while (ch == ' ' || ch == '\r' || ch == '\t') ch = fgetc(f);
  while (ch != EOF && ch != ' ' && ch != '\n' && ch != '\r' && ch != '\t') { w.push_back((char)ch); ch = fgetc(f); }
  if (ch == '\n' || ch == EOF) *eol = true;
  return !w.empty();
}

bool read_number(FILE *f, uint64_t *v) {
  std::string w;
  bool eol;
  if (!read_word(f, w, &eol)) return false;
  char *end = nullptr;
  *v = strtoull(w.c_str(), &end, 10);
  return end && *end == 0;
}

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w;
  bool eol;
  for (;;) {
    if (!read_word(f, w, &eol)) { if (feof(f)) break; continue; }
    if (w == "e") {
      printf("e");
      for (int b = 0; b < 256; ++b) {
        char *esc = static_cast<char *>(malloc(5));                    // exactly the room the header asks for
        if (!esc) return 2;
        const int len = bce::top_escape((uint8_t)b, esc);
        if (len != (int)std::string(esc).size()) return 4;
        printf(" %s", esc);
        free(esc);
      }
      printf("\n");
      continue;
    }
    if (w != "s") return 3;
    uint64_t limit = 0, m = 0;
    if (!read_number(f, &limit) || !read_number(f, &m) || limit < 1 || m < 1 || m > (1u << 24)) return 3;
    std::vector<uint32_t> sizes(m);
    for (uint64_t i = 0; i < m; ++i) {
      uint64_t v = 0;
      if (!read_number(f, &v) || v < 1 || v > 0x7FFFFFFFull) return 3;
      sizes[i] = (uint32_t)v;
    }
    uint64_t *H = static_cast<uint64_t *>(calloc(bce::kTopBins, sizeof(uint64_t)));
    if (!H) return 2;
    for (uint32_t s : sizes) H[bce::top_bin(s)] += 1;
    const uint64_t classes = bce::top_classes(H), want = classes < limit ? classes : limit;
    if (classes != m) return 4;
    uint64_t cand = 0;
    int top = 0;
    const int t = bce::top_threshold(H, want, &cand, &top);
    free(H);
    const uint32_t bits = bce::top_key_bits(t, top), mask = bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1u;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;                  // (key, index), in row order
    for (uint64_t i = 0; i < m; ++i)
      if ((sizes[i] >> t) != 0) pairs.emplace_back(bce::top_key(top, sizes[i]), (uint32_t)i);
    if (pairs.size() != cand) return 4;                                // the histogram's count is the candidates' count, exactly
    for (const auto &p : pairs) if ((p.first & mask) != p.first) return 4;   // no key has a bit above the sorted ones
    std::stable_sort(pairs.begin(), pairs.end(), [&](const auto &a, const auto &b) { return (a.first & mask) < (b.first & mask); });
    const uint64_t found = want < cand ? want : cand;
    printf("s %d %llu %d %u %llu", t, (unsigned long long)cand, top, bits, (unsigned long long)found);
    for (uint64_t e = 0; e < found; ++e) printf(" %u:%u", bce::top_key_max(top) - pairs[e].first, pairs[e].second);
    printf("\n");
  }
  if (f != stdin) fclose(f);
  return 0;
}
