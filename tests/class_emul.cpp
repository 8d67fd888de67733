// class_emul.cpp -- TEST-ONLY: class_step.h (the backward search by byte classes kd_classes.hip runs) on the host, over planes and
// ranks built naively from a BWT, the way near_emul.cpp runs near_step.h (tests/test_class_cpu.py compares its answers with a brute
// force over the circular text); and class_expr.h, the expression language of `bce -ge`, beside its Python twin.  A stand-alone
// program, so that it can run under ASan + UBSan.
//   search, input (a file): cases of lines "n offset npat", "<BWT, 2 n hex digits>", then npat lines "<budget> <masks: 64 hex
//     digits per class, its 8 words little-endian, or ->";  output per pattern: "status nodes" and " | lo hi" for every answer
//   --parse, input (a file): lines "<0 or 1: ignore case> <expression in hex, or ->";  output per line: "bad", or "ok" and the
//     masks in the same hex (- for none)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../bce_amd/csrc/class_expr.h"
#include "../bce_amd/csrc/class_step.h"

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

int parse_mode(FILE *f) {
  std::string w;
  std::vector<uint8_t> expr;
  std::vector<uint32_t> masks;
  while (read_word(f, w)) {
    if (w != "0" && w != "1") return 3;
    const bool ignore_case = w == "1";
    if (!read_word(f, w) || !from_hex(w, expr)) return 3;
    const char *why = nullptr;
    if (!bce::compile_classes(expr.data(), expr.size(), ignore_case, masks, &why)) {
      if (!why) abort();
      printf("bad\n");
      continue;
    }
    if (masks.size() % 8 || masks.size() / 8 > bce::kClassExprMax) abort();
    printf("ok ");
    for (uint32_t v : masks) printf("%02x%02x%02x%02x", v & 255u, (v >> 8) & 255u, (v >> 16) & 255u, v >> 24);
    printf(masks.empty() ? "-\n" : "\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const bool parse = argc > 1 && strcmp(argv[1], "--parse") == 0;
  const char *path = parse ? (argc > 2 ? argv[2] : nullptr) : argc > 1 ? argv[1] : nullptr;
  FILE *f = path ? fopen(path, "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  if (parse) {
    const int rc = parse_mode(f);
    if (f != stdin) fclose(f);
    return rc;
  }
  std::string w;
  while (read_word(f, w)) {
    const unsigned long n = strtoul(w.c_str(), nullptr, 10);
    if (!read_word(f, w)) return 3;                                 // (the offset: the rows do not depend on it)
    if (!read_word(f, w)) return 3;
    const unsigned long npat = strtoul(w.c_str(), nullptr, 10);
    std::vector<uint8_t> bwt, raw;
    if (!read_word(f, w) || !from_hex(w, bwt) || bwt.size() != n || n == 0) return 3;
    const Planes pl(bwt);
    auto rank2 = [&](int j, uint32_t a, uint32_t b, uint32_t &ra, uint32_t &rb) {
      ra = pl.pre[j].at(a);
      rb = pl.pre[j].at(b);
    };
    for (unsigned long p = 0; p < npat; ++p) {
      if (!read_word(f, w)) return 3;
      const unsigned long long budget = strtoull(w.c_str(), nullptr, 10);
      if (!read_word(f, w) || !from_hex(w, raw) || raw.size() % 32) return 3;
      std::vector<uint32_t> masks(raw.size() / 4 + 8);               // (eight words more, so that an empty pattern has an address)
      for (size_t i = 0; i < raw.size() / 4; ++i) masks[i] = raw[4 * i] | raw[4 * i + 1] << 8 | raw[4 * i + 2] << 16 | (uint32_t)raw[4 * i + 3] << 24;
      uint64_t nodes = 0;
      std::string rows;
      const uint32_t status = bce::class_search(masks.data(), (uint32_t)(raw.size() / 32), pl.n, budget, pl.zeros, nodes, rank2, [&](uint32_t lo, uint32_t hi) {
        if (lo >= hi || hi > pl.n) abort();
        rows += " | " + std::to_string(lo) + " " + std::to_string(hi);
      });
      printf("%u %llu%s\n", status, (unsigned long long)nodes, rows.c_str());
    }
  }
  if (f != stdin) fclose(f);
  return 0;
}
