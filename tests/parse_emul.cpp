// parse_emul.cpp -- TEST-ONLY: the rules kd_parse.hip shares with the host (parse_step.h) driven through the kernels' block
// decomposition with a block of B = 4 or 8 positions and a top scan that takes 2 blocks a pass, so that exits, walk, mark, the
// run-length rule and the patch's tiles cross blocks on inputs of tens of bytes (tests/test_parse_cpu.py compares with
// tests/parse_ref.py).  A stand-alone program, so that it can run under ASan + UBSan; every array is a heap block of exactly its size.
//   input (a file, or stdin), words:
//     "parse B min_len" <text hex> <q lengths or -> <q positions or -> <query hex or ->
//     "patch B nlits" <text hex> <ops "len:src,..." or -> <literal bytes hex or ->      (nlits: what the caller CLAIMS to pass)
//   output, one line each:
//     "parse <ops or -> <literal bytes hex or -> nops nlits ncopies copied <patched hex or ->"
//     "patch ok <hex or ->"   or   "patch bad <the refusal's words>"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../bce_amd/csrc/parse_step.h"

namespace {

using namespace bce;

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

bool words_of(const std::string &s, char sep, std::vector<uint32_t> &out) {
  out.clear();
  if (s == "-") return true;
  const char *p = s.c_str();
  while (*p) {
    char *end = nullptr;
    const unsigned long long v = strtoull(p, &end, 10);
    if (end == p || v > 0xFFFFFFFFull) return false;
    out.push_back((uint32_t)v);
    p = end;
    if (*p == sep || *p == ':') ++p; else if (*p) return false;
  }
  return true;
}

void print_hex(const std::vector<uint8_t> &b) {
  if (b.empty()) { printf("-"); return; }
  for (uint8_t v : b) printf("%02x", v);
}

struct Ops { std::vector<uint32_t> w; };                // pairs (len, src)

// ---- the parse, launch by launch (kd_parse.hip) ----
bool parse(uint32_t B, uint32_t P, const std::vector<uint32_t> &len, const std::vector<uint32_t> &pos, const std::vector<uint8_t> &query,
           uint32_t min_len, Ops &ops, std::vector<uint8_t> &lits, uint64_t info[4]) {
  const uint32_t q = (uint32_t)len.size();
  info[0] = info[1] = info[2] = info[3] = 0;
  ops.w.clear();
  lits.clear();
  if (q == 0) return true;
  const uint32_t nb = (q + B - 1) / B;
  uint32_t rounds = 0;
  while ((1u << rounds) < B) ++rounds;
  // exit: per block, pointer doubling over two arrays
  std::vector<uint32_t> exit1(q);
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t base = b * B;
    std::vector<uint32_t> nxt[2] = {std::vector<uint32_t>(B), std::vector<uint32_t>(B)};
    for (uint32_t i = 0; i < B; ++i) nxt[0][i] = base + i < q ? parse_next1(base + i, parse_jump(len[base + i], min_len)) : 0u;
    int cur = 0;
    for (uint32_t r = 0; r < rounds; ++r) {
      for (uint32_t i = 0; i < B; ++i) {
        uint32_t v = nxt[cur][i];
        if (!parse_left_block(v, base)) v = nxt[cur].at(v - 1u - base);
        nxt[cur ^ 1][i] = v;
      }
      cur ^= 1;
    }
    for (uint32_t i = 0; i < B && base + i < q; ++i) {
      if (!parse_left_block(nxt[cur][i], base)) return false;        // the rounds did not reach across the block
      exit1[base + i] = nxt[cur][i];
    }
  }
  // walk
  std::vector<uint32_t> entry(nb, PARSE_NO_ENTRY);
  for (uint32_t e = q - 1u;;) {
    entry.at(e / B) = e;
    const uint32_t v = exit1.at(e);
    if (v == 0u) break;
    e = v - 1u;
  }
  // mark: whole rows
  std::vector<uint8_t> flag((size_t)nb * B, PARSE_NONE);
  for (uint32_t b = 0; b < nb; ++b) {
    if (entry[b] == PARSE_NO_ENTRY) continue;
    const uint32_t base = b * B;
    for (uint32_t i = entry[b] - base;;) {
      const uint32_t l = len.at(base + i);
      flag.at(base + i) = parse_kind(l, min_len);
      const uint32_t j = parse_jump(l, min_len);
      if (j > i) break;
      i -= j;
    }
  }
  auto right = [&](size_t e) { return e + 1 < flag.size() ? flag[e + 1] : PARSE_NONE; };
  // count, top (P blocks a pass), emit
  std::vector<uint64_t> bsum(nb);
  uint64_t copies = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < B; ++i) {
      const size_t e = (size_t)b * B + i;
      s += (uint64_t)parse_is_head(flag[e], right(e)) << 32 | (flag[e] == PARSE_LIT);
      copies += flag[e] == PARSE_COPY;
    }
    bsum[b] = s;
  }
  uint64_t carry = 0;
  for (uint32_t at = 0; at < nb; at += P) {
    uint64_t tot = 0;
    for (uint32_t i = at; i < at + P && i < nb; ++i) { const uint64_t v = bsum[i]; bsum[i] = carry + tot; tot += v; }
    carry += tot;
  }
  info[0] = carry >> 32; info[1] = carry & 0xFFFFFFFFull; info[2] = copies; info[3] = q - info[1];
  ops.w.assign((size_t)info[0] * 2, 0xDEADBEEFu);
  lits.assign((size_t)info[1], 0);
  std::vector<uint32_t> hpre((size_t)info[0]);
  for (uint32_t b = 0; b < nb; ++b) {
    uint32_t k = (uint32_t)(bsum[b] >> 32), l = (uint32_t)bsum[b];
    for (uint32_t i = 0; i < B; ++i) {
      const size_t e = (size_t)b * B + i;
      if (flag[e] == PARSE_LIT) lits.at(l++) = query.at(e);
      if (parse_is_head(flag[e], right(e))) {
        if (flag[e] == PARSE_COPY) { ops.w.at(2 * (size_t)k) = len.at(e); ops.w.at(2 * (size_t)k + 1) = pos.empty() ? 0u : pos.at(e); }
        else ops.w.at(2 * (size_t)k + 1) = PARSE_LITERAL;
        hpre.at(k++) = l;
      }
    }
  }
  for (size_t k = 0; k < hpre.size(); ++k)
    if (ops.w[2 * k + 1] == PARSE_LITERAL) ops.w[2 * k] = hpre[k] - (k ? hpre[k - 1] : 0u);
  return true;
}

// ---- the patch: check, top, fill, copy by tiles of output (B bytes a tile, 3 bytes a chunk) ----
const char *patch(uint32_t B, const std::vector<uint8_t> &text, const Ops &ops, const std::vector<uint8_t> &lits, uint64_t nlits,
                  std::vector<uint8_t> &out) {
  out.clear();
  const uint32_t nops = (uint32_t)(ops.w.size() / 2), n = (uint32_t)text.size();
  uint32_t bits = 0;
  uint64_t total = 0, lit_total = 0;
  std::vector<uint64_t> off64(nops), loff64(nops);
  for (uint32_t k = 0; k < nops; ++k) {
    bits |= patch_op_bad(ops.w[2 * k], ops.w[2 * k + 1], n);
    off64[k] = total; loff64[k] = lit_total;
    total += ops.w[2 * k];
    lit_total += patch_lit_len(ops.w[2 * k], ops.w[2 * k + 1]);
  }
  if (const char *why = patch_list_bad(bits, total, lit_total, nlits)) return why;
  if (lits.size() != nlits) return "emulator: the literal bytes given are not the count given";
  if (nops == 0) return nullptr;
  std::vector<uint32_t> off(nops + 1), loff(nops);
  for (uint32_t k = 0; k < nops; ++k) { off[k] = (uint32_t)off64[k]; loff[k] = (uint32_t)loff64[k]; }
  off[nops] = (uint32_t)total;
  out.assign((size_t)total, 0xEE);
  auto src = [&](uint32_t k) { return ops.w[2 * k + 1] == PARSE_LITERAL ? lits.data() + loff[k] : text.data() + ops.w[2 * k + 1]; };
  const uint32_t chunk = 3;
  for (uint32_t lead = 0; lead < chunk; ++lead) {                     // every alignment of the output's address gives the same bytes
    std::vector<uint8_t> res((size_t)total, 0xEE);
    const uint64_t span = (uint64_t)lead + total, tile = (uint64_t)B * chunk;
    for (uint64_t t0 = 0; t0 < span; t0 += tile) {
      const uint64_t t1 = t0 + tile < span ? t0 + tile : span;
      const uint32_t first = (uint32_t)(t0 > lead ? t0 - lead : 0u), last = (uint32_t)(t1 - 1u - lead);
      const uint32_t k0 = patch_op_of(off.data(), nops, first), k1 = patch_op_of(off.data(), nops, last);
      for (uint64_t c0 = t0; c0 < t1; c0 += chunk) {
        const uint32_t lo = (uint32_t)(c0 > lead ? c0 - lead : 0u), hi = (uint32_t)((c0 + chunk < span ? c0 + chunk : span) - lead);
        uint32_t k = k0 + patch_op_of(off.data() + k0, k1 - k0 + 1u, lo);
        uint32_t begin = off.at(k), end = off.at(k + 1);
        const uint8_t *s = src(k);
        if (hi - lo == chunk && end >= hi) { memcpy(res.data() + lo, s + (lo - begin), chunk); continue; }
        for (uint32_t o = lo; o < hi; ++o) {
          while (end <= o) { ++k; begin = end; end = off.at(k + 1); s = src(k); }
          res.at(o) = s[o - begin];
        }
      }
    }
    if (lead && res != out) return "emulator: the result depends on the output's alignment";
    out = res;
  }
  return nullptr;
}

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w, a, b, c, d;
  while (read_word(f, w)) {
    std::string sb, sm;
    if (!read_word(f, sb) || !read_word(f, sm) || !read_word(f, a) || !read_word(f, b) || !read_word(f, c)) return 3;
    const uint32_t B = (uint32_t)strtoul(sb.c_str(), nullptr, 10);
    if (B != 4 && B != 8) return 3;
    std::vector<uint8_t> text, lits, out;
    if (!from_hex(a, text)) return 3;
    Ops ops;
    if (w == "parse") {
      if (!read_word(f, d)) return 3;
      const uint32_t min_len = (uint32_t)strtoul(sm.c_str(), nullptr, 10);
      std::vector<uint32_t> len, pos;
      std::vector<uint8_t> query;
      if (min_len < 1 || !words_of(b, ',', len) || !words_of(c, ',', pos) || !from_hex(d, query) || query.size() != len.size() ||
          (!pos.empty() && pos.size() != len.size()))
        return 3;
      for (size_t i = 0; i < len.size(); ++i) if (len[i] > i + 1) return 3;
      uint64_t info[4];
      if (!parse(B, 2, len, pos, query, min_len, ops, lits, info)) return 4;
      printf("parse ");
      if (ops.w.empty()) printf("-");
      for (size_t k = 0; k < ops.w.size() / 2; ++k) printf(k ? ",%u:%u" : "%u:%u", ops.w[2 * k], ops.w[2 * k + 1]);
      printf(" ");
      print_hex(lits);
      printf(" %llu %llu %llu %llu ", (unsigned long long)info[0], (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[3]);
      if (pos.empty()) { printf("-\n"); continue; }
      const char *why = patch(B, text, ops, lits, lits.size(), out);
      if (why) { printf("BAD:%s\n", why); continue; }
      print_hex(out);
      printf("\n");
    } else if (w == "patch") {
      const uint64_t nlits = strtoull(sm.c_str(), nullptr, 10);
      if (!words_of(b, ',', ops.w) || ops.w.size() % 2 || !from_hex(c, lits)) return 3;
      const char *why = patch(B, text, ops, lits, nlits, out);
      if (why) { printf("patch bad %s\n", why); continue; }
      printf("patch ok ");
      print_hex(out);
      printf("\n");
    } else {
      return 3;
    }
  }
  if (f != stdin) fclose(f);
  return 0;
}
