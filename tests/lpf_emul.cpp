// lpf_emul.cpp -- TEST-ONLY: the rules kd_self.hip shares with the host (lpf_step.h) driven through the kernels' block
// decomposition with a block of B = 4 or 8 rows, so that local and far answers, the top tree and the chain's jumps cross blocks on
// inputs of tens of bytes (tests/test_lpf_cpu.py compares with tests/lpf_ref.py).  A stand-alone program, so that it can run under
// ASan + UBSan; the text, the rows and every tree are heap blocks of exactly their size.  The chain runs over the mirrored arrays by
// parse_step.h's rules one position at a time: its block decomposition is kd_parse's and tests/parse_emul.cpp's.
//   input (a file, or stdin), words:
//     "nsv B" <values "v,v,..">
//     "self B min_len max_len" <text hex> <the sorted rotations "r,r,..">
//   output, one line each:
//     "nsv <psv> <nsv>"
//     "self <lpf> <src> <ops "len:src,.."> <literal bytes hex or -> nops nlits ncopies copied"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../bce_amd/csrc/lpf_step.h"
#include "../bce_amd/csrc/parse_step.h"

namespace {

using namespace bce;

bool read_word(FILE *f, std::string &w) {
  w.clear();
  int ch = fgetc(f);
  while (ch == ' ' || ch == '\n' || ch == '\r' || ch == '\t') ch = fgetc(f);
  while (ch != EOF && ch != ' ' && ch != '\n' && ch != '\r' && ch != '\t') { w.push_back((char)ch); ch = fgetc(f); }
  return !w.empty();
}

// an array of exactly n elements on the heap (n == 0: one element nobody reads)
template <class T>
struct Block {
  std::unique_ptr<T[]> p;
  size_t n = 0;
  explicit Block(size_t n_ = 0) : p(new T[n_ ? n_ : 1]), n(n_) {}
  T *get() { return p.get(); }
  const T *get() const { return p.get(); }
};

bool from_hex(const std::string &s, Block<uint8_t> &out) {
  if (s == "-") { out = Block<uint8_t>(0); return true; }
  if (s.size() % 2) return false;
  out = Block<uint8_t>(s.size() / 2);
  for (size_t i = 0; i < s.size(); i += 2) {
    unsigned v = 0;
    if (sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
    out.get()[i / 2] = (uint8_t)v;
  }
  return true;
}

bool words_of(const std::string &s, Block<uint32_t> &out) {
  std::vector<uint32_t> v;
  if (s != "-") {
    const char *p = s.c_str();
    while (*p) {
      char *end = nullptr;
      const unsigned long long w = strtoull(p, &end, 10);
      if (end == p || w > 0xFFFFFFFFull) return false;
      v.push_back((uint32_t)w);
      p = end;
      if (*p == ',') ++p; else if (*p) return false;
    }
  }
  out = Block<uint32_t>(v.size());
  for (size_t i = 0; i < v.size(); ++i) out.get()[i] = v[i];
  return true;
}

void print_words(const uint32_t *w, size_t n) {
  if (!n) { printf("-"); return; }
  for (size_t i = 0; i < n; ++i) printf(i ? ",%u" : "%u", w[i]);
}

// the two storeys over vals[0, n), launch by launch (kd_self.hip: tree, top)
struct Trees {
  uint32_t B, nb, NB;
  Block<uint32_t> inner, top;
  Trees(const uint32_t *vals, uint32_t n, uint32_t B_) : B(B_), nb((n + B_ - 1) / B_), NB(1) {
    while (NB < nb) NB <<= 1;
    inner = Block<uint32_t>((size_t)nb * B);
    top = Block<uint32_t>((size_t)NB * 2);
    for (uint32_t k = 0; k < 2 * NB; ++k) top.get()[k] = NSV_PAD;
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t base = b * B;
      Block<uint32_t> t((size_t)2 * B);
      t.get()[0] = NSV_PAD;
      for (uint32_t i = 0; i < B; ++i) t.get()[B + i] = i < n - base ? vals[base + i] : NSV_PAD;
      for (uint32_t w = B / 2; w >= 1u; w >>= 1)
        for (uint32_t k = w; k < 2 * w; ++k) t.get()[k] = nsv_min(t.get()[2 * k], t.get()[2 * k + 1]);
      for (uint32_t i = 0; i < B; ++i) inner.get()[base + i] = t.get()[i];
      top.get()[NB + b] = t.get()[1];
    }
    for (uint32_t w = NB / 2; w >= 1u; w >>= 1)
      for (uint32_t k = w; k < 2 * w; ++k) top.get()[k] = nsv_min(top.get()[2 * k], top.get()[2 * k + 1]);
  }
};

// solve: every block's tree back into a block of its own, local answers there, far answers from the top tree
void solve(const uint32_t *vals, uint32_t n, const Trees &tr, uint32_t *psv, uint32_t *nsv) {
  const uint32_t B = tr.B;
  for (uint32_t b = 0; b < tr.nb; ++b) {
    const uint32_t base = b * B;
    Block<uint32_t> t((size_t)2 * B);
    for (uint32_t i = 0; i < B; ++i) {
      t.get()[i] = tr.inner.get()[base + i];
      t.get()[B + i] = i < n - base ? vals[base + i] : NSV_PAD;
    }
    for (uint32_t i = 0; i < B && i < n - base; ++i) {
      const uint32_t v = t.get()[B + i];
      const uint32_t p = nsv_tree_prev(t.get(), B, i, v), q = nsv_tree_next(t.get(), B, i, v);
      psv[base + i] = p != NSV_NONE ? base + p : nsv_far_prev(tr.top.get(), tr.NB, tr.inner.get(), vals, n, B, b, v);
      nsv[base + i] = q != NSV_NONE ? base + q : nsv_far_next(tr.top.get(), tr.NB, tr.inner.get(), vals, n, B, b, v);
    }
  }
}

bool block_size(uint32_t B) { return B == 4 || B == 8; }

int run(FILE *in) {
  std::string kind, w;
  while (read_word(in, kind)) {
    if (kind == "nsv") {
      Block<uint32_t> vals;
      if (!read_word(in, w)) return 3;
      const uint32_t B = (uint32_t)strtoul(w.c_str(), nullptr, 10);
      if (!block_size(B) || !read_word(in, w) || !words_of(w, vals) || vals.n == 0) return 3;
      const uint32_t n = (uint32_t)vals.n;
      Trees tr(vals.get(), n, B);
      Block<uint32_t> psv(n), nsv(n);
      solve(vals.get(), n, tr, psv.get(), nsv.get());
      printf("nsv ");
      print_words(psv.get(), n);
      printf(" ");
      print_words(nsv.get(), n);
      printf("\n");
    } else if (kind == "self") {
      uint32_t par[3];
      for (uint32_t &p : par) {
        if (!read_word(in, w)) return 3;
        p = (uint32_t)strtoul(w.c_str(), nullptr, 10);
      }
      const uint32_t B = par[0], min_len = par[1], max_len = par[2];
      Block<uint8_t> text;
      Block<uint32_t> sa;
      if (!block_size(B) || min_len < 1 || min_len > max_len || !read_word(in, w) || !from_hex(w, text) || text.n == 0) return 3;
      if (!read_word(in, w) || !words_of(w, sa) || sa.n != text.n) return 3;
      const uint32_t n = (uint32_t)text.n;
      for (uint32_t r = 0; r < n; ++r) if (sa.get()[r] >= n) return 3;
      // lpf: the solve kernel's second instantiation, at the text position and at its mirror
      Block<uint32_t> lpf(n), src(n), rlen(n), rsrc(n), psv(n), nsv(n);
      Block<uint8_t> rtext(n);
      if (n == 1) { lpf.get()[0] = rlen.get()[0] = 0; src.get()[0] = rsrc.get()[0] = NSV_NONE; }
      else {
        Trees tr(sa.get(), n, B);
        solve(sa.get(), n, tr, psv.get(), nsv.get());
        for (uint32_t r = 0; r < n; ++r) {
          const uint32_t i = sa.get()[r], p = psv.get()[r], q = nsv.get()[r];
          uint32_t s;
          const uint32_t l = lpf_pick(text.get(), n, i, p != NSV_NONE ? sa.get()[p] : NSV_NONE, q != NSV_NONE ? sa.get()[q] : NSV_NONE, max_len, &s);
          lpf.get()[i] = rlen.get()[self_mirror(n, i)] = l;
          src.get()[i] = rsrc.get()[self_mirror(n, i)] = s;
        }
      }
      for (uint32_t i = 0; i < n; ++i) rtext.get()[self_mirror(n, i)] = text.get()[i];
      // the chain over the mirrors, from the last mirrored position down; heads and runs by parse_step.h's rules
      Block<uint8_t> flag(n);
      memset(flag.get(), PARSE_NONE, n);
      for (uint32_t e = n - 1u;;) {
        const uint32_t l = rlen.get()[e];
        flag.get()[e] = parse_kind(l, min_len);
        const uint32_t nx = parse_next1(e, parse_jump(l, min_len));
        if (nx == 0u) break;
        e = nx - 1u;
      }
      std::vector<uint32_t> ops;
      std::vector<uint8_t> lits;
      uint64_t ncopies = 0;
      uint32_t run_len = 0;
      for (uint32_t e = 0; e < n; ++e) {
        const uint8_t f = flag.get()[e], right = e + 1u < n ? flag.get()[e + 1u] : PARSE_NONE;
        if (f == PARSE_LIT) { lits.push_back(rtext.get()[e]); ++run_len; }
        if (!parse_is_head(f, right)) continue;
        if (f == PARSE_COPY) { ops.push_back(rlen.get()[e]); ops.push_back(rsrc.get()[e]); ++ncopies; }
        else { ops.push_back(run_len); ops.push_back(PARSE_LITERAL); run_len = 0; }
      }
      // turned round: element k against element count - 1 - k
      const uint32_t nops = (uint32_t)(ops.size() / 2), nlits = (uint32_t)lits.size();
      for (uint32_t k = 0; k < nops / 2u; ++k) {
        const uint32_t m = self_mirror(nops, k);
        std::swap(ops[2 * k], ops[2 * m]);
        std::swap(ops[2 * k + 1], ops[2 * m + 1]);
      }
      for (uint32_t k = 0; k < nlits / 2u; ++k) std::swap(lits[k], lits[self_mirror(nlits, k)]);
      printf("self ");
      print_words(lpf.get(), n);
      printf(" ");
      print_words(src.get(), n);
      printf(" ");
      for (uint32_t k = 0; k < nops; ++k) printf(k ? ",%u:%u" : "%u:%u", ops[2 * k], ops[2 * k + 1]);
      printf(" ");
      if (lits.empty()) printf("-");
      for (uint8_t v : lits) printf("%02x", v);
      printf(" %u %u %llu %u\n", nops, nlits, (unsigned long long)ncopies, n - nlits);
    } else return 3;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!in) return 2;
  const int rc = run(in);
  if (in != stdin) fclose(in);
  return rc;
}
