// maxrep_emul.cpp -- TEST-ONLY: the rules kd_maxrep.hip shares with the host (bce_amd/csrc/maxrep_step.h) driven through the kernels'
// block decomposition with a block of B = 4 or 8 rows, so that local and far answers, the top tree, the prefix count's carry and the
// selection cross blocks on inputs of tens of rows (tests/test_maxrep_cpu.py compares with tests/maxrep_ref.py).  A stand-alone
// program, so that it can run under ASan + UBSan; the rows, the bytes, every tree and the 64 counters are heap blocks of exactly
// their size.
//   input (a file, or stdin), words:
//     "rows B min_len max_len order limit" <lcp "v,v,.."> <bw "v,v,..">
//     "sel limit" <weights "w,w,..">                       (decimal, up to 2^64 - 1, all >= 1)
//   output, one line each:
//     "rows <total> <capped> <bwt_runs> <found> <entries "len:count:first:row,..">"      the list as the device orders it
//     "sel <t> <candidates> <top> <bits> <found> <indices "i,i,..">"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../bce_amd/csrc/maxrep_step.h"

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

bool numbers_of(const std::string &s, std::vector<uint64_t> &v) {
  v.clear();
  if (s == "-") return true;
  const char *p = s.c_str();
  while (*p) {
    char *end = nullptr;
    v.push_back(strtoull(p, &end, 10));
    if (end == p) return false;
    p = end;
    if (*p == ',') ++p; else if (*p) return false;
  }
  return true;
}

bool read_number(FILE *f, uint64_t *v) {
  std::string w;
  if (!read_word(f, w)) return false;
  char *end = nullptr;
  *v = strtoull(w.c_str(), &end, 10);
  return end && *end == 0;
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

// The selection on the weights wt[0, n) (0: the row represents nothing), as kd_maxrep.hip runs it; the chosen rows through *rows.
int select_rows(const uint64_t *wt, size_t n, uint64_t limit, std::vector<size_t> *rows, int *t_out, uint64_t *cand_out, int *top_out, uint32_t *bits_out,
                uint64_t *total_out) {
  uint64_t *H = static_cast<uint64_t *>(calloc(kMxrBins, sizeof(uint64_t)));   // exactly the counters the header speaks of
  if (!H) return 2;
  for (size_t r = 0; r < n; ++r) if (wt[r]) H[mxr_bin(wt[r])] += 1;
  const uint64_t total = mxr_total(H), want = total < limit ? total : limit;
  *total_out = total;
  rows->clear();
  *t_out = 0; *cand_out = 0; *top_out = 0; *bits_out = 0;
  if (!total) { free(H); return 0; }
  uint64_t cand = 0;
  int top = 0;
  const int t = mxr_threshold(H, want, &cand, &top);
  free(H);
  const uint32_t bits = mxr_key_bits(t, top);
  const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
  std::vector<std::pair<uint64_t, size_t>> pairs;                     // (key, row), in row order
  for (size_t r = 0; r < n; ++r) if (wt[r] >> t) pairs.emplace_back(mxr_key(top, wt[r]), r);
  if (pairs.size() != cand) return 4;                                 // the histogram's count is the candidates' count, exactly
  for (const auto &p : pairs) if ((p.first & mask) != p.first) return 4;   // no key has a bit above the sorted ones
  std::stable_sort(pairs.begin(), pairs.end(), [&](const auto &a, const auto &b) { return (a.first & mask) < (b.first & mask); });
  const uint64_t found = want < cand ? want : cand;
  for (uint64_t e = 0; e < found; ++e) rows->push_back(pairs[e].second);
  *t_out = t; *cand_out = cand; *top_out = top; *bits_out = bits;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string w;
  while (read_word(f, w)) {
    std::vector<uint64_t> nums;
    std::vector<size_t> rows;
    int t = 0, top = 0;
    uint32_t bits = 0;
    uint64_t cand = 0, total = 0;
    if (w == "sel") {
      uint64_t limit = 0;
      if (!read_number(f, &limit) || limit < 1 || !read_word(f, w) || !numbers_of(w, nums)) return 3;
      Block<uint64_t> wt(nums.size());
      for (size_t i = 0; i < nums.size(); ++i) { if (!nums[i]) return 3; wt.get()[i] = nums[i]; }
      if (const int rc = select_rows(wt.get(), nums.size(), limit, &rows, &t, &cand, &top, &bits, &total)) return rc;
      printf("sel %d %llu %d %u %zu ", t, (unsigned long long)cand, top, bits, rows.size());
      if (rows.empty()) printf("-");
      for (size_t e = 0; e < rows.size(); ++e) printf(e ? ",%zu" : "%zu", rows[e]);
      printf("\n");
      continue;
    }
    if (w != "rows") return 3;
    uint64_t B = 0, min_len = 0, max_len = 0, order = 0, limit = 0;
    if (!read_number(f, &B) || !read_number(f, &min_len) || !read_number(f, &max_len) || !read_number(f, &order) || !read_number(f, &limit)) return 3;
    if ((B != 4 && B != 8) || min_len < 1 || order > 2 || limit < 1) return 3;
    std::vector<uint64_t> bwn;
    if (!read_word(f, w) || !numbers_of(w, nums) || !read_word(f, w) || !numbers_of(w, bwn) || nums.size() != bwn.size() || nums.empty()) return 3;
    const uint32_t n = (uint32_t)nums.size();
    Block<uint32_t> vals(n), D(n), first(n);
    Block<uint8_t> bw(n);
    Block<uint64_t> wt(n);
    for (uint32_t r = 0; r < n; ++r) { vals.get()[r] = (uint32_t)nums[r]; bw.get()[r] = (uint8_t)bwn[r]; }
    // change: the count inside every block, the blocks' counts carried, the carry added
    const uint32_t nb = (n + (uint32_t)B - 1) / (uint32_t)B;
    Block<uint64_t> bsum(nb);
    for (uint32_t b = 0; b < nb; ++b) {
      uint32_t cnt = 0;
      for (uint32_t r = b * (uint32_t)B; r < n && r < (b + 1) * (uint32_t)B; ++r) {
        cnt += r > 0 && bw.get()[r] != bw.get()[r - 1];
        D.get()[r] = cnt;
      }
      bsum.get()[b] = cnt;
    }
    uint64_t carry = 0;
    for (uint32_t b = 0; b < nb; ++b) { const uint64_t s = bsum.get()[b]; bsum.get()[b] = carry; carry += s; }
    for (uint32_t r = 0; r < n; ++r) D.get()[r] += (uint32_t)bsum.get()[r / (uint32_t)B];
    // solve: every block's tree into a block of its own
    const Trees tr(vals.get(), n, (uint32_t)B);
    uint64_t capped = 0;
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t base = b * (uint32_t)B;
      Block<uint32_t> tt((size_t)2 * B);
      for (uint32_t i = 0; i < B; ++i) {
        tt.get()[i] = tr.inner.get()[base + i];
        tt.get()[B + i] = i < n - base ? vals.get()[base + i] : NSV_PAD;
      }
      for (uint32_t i = 0; i < B && i < n - base; ++i) {
        uint32_t p = 0;
        const uint64_t wgt = mxr_row(tt.get(), (uint32_t)B, i, b, tr.top.get(), tr.NB, tr.inner.get(), vals.get(), n, D.get(), (uint32_t)min_len,
                                     (uint32_t)order, &p);
        wt.get()[base + i] = wgt;
        first.get()[base + i] = wgt ? p : NSV_NONE;
        capped += wgt && vals.get()[base + i] == max_len;
      }
    }
    if (const int rc = select_rows(wt.get(), n, limit, &rows, &t, &cand, &top, &bits, &total)) return rc;
    printf("rows %llu %llu %llu %zu ", (unsigned long long)total, (unsigned long long)capped, (unsigned long long)(carry + 1), rows.size());
    if (rows.empty()) printf("-");
    for (size_t e = 0; e < rows.size(); ++e) {
      const size_t r = rows[e];
      const uint32_t len = vals.get()[r];
      if (mxr_weight((uint32_t)order, len, mxr_count_of((uint32_t)order, wt.get()[r], len)) != wt.get()[r]) return 4;   // the count comes back from the weight
      printf(e ? ",%u:%u:%u:%zu" : "%u:%u:%u:%zu", len, mxr_count_of((uint32_t)order, wt.get()[r], len), first.get()[r], r);
    }
    printf("\n");
  }
  if (f != stdin) fclose(f);
  return 0;
}
