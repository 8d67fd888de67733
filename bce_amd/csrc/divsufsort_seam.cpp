// divsufsort_seam.cpp -- libdivsufsort_hip.so: libdivsufsort's 32-bit entry points -- the two akamiru/bce calls (bce.cpp:901,
// :1091), divsufsort, bw_transform, sufcheck and the two searches -- under their original names and signatures
// (include/divsufsort_hip.h), served by libbcehip.so on one process-wide context.  Plain C++; everything GPU is behind
// bce_hip_divbwt / bce_hip_inverse_bwt / bce_hip_suffix_array / bce_hip_sufcheck; the searches are host code.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "../../include/bce_hip.h"
#include "../../include/divsufsort_hip.h"

namespace {
std::mutex g_mu;
bce_hip_ctx *g_ctx = nullptr;

bce_hip_ctx *context() {                       // g_mu held
  if (!g_ctx) {
    const char *e = getenv("BCE_HIP_DEVICE");
    if (bce_hip_create(&g_ctx, e ? atoi(e) : 0) != BCE_HIP_OK) g_ctx = nullptr;
  }
  return g_ctx;
}
int status_of(int rc) { return rc == BCE_HIP_OK ? 0 : (rc == BCE_HIP_E_ARG ? -1 : -2); }

// suffix T[at, Tsize) against P: < 0 the suffix sorts before every string that starts with P (a suffix that is a proper prefix of
// P included), 0 it starts with P, > 0 it sorts behind them
int compare_at(const sauchar_t *T, saidx_t Tsize, saidx_t at, const sauchar_t *P, saidx_t Psize) {
  if (at < 0 || at > Tsize) return -1;         // (no entry of a suffix array: nothing of T is read for it)
  const saidx_t have = Tsize - at, m = have < Psize ? have : Psize;
  const int r = m > 0 ? memcmp(T + at, P, (size_t)m) : 0;
  if (r) return r;
  return have < Psize ? -1 : 0;
}
// rows of SA[0, SAsize) whose suffix starts with P[0, Psize), Psize >= 1: the first row that is not below the matches, then the
// first that is above them
saidx_t search_rows(const sauchar_t *T, saidx_t Tsize, const sauchar_t *P, saidx_t Psize, const saidx_t *SA, saidx_t SAsize, saidx_t *idx) {
  saidx_t lo = 0, hi = SAsize;
  while (lo < hi) {
    const saidx_t mid = lo + (hi - lo) / 2;
    if (compare_at(T, Tsize, SA[mid], P, Psize) < 0) lo = mid + 1; else hi = mid;
  }
  const saidx_t left = lo;
  hi = SAsize;
  while (lo < hi) {
    const saidx_t mid = lo + (hi - lo) / 2;
    if (compare_at(T, Tsize, SA[mid], P, Psize) <= 0) lo = mid + 1; else hi = mid;
  }
  if (idx) *idx = left;
  return lo - left;
}
}  // namespace

extern "C" {

saidx_t divbwt(const sauchar_t *T, sauchar_t *U, saidx_t * /*A: workspace, not needed*/, saidx_t n) {
  if (!T || !U || n < 0) return -1;
  if (n == 0) return 0;
  if (n == 1) { U[0] = T[0]; return 1; }       // (libdivsufsort's own special case)
  std::lock_guard<std::mutex> g(g_mu);
  bce_hip_ctx *c = context();
  if (!c) return -2;
  uint32_t primary = 0;
  const int rc = bce_hip_divbwt(c, T, U, (uint32_t)n, &primary);
  return rc == BCE_HIP_OK ? (saidx_t)primary : (saidx_t)status_of(rc);
}

saint_t inverse_bw_transform(const sauchar_t *T, sauchar_t *U, saidx_t * /*A*/, saidx_t n, saidx_t idx) {
  if (!T || !U || n < 0 || idx < 0 || idx > n || (n > 0 && idx == 0)) return -1;
  if (n == 0) return 0;
  if (n == 1) { U[0] = T[0]; return 0; }
  std::lock_guard<std::mutex> g(g_mu);
  bce_hip_ctx *c = context();
  if (!c) return -2;
  return (saint_t)status_of(bce_hip_inverse_bwt(c, T, U, (uint32_t)n, (uint32_t)idx));
}

saint_t divsufsort(const sauchar_t *T, saidx_t *SA, saidx_t n) {
  if (!T || !SA || n < 0) return -1;
  if (n == 0) return 0;
  if (n == 1) { SA[0] = 0; return 0; }
  std::lock_guard<std::mutex> g(g_mu);
  bce_hip_ctx *c = context();
  if (!c) return -2;
  return (saint_t)status_of(bce_hip_suffix_array(c, T, (uint32_t)n, reinterpret_cast<uint32_t *>(SA), nullptr));
}

saint_t bw_transform(const sauchar_t *T, sauchar_t *U, saidx_t * /*SA: workspace, not needed*/, saidx_t n, saidx_t *idx) {
  if (!T || !U || !idx || n < 0) return -1;
  if (n <= 1) {
    if (n == 1) U[0] = T[0];
    *idx = n;
    return 0;
  }
  const saidx_t primary = divbwt(T, U, nullptr, n);
  if (primary < 0) return (saint_t)primary;
  *idx = primary;
  return 0;
}

saint_t sufcheck(const sauchar_t *T, const saidx_t *SA, saidx_t n, saint_t verbose) {
  if (!T || !SA || n < 0) {
    if (verbose) fprintf(stderr, "sufcheck: invalid arguments.\n");
    return -1;
  }
  if (n == 0) {
    if (verbose) fprintf(stderr, "sufcheck: 0 suffixes in order.\n");
    return 0;
  }
  uint64_t bad = 0;
  uint32_t reason = 0;
  {
    std::lock_guard<std::mutex> g(g_mu);
    bce_hip_ctx *c = context();
    const int rc = c ? bce_hip_sufcheck(c, T, reinterpret_cast<const uint32_t *>(SA), (uint32_t)n, &bad, &reason) : BCE_HIP_E_DEVICE;
    if (rc != BCE_HIP_OK) {
      if (verbose) fprintf(stderr, "sufcheck: not checked: %s\n", c ? bce_hip_last_error(c) : "no GPU context");
      return rc == BCE_HIP_E_ARG ? -1 : -5;
    }
  }
  switch (reason) {
    case BCE_HIP_SUFCHECK_OK:
      if (verbose) fprintf(stderr, "sufcheck: %d suffixes in order.\n", (int)n);
      return 0;
    case BCE_HIP_SUFCHECK_RANGE:
      if (verbose) fprintf(stderr, "sufcheck: out of the range [0,%d]: SA[%llu]=%d\n", (int)n - 1, (unsigned long long)bad, (int)SA[bad]);
      return -2;
    case BCE_HIP_SUFCHECK_MISSING:
      if (verbose) fprintf(stderr, "sufcheck: no row names text position %llu.\n", (unsigned long long)bad);
      return -4;
    default: {
      const saidx_t a = SA[bad - 1], b = SA[bad];
      const bool first = T[a] > T[b];
      if (verbose) fprintf(stderr, first ? "sufcheck: suffixes in wrong order: row %llu, first bytes T[SA[%llu]=%d]=%d > T[SA[%llu]=%d]=%d\n"
                                         : "sufcheck: suffixes in wrong order: row %llu, SA[%llu]=%d (byte %d) stands above SA[%llu]=%d (byte %d)\n",
                           (unsigned long long)bad, (unsigned long long)bad - 1, (int)a, (int)T[a], (unsigned long long)bad, (int)b, (int)T[b]);
      return first ? -3 : -4;
    }
  }
}

saidx_t sa_search(const sauchar_t *T, saidx_t Tsize, const sauchar_t *P, saidx_t Psize, const saidx_t *SA, saidx_t SAsize, saidx_t *idx) {
  if (idx) *idx = -1;
  if (!T || !P || !SA || Tsize < 0 || Psize < 0 || SAsize < 0) return -1;
  if (Tsize == 0 || SAsize == 0) return 0;
  if (Psize == 0) { if (idx) *idx = 0; return SAsize; }
  return search_rows(T, Tsize, P, Psize, SA, SAsize, idx);
}

saidx_t sa_simplesearch(const sauchar_t *T, saidx_t Tsize, const saidx_t *SA, saidx_t SAsize, saint_t c, saidx_t *idx) {
  if (idx) *idx = -1;
  if (!T || !SA || Tsize < 0 || SAsize < 0) return -1;
  if (Tsize == 0 || SAsize == 0) return 0;
  const sauchar_t byte = (sauchar_t)c;
  return search_rows(T, Tsize, &byte, 1, SA, SAsize, idx);
}

const char *divsufsort_version(void) { return "2.0.1-hip"; }

}  // extern "C"
