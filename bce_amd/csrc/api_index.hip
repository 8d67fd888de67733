// api_index.hip -- C ABI of the index queries (include/bce_hip.h): counts and positions; the same two within k mismatches
// (kd_near.hip), within k edits (kd_edit.hip) and for patterns of byte classes (kd_classes.hip); longest matches and coverage,
// the LCP array and its reductions, the list of the most frequent k-grams, parse and patch, the longest previous factors and the
// self-parse; and the test hooks that run their block scans alone.  The device work is in kd_count / kd_locate / kd_near /
// kd_edit / kd_classes / kd_match / kd_lcp / kd_parse / kd_self.hip.  Every query comes twice, for host buffers and for device
// buffers: the two differ in staging and in the copy out, and in nothing else.
//
// All of them judge the arguments before the context's state and the state before the arrays, then run their body through
// query_call in phase 3, as bce_hip_rank1: the planes are read, so what an allocation may give back is what an enumeration beside
// them would.  Nothing a stage keeps is written: staging, scratch and result words are the queries' own (common.h: qb).
#include "common.h"
#include "parse_step.h"

using namespace bce;

// The body of a query: no exception leaves, the context's device is current, `phase` holds while it runs, and whatever the body
// has queued is complete -- and has left no error behind -- when BCE_HIP_OK comes back.
template <class F>
static int query_call(bce_hip_ctx *c, int phase, F &&body) {
  return bce_guarded(c, [&]() -> int {
    BCE_HIP_TRY(c, hipSetDevice(c->device));
    PhaseScope scope(c, phase);
    BCE_TRY(body());
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
    BCE_HIP_TRY(c, hipGetLastError());
    return BCE_HIP_OK;
  });
}

// `bytes` of the caller's host memory into a grow-only buffer of the context (never an empty allocation); queued
static int stage(bce_hip_ctx *c, DevBuf &b, const void *host, size_t bytes) {
  BCE_TRY(ensure(c, b, bytes ? bytes : 1));
  if (bytes) BCE_HIP_TRY(c, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, c->stream));
  return BCE_HIP_OK;
}
static int stage_patterns(bce_hip_ctx *c, DevBuf &pat, DevBuf &off, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat) {
  BCE_TRY(stage(c, pat, patterns, (size_t)offsets[npat]));
  return stage(c, off, offsets, ((size_t)npat + 1) * 8);
}
static int copy_out(bce_hip_ctx *c, void *host, const DevBuf &b, size_t bytes) {
  if (bytes) BCE_HIP_TRY(c, hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, c->stream));
  return BCE_HIP_OK;
}

// a list of npat >= 1 patterns in host memory: offsets that do not decrease, and bytes where they name some
static int pattern_list_args(bce_hip_ctx *c, const char *what, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat) {
  if (!offsets) return BCE_HIP_E_ARG;
  for (uint32_t p = 0; p < npat; ++p)
    if (offsets[p + 1] < offsets[p]) { snprintf(c->err, sizeof c->err, "%s: pattern offsets decrease at %u", what, p); return BCE_HIP_E_ARG; }
  return offsets[npat] && !patterns ? BCE_HIP_E_ARG : BCE_HIP_OK;
}
static int length_bound(bce_hip_ctx *c, const char *what, uint32_t max_len) {
  if (max_len >= 1 && max_len <= BCE_HIP_MATCH_MAX_LEN) return BCE_HIP_OK;
  snprintf(c->err, sizeof c->err, "%s: a length bound of %u, outside 1 .. %u", what, max_len, BCE_HIP_MATCH_MAX_LEN);
  return BCE_HIP_E_ARG;
}

// ---- what a query needs of the context ---------------------------------------------------------------------------------------------
static int planes_state(bce_hip_ctx *c, const char *what) {
  if (c->stage >= 3) return BCE_HIP_OK;
  snprintf(c->err, sizeof c->err, "%s: the context holds no planes (stage %d; bce_hip_build_planes first)", what, c->stage);
  return BCE_HIP_E_STATE;
}
// The planes and K1's suffix array.  ctx_trim keeps sa[sa_res] in phase 3, for the depth-first tail, and nothing after K1 writes
// that array until the next load or decode (K3's tail, the encoder, the estimate, the scan, the queries and the sort hooks only read
// it or never name it), so it stands for as long as k1_valid does.  A text of one byte has no array: its only rotation starts at 0.
static int sa_state(bce_hip_ctx *c, const uint32_t **sa, const char *what) {
  BCE_TRY(planes_state(c, what));
  *sa = nullptr;
  if (c->k1_valid && c->sa[c->sa_res].p && c->sa[c->sa_res].cap >= (size_t)c->n * 4) { *sa = c->sa[c->sa_res].as<uint32_t>(); return BCE_HIP_OK; }
  if (c->n == 1 && c->text_loaded) return BCE_HIP_OK;
  snprintf(c->err, sizeof c->err, c->text_loaded ? "%s: the suffix array of this input is gone" : "%s: there is no suffix array behind an injected BWT", what);
  return BCE_HIP_E_STATE;
}
// ... and the text itself
static int text_state(bce_hip_ctx *c, const uint32_t **sa, const char *what) {
  BCE_TRY(sa_state(c, sa, what));
  if (c->text_loaded && c->text.p && c->text.cap >= (size_t)c->n) return BCE_HIP_OK;
  snprintf(c->err, sizeof c->err, "%s: there is no suffix array behind an injected BWT", what);
  return BCE_HIP_E_STATE;
}

extern "C" {

// ---- test hooks: the block scans of the index queries alone (kd_lcp.hip, kd_match.hip) ----------------------------
// Phase 0, as the sort hooks: nothing of the context is given back to make room, and only the features' own rep_* / mat_* buffers
// are written.  The LCP words are copied into rep_lcp first: the reductions load them sixteen bytes at a time from there.
int bce_hip_lcp_reduce_device(bce_hip_ctx *c, const void *d_lcp, uint32_t n, const void *d_sa, const uint32_t *ks, uint32_t nk,
                              bce_hip_kgram *out, uint32_t repeat3[3]) {
  if (!c || !d_lcp || !d_sa || n == 0 || n > 0x7FFFFFFFu || nk > BCE_HIP_KGRAMS_MAX || (nk && (!ks || !out))) return BCE_HIP_E_ARG;
  return query_call(c, 0, [&]() -> int {
    DevBuf &lcp = c->qbuf[qb::rep_lcp];
    const size_t words = (size_t)n * 4;
    BCE_TRY(ensure(c, lcp, words));
    BCE_HIP_TRY(c, hipMemcpyAsync(lcp.p, d_lcp, words, hipMemcpyDeviceToDevice, c->stream));
    const uint32_t *sa = static_cast<const uint32_t *>(d_sa);
    if (nk) BCE_TRY(kd_kgrams(c, sa, lcp.as<uint32_t>(), n, ks, nk, out));
    if (repeat3) BCE_TRY(kd_longest_repeat(c, sa, lcp.as<uint32_t>(), n, repeat3));
    return BCE_HIP_OK;
  });
}

// the selection of bce_hip_top_kgrams alone: the entries are staged in top_out, as a call with host buffers stages them
int bce_hip_top_classes_of_lcp_device(bce_hip_ctx *c, const void *d_lcp, uint32_t n, const void *d_sa, uint32_t k, uint32_t limit,
                                      bce_hip_top_kgram *out, uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]) {
  if (!c || !d_lcp || !d_sa || !out || !found || n == 0 || n > 0x7FFFFFFFu || k > BCE_HIP_MATCH_MAX_LEN || limit < 1 || limit > BCE_HIP_TOP_MAX) return BCE_HIP_E_ARG;
  uint32_t got = 0;
  uint64_t classes = 0, hist[32];
  BCE_TRY(query_call(c, 0, [&]() -> int {
    DevBuf &lcp = c->qbuf[qb::rep_lcp], &ent = c->qbuf[qb::top_out];
    const size_t words = (size_t)n * 4;
    BCE_TRY(ensure(c, lcp, words));
    BCE_TRY(ensure(c, ent, (size_t)(limit < n ? limit : n) * sizeof(bce_hip_top_kgram)));
    BCE_HIP_TRY(c, hipMemcpyAsync(lcp.p, d_lcp, words, hipMemcpyDeviceToDevice, c->stream));
    BCE_TRY(kd_top_kgrams(c, static_cast<const uint32_t *>(d_sa), lcp.as<uint32_t>(), n, nullptr, k, limit, ent.as<bce_hip_top_kgram>(), nullptr, &got,
                          &classes, hist));
    return copy_out(c, out, ent, (size_t)got * sizeof(bce_hip_top_kgram));
  }));
  *found = got;
  if (distinct) *distinct = classes;
  if (size_hist) memcpy(size_hist, hist, sizeof hist);
  return BCE_HIP_OK;
}

int bce_hip_coverage_of_lengths_device(bce_hip_ctx *c, const void *d_len, uint64_t q, uint32_t min_len, uint64_t *covered) {
  if (!c || !covered || q > 0x7FFFFFFFull || min_len < 1 || min_len > BCE_HIP_MATCH_MAX_LEN || (q && !d_len)) return BCE_HIP_E_ARG;
  return query_call(c, 0, [&] { return kd_coverage(c, static_cast<const uint32_t *>(d_len), (uint32_t)q, min_len, covered); });
}

// ---- pattern counts from the planes (kd_count.hip) ---------------------------------------------------------
int bce_hip_count(bce_hip_ctx *c, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint64_t *counts) {
  if (!c) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(planes_state(c, "count"));
  if (!counts) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "count", patterns, offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &pat = c->qbuf[qb::cnt_pat], &off = c->qbuf[qb::cnt_off], &out = c->qbuf[qb::cnt_out];
    BCE_TRY(ensure(c, out, (size_t)npat * 8));
    BCE_TRY(stage_patterns(c, pat, off, patterns, offsets, npat));
    BCE_TRY(kd_count(c, pat.as<uint8_t>(), off.as<uint64_t>(), npat, out.as<uint64_t>()));
    return copy_out(c, counts, out, (size_t)npat * 8);
  });
}

int bce_hip_count_device(bce_hip_ctx *c, const void *d_patterns, const void *d_offsets, uint32_t npat, void *d_counts) {
  if (!c) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(planes_state(c, "count"));
  if (!d_patterns || !d_offsets || !d_counts) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return kd_count(c, static_cast<const uint8_t *>(d_patterns), static_cast<const uint64_t *>(d_offsets), npat, static_cast<uint64_t *>(d_counts));
  });
}

// ---- pattern positions from the planes and K1's suffix array (kd_locate.hip) -----------------------------------------------
// The overflow protocol, once for both entry points.  d_*: device arrays; h_hits / h_pos: where a call with host buffers wants the
// offsets and positions (then d_pos is staged in loc_pos once the total is known).  hit offsets and *total are out before the
// first reason to refuse; the positions are touched only when all of them fit.
static int locate_run(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, bool linear, uint64_t *d_hits,
                      uint64_t *h_hits, uint32_t *d_pos, uint32_t *h_pos, bool sizing, uint64_t cap, uint64_t *total) {
  uint64_t rows = 0, hits = 0;
  const int rc = kd_locate_size(c, sa, d_pat, d_off, npat, linear, d_hits, &rows, &hits);
  if (rc != BCE_HIP_OK && rc != BCE_HIP_E_OVERFLOW) return rc;
  if (h_hits) {
    BCE_HIP_TRY(c, hipMemcpyAsync(h_hits, d_hits, ((size_t)npat + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *total = hits;
  if (rc != BCE_HIP_OK || sizing) return rc;
  if (hits > cap) { snprintf(c->err, sizeof c->err, "locate: %llu hits, room for %llu", (unsigned long long)hits, (unsigned long long)cap); return BCE_HIP_E_OVERFLOW; }
  if (hits == 0) return BCE_HIP_OK;
  if (h_pos) {
    BCE_TRY(ensure(c, c->qbuf[qb::loc_pos], (size_t)hits * 4));
    d_pos = c->qbuf[qb::loc_pos].as<uint32_t>();
  }
  BCE_TRY(kd_locate_fill(c, sa, d_off, npat, linear, rows, hits, d_pos));
  return h_pos ? copy_out(c, h_pos, c->qbuf[qb::loc_pos], (size_t)hits * 4) : BCE_HIP_OK;
}

int bce_hip_locate(bce_hip_ctx *c, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t flags, uint64_t *hit_offsets,
                   uint32_t *positions, uint64_t cap, uint64_t *total) {
  if (!c || !total || (flags & ~BCE_HIP_LOCATE_LINEAR)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) { if (hit_offsets) hit_offsets[0] = 0; return BCE_HIP_OK; }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate"));
  if (!hit_offsets || (!positions && cap)) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "locate", patterns, offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &pat = c->qbuf[qb::loc_pat], &off = c->qbuf[qb::loc_off], &hits = c->qbuf[qb::loc_hits];
    BCE_TRY(ensure(c, hits, ((size_t)npat + 1) * 8));
    BCE_TRY(stage_patterns(c, pat, off, patterns, offsets, npat));
    return locate_run(c, sa, pat.as<uint8_t>(), off.as<uint64_t>(), npat, flags & BCE_HIP_LOCATE_LINEAR, hits.as<uint64_t>(), hit_offsets, nullptr,
                      positions, !positions, cap, total);
  });
}

int bce_hip_locate_device(bce_hip_ctx *c, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t flags, void *d_hit_offsets,
                          void *d_positions, uint64_t cap, uint64_t *total) {
  if (!c || !total || (flags & ~BCE_HIP_LOCATE_LINEAR)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) {
    if (!d_hit_offsets) return BCE_HIP_OK;
    return query_call(c, 0, [&]() -> int { BCE_HIP_TRY(c, hipMemsetAsync(d_hit_offsets, 0, 8, c->stream)); return BCE_HIP_OK; });
  }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate"));
  if (!d_patterns || !d_offsets || !d_hit_offsets || (!d_positions && cap)) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return locate_run(c, sa, static_cast<const uint8_t *>(d_patterns), static_cast<const uint64_t *>(d_offsets), npat, flags & BCE_HIP_LOCATE_LINEAR,
                      static_cast<uint64_t *>(d_hit_offsets), nullptr, static_cast<uint32_t *>(d_positions), nullptr, !d_positions, cap, total);
  });
}

// ---- counts and positions within k mismatches (kd_near.hip) ----------------------------------------------------------------------
// The count's and the locate's rules, checks and protocol; k is judged beside ctx and the flags, the patterns' lengths with the list.
static int near_lengths(bce_hip_ctx *c, const char *what, const uint64_t *offsets, uint32_t npat) {
  for (uint32_t p = 0; p < npat; ++p)
    if (offsets[p + 1] - offsets[p] > BCE_HIP_NEAR_MAX_LEN) {
      snprintf(c->err, sizeof c->err, "%s: pattern %u has %llu bytes, more than %u", what, p, (unsigned long long)(offsets[p + 1] - offsets[p]), BCE_HIP_NEAR_MAX_LEN);
      return BCE_HIP_E_ARG;
    }
  return BCE_HIP_OK;
}

int bce_hip_count_near(bce_hip_ctx *c, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint64_t *counts) {
  if (!c || k > BCE_HIP_NEAR_MAX_K) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(planes_state(c, "count_near"));
  if (!counts) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "count_near", patterns, offsets, npat));
  BCE_TRY(near_lengths(c, "count_near", offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &pat = c->qbuf[qb::near_pat], &off = c->qbuf[qb::near_off], &out = c->qbuf[qb::near_out];
    const size_t bytes = (size_t)npat * (k + 1) * 8;
    BCE_TRY(ensure(c, out, bytes));
    BCE_TRY(stage_patterns(c, pat, off, patterns, offsets, npat));
    BCE_TRY(kd_near_count(c, pat.as<uint8_t>(), off.as<uint64_t>(), npat, k, out.as<uint64_t>()));
    return copy_out(c, counts, out, bytes);
  });
}

int bce_hip_count_near_device(bce_hip_ctx *c, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, void *d_counts) {
  if (!c || k > BCE_HIP_NEAR_MAX_K) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(planes_state(c, "count_near"));
  if (!d_patterns || !d_offsets || !d_counts) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return kd_near_count(c, static_cast<const uint8_t *>(d_patterns), static_cast<const uint64_t *>(d_offsets), npat, k, static_cast<uint64_t *>(d_counts));
  });
}

// locate_run with the distances beside the positions
static int locate_near_run(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                           uint64_t *d_hits, uint64_t *h_hits, uint32_t *d_pos, uint8_t *d_dist, uint32_t *h_pos, uint8_t *h_dist, bool sizing,
                           uint64_t cap, uint64_t *total) {
  uint64_t rows = 0, hits = 0;
  const int rc = kd_near_size(c, sa, d_pat, d_off, npat, k, linear, d_hits, &rows, &hits);
  if (rc != BCE_HIP_OK && rc != BCE_HIP_E_OVERFLOW) return rc;
  if (h_hits) {
    BCE_HIP_TRY(c, hipMemcpyAsync(h_hits, d_hits, ((size_t)npat + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *total = hits;
  if (rc != BCE_HIP_OK || sizing) return rc;
  if (hits > cap) { snprintf(c->err, sizeof c->err, "locate_near: %llu hits, room for %llu", (unsigned long long)hits, (unsigned long long)cap); return BCE_HIP_E_OVERFLOW; }
  if (hits == 0) return BCE_HIP_OK;
  if (h_pos) {
    BCE_TRY(ensure(c, c->qbuf[qb::near_pos], (size_t)hits * 4));
    BCE_TRY(ensure(c, c->qbuf[qb::near_dist], (size_t)hits));
    d_pos = c->qbuf[qb::near_pos].as<uint32_t>();
    d_dist = c->qbuf[qb::near_dist].as<uint8_t>();
  }
  BCE_TRY(kd_near_fill(c, sa, d_pat, d_off, npat, k, linear, rows, hits, d_pos, d_dist));
  if (!h_pos) return BCE_HIP_OK;
  BCE_TRY(copy_out(c, h_pos, c->qbuf[qb::near_pos], (size_t)hits * 4));
  return copy_out(c, h_dist, c->qbuf[qb::near_dist], (size_t)hits);
}

int bce_hip_locate_near(bce_hip_ctx *c, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                        uint64_t *hit_offsets, uint32_t *positions, uint8_t *dists, uint64_t cap, uint64_t *total) {
  if (!c || !total || (flags & ~BCE_HIP_LOCATE_LINEAR) || k > BCE_HIP_NEAR_MAX_K || npat > (1u << 30)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) { if (hit_offsets) hit_offsets[0] = 0; return BCE_HIP_OK; }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate_near"));
  if (!hit_offsets || (!positions && cap) || !positions != !dists) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "locate_near", patterns, offsets, npat));
  BCE_TRY(near_lengths(c, "locate_near", offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &pat = c->qbuf[qb::near_pat], &off = c->qbuf[qb::near_off], &hits = c->qbuf[qb::near_hits];
    BCE_TRY(ensure(c, hits, ((size_t)npat + 1) * 8));
    BCE_TRY(stage_patterns(c, pat, off, patterns, offsets, npat));
    return locate_near_run(c, sa, pat.as<uint8_t>(), off.as<uint64_t>(), npat, k, flags & BCE_HIP_LOCATE_LINEAR, hits.as<uint64_t>(), hit_offsets,
                           nullptr, nullptr, positions, dists, !positions, cap, total);
  });
}

int bce_hip_locate_near_device(bce_hip_ctx *c, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, uint32_t flags,
                               void *d_hit_offsets, void *d_positions, void *d_dists, uint64_t cap, uint64_t *total) {
  if (!c || !total || (flags & ~BCE_HIP_LOCATE_LINEAR) || k > BCE_HIP_NEAR_MAX_K || npat > (1u << 30)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) {
    if (!d_hit_offsets) return BCE_HIP_OK;
    return query_call(c, 0, [&]() -> int { BCE_HIP_TRY(c, hipMemsetAsync(d_hit_offsets, 0, 8, c->stream)); return BCE_HIP_OK; });
  }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate_near"));
  if (!d_patterns || !d_offsets || !d_hit_offsets || (!d_positions && cap) || !d_positions != !d_dists) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return locate_near_run(c, sa, static_cast<const uint8_t *>(d_patterns), static_cast<const uint64_t *>(d_offsets), npat, k,
                           flags & BCE_HIP_LOCATE_LINEAR, static_cast<uint64_t *>(d_hit_offsets), nullptr, static_cast<uint32_t *>(d_positions),
                           static_cast<uint8_t *>(d_dists), nullptr, nullptr, !d_positions, cap, total);
  });
}

// ---- counts and positions within k edits (kd_edit.hip) ------------------------------------------------------------------------------
// The near calls' rules, checks and protocol; k, the flags and npat's cap are judged beside ctx, the patterns' lengths with the list.
// Both need the suffix array: the hits are reduced from candidates by position.
static bool edit_args(uint32_t npat, uint32_t k, uint32_t flags) {
  return !(flags & ~BCE_HIP_LOCATE_LINEAR) && k <= BCE_HIP_EDIT_MAX_K && npat <= BCE_HIP_EDIT_MAX_PATTERNS;
}
static int edit_lengths(bce_hip_ctx *c, const char *what, const uint64_t *offsets, uint32_t npat) {
  for (uint32_t p = 0; p < npat; ++p)
    if (offsets[p + 1] - offsets[p] > BCE_HIP_EDIT_MAX_LEN) {
      snprintf(c->err, sizeof c->err, "%s: pattern %u has %llu bytes, more than %u", what, p, (unsigned long long)(offsets[p + 1] - offsets[p]), BCE_HIP_EDIT_MAX_LEN);
      return BCE_HIP_E_ARG;
    }
  return BCE_HIP_OK;
}

int bce_hip_count_edit(bce_hip_ctx *c, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags, uint64_t *counts) {
  if (!c || !edit_args(npat, k, flags)) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "count_edit"));
  if (!counts) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "count_edit", patterns, offsets, npat));
  BCE_TRY(edit_lengths(c, "count_edit", offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &pat = c->qbuf[qb::edit_pat], &off = c->qbuf[qb::edit_off], &out = c->qbuf[qb::edit_out];
    const size_t bytes = (size_t)npat * (k + 1) * 8;
    BCE_TRY(ensure(c, out, bytes));
    BCE_TRY(stage_patterns(c, pat, off, patterns, offsets, npat));
    BCE_TRY(kd_edit_count(c, sa, pat.as<uint8_t>(), off.as<uint64_t>(), npat, k, flags & BCE_HIP_LOCATE_LINEAR, out.as<uint64_t>()));
    return copy_out(c, counts, out, bytes);
  });
}

int bce_hip_count_edit_device(bce_hip_ctx *c, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, uint32_t flags, void *d_counts) {
  if (!c || !edit_args(npat, k, flags)) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "count_edit"));
  if (!d_patterns || !d_offsets || !d_counts) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return kd_edit_count(c, sa, static_cast<const uint8_t *>(d_patterns), static_cast<const uint64_t *>(d_offsets), npat, k,
                         flags & BCE_HIP_LOCATE_LINEAR, static_cast<uint64_t *>(d_counts));
  });
}

// locate_near_run with the lengths beside the positions and distances; the sizing is the whole search and reduce
static int locate_edit_run(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                           uint64_t *d_hits, uint64_t *h_hits, uint32_t *d_pos, uint16_t *d_len, uint8_t *d_dist, uint32_t *h_pos, uint16_t *h_len,
                           uint8_t *h_dist, bool sizing, uint64_t cap, uint64_t *total) {
  uint64_t hits = 0;
  const uint32_t *pos = nullptr, *tag = nullptr;
  BCE_TRY(kd_edit_size(c, sa, d_pat, d_off, npat, k, linear, d_hits, &hits, &pos, &tag));
  if (h_hits) {
    BCE_HIP_TRY(c, hipMemcpyAsync(h_hits, d_hits, ((size_t)npat + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *total = hits;
  if (sizing) return BCE_HIP_OK;
  if (hits > cap) { snprintf(c->err, sizeof c->err, "locate_edit: %llu hits, room for %llu", (unsigned long long)hits, (unsigned long long)cap); return BCE_HIP_E_OVERFLOW; }
  if (hits == 0) return BCE_HIP_OK;
  if (h_pos) {
    BCE_TRY(ensure(c, c->qbuf[qb::edit_pos], (size_t)hits * 4));
    BCE_TRY(ensure(c, c->qbuf[qb::edit_len], (size_t)hits * 2));
    BCE_TRY(ensure(c, c->qbuf[qb::edit_dist], (size_t)hits));
    d_pos = c->qbuf[qb::edit_pos].as<uint32_t>();
    d_len = c->qbuf[qb::edit_len].as<uint16_t>();
    d_dist = c->qbuf[qb::edit_dist].as<uint8_t>();
  }
  BCE_TRY(kd_edit_fill(c, d_off, npat, k, d_hits, hits, pos, tag, d_pos, d_len, d_dist));
  if (!h_pos) return BCE_HIP_OK;
  BCE_TRY(copy_out(c, h_pos, c->qbuf[qb::edit_pos], (size_t)hits * 4));
  BCE_TRY(copy_out(c, h_len, c->qbuf[qb::edit_len], (size_t)hits * 2));
  return copy_out(c, h_dist, c->qbuf[qb::edit_dist], (size_t)hits);
}

int bce_hip_locate_edit(bce_hip_ctx *c, const uint8_t *patterns, const uint64_t *offsets, uint32_t npat, uint32_t k, uint32_t flags,
                        uint64_t *hit_offsets, uint32_t *positions, uint16_t *lens, uint8_t *dists, uint64_t cap, uint64_t *total) {
  if (!c || !total || !edit_args(npat, k, flags)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) { if (hit_offsets) hit_offsets[0] = 0; return BCE_HIP_OK; }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate_edit"));
  if (!hit_offsets || (!positions && cap) || !positions != !dists || !positions != !lens) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "locate_edit", patterns, offsets, npat));
  BCE_TRY(edit_lengths(c, "locate_edit", offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &pat = c->qbuf[qb::edit_pat], &off = c->qbuf[qb::edit_off], &hits = c->qbuf[qb::edit_hits];
    BCE_TRY(ensure(c, hits, ((size_t)npat + 1) * 8));
    BCE_TRY(stage_patterns(c, pat, off, patterns, offsets, npat));
    return locate_edit_run(c, sa, pat.as<uint8_t>(), off.as<uint64_t>(), npat, k, flags & BCE_HIP_LOCATE_LINEAR, hits.as<uint64_t>(), hit_offsets,
                           nullptr, nullptr, nullptr, positions, lens, dists, !positions, cap, total);
  });
}

int bce_hip_locate_edit_device(bce_hip_ctx *c, const void *d_patterns, const void *d_offsets, uint32_t npat, uint32_t k, uint32_t flags,
                               void *d_hit_offsets, void *d_positions, void *d_lens, void *d_dists, uint64_t cap, uint64_t *total) {
  if (!c || !total || !edit_args(npat, k, flags)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) {
    if (!d_hit_offsets) return BCE_HIP_OK;
    return query_call(c, 0, [&]() -> int { BCE_HIP_TRY(c, hipMemsetAsync(d_hit_offsets, 0, 8, c->stream)); return BCE_HIP_OK; });
  }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate_edit"));
  if (!d_patterns || !d_offsets || !d_hit_offsets || (!d_positions && cap) || !d_positions != !d_dists || !d_positions != !d_lens) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return locate_edit_run(c, sa, static_cast<const uint8_t *>(d_patterns), static_cast<const uint64_t *>(d_offsets), npat, k,
                           flags & BCE_HIP_LOCATE_LINEAR, static_cast<uint64_t *>(d_hit_offsets), nullptr, static_cast<uint32_t *>(d_positions),
                           static_cast<uint16_t *>(d_lens), static_cast<uint8_t *>(d_dists), nullptr, nullptr, nullptr, !d_positions, cap, total);
  });
}

// ---- counts and positions of patterns of byte classes, under a budget (kd_classes.hip) --------------------------------------------
// The count's and the locate's rules, checks and protocol; max_nodes is judged beside ctx and the flags.  The patterns' lengths and
// their wide classes are judged by the prepare pass on the device, for host buffers too.
static bool class_budget(uint32_t &max_nodes) {
  if (max_nodes == 0) max_nodes = BCE_HIP_CLASS_DEFAULT_NODES;
  return max_nodes <= BCE_HIP_CLASS_MAX_NODES;
}
static int stage_classes(bce_hip_ctx *c, const uint32_t *masks, const uint64_t *offsets, uint32_t npat) {
  BCE_TRY(stage(c, c->qbuf[qb::cls_mask], masks, (size_t)offsets[npat] * 32));
  BCE_TRY(stage(c, c->qbuf[qb::cls_off], offsets, ((size_t)npat + 1) * 8));
  return ensure(c, c->qbuf[qb::cls_status], (size_t)npat * 4);
}

int bce_hip_count_classes(bce_hip_ctx *c, const uint32_t *masks, const uint64_t *offsets, uint32_t npat, uint32_t max_nodes, uint64_t *counts,
                          uint64_t *work, uint32_t *status) {
  if (!c || !class_budget(max_nodes)) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(planes_state(c, "count_classes"));
  if (!counts || !status) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "count_classes", reinterpret_cast<const uint8_t *>(masks), offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &out = c->qbuf[qb::cls_out], &wrk = c->qbuf[qb::cls_work], &st = c->qbuf[qb::cls_status];
    BCE_TRY(ensure(c, out, (size_t)npat * 8));
    BCE_TRY(ensure(c, wrk, (size_t)npat * 8));
    BCE_TRY(stage_classes(c, masks, offsets, npat));
    BCE_TRY(kd_class_count(c, c->qbuf[qb::cls_mask].as<uint32_t>(), c->qbuf[qb::cls_off].as<uint64_t>(), npat, max_nodes, out.as<uint64_t>(),
                           wrk.as<uint64_t>(), st.as<uint32_t>()));
    BCE_TRY(copy_out(c, counts, out, (size_t)npat * 8));
    if (work) BCE_TRY(copy_out(c, work, wrk, (size_t)npat * 8));
    return copy_out(c, status, st, (size_t)npat * 4);
  });
}

int bce_hip_count_classes_device(bce_hip_ctx *c, const void *d_masks, const void *d_offsets, uint32_t npat, uint32_t max_nodes, void *d_counts,
                                 void *d_work, void *d_status) {
  if (!c || !class_budget(max_nodes)) return BCE_HIP_E_ARG;
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(planes_state(c, "count_classes"));
  if (!d_masks || !d_offsets || !d_counts || !d_status) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return kd_class_count(c, static_cast<const uint32_t *>(d_masks), static_cast<const uint64_t *>(d_offsets), npat, max_nodes,
                          static_cast<uint64_t *>(d_counts), static_cast<uint64_t *>(d_work), static_cast<uint32_t *>(d_status));
  });
}

// locate_run with the verdicts beside the hit offsets
static int locate_classes_run(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes,
                              bool linear, uint64_t *d_hits, uint64_t *h_hits, uint32_t *d_status, uint32_t *h_status, uint32_t *d_pos, uint32_t *h_pos,
                              bool sizing, uint64_t cap, uint64_t *total) {
  uint64_t rows = 0, hits = 0;
  const int rc = kd_class_size(c, sa, d_masks, d_off, npat, max_nodes, linear, d_hits, d_status, &rows, &hits);
  if (rc != BCE_HIP_OK && rc != BCE_HIP_E_OVERFLOW) return rc;
  if (h_hits) {
    BCE_HIP_TRY(c, hipMemcpyAsync(h_hits, d_hits, ((size_t)npat + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    BCE_HIP_TRY(c, hipMemcpyAsync(h_status, d_status, (size_t)npat * 4, hipMemcpyDeviceToHost, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *total = hits;
  if (rc != BCE_HIP_OK || sizing) return rc;
  if (hits > cap) { snprintf(c->err, sizeof c->err, "locate_classes: %llu hits, room for %llu", (unsigned long long)hits, (unsigned long long)cap); return BCE_HIP_E_OVERFLOW; }
  if (hits == 0) return BCE_HIP_OK;
  if (h_pos) {
    BCE_TRY(ensure(c, c->qbuf[qb::cls_pos], (size_t)hits * 4));
    d_pos = c->qbuf[qb::cls_pos].as<uint32_t>();
  }
  BCE_TRY(kd_class_fill(c, sa, d_masks, d_off, npat, max_nodes, linear, rows, hits, d_status, d_pos));
  return h_pos ? copy_out(c, h_pos, c->qbuf[qb::cls_pos], (size_t)hits * 4) : BCE_HIP_OK;
}

int bce_hip_locate_classes(bce_hip_ctx *c, const uint32_t *masks, const uint64_t *offsets, uint32_t npat, uint32_t max_nodes, uint32_t flags,
                           uint64_t *hit_offsets, uint32_t *status, uint32_t *positions, uint64_t cap, uint64_t *total) {
  if (!c || !total || (flags & ~BCE_HIP_LOCATE_LINEAR) || !class_budget(max_nodes)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) { if (hit_offsets) hit_offsets[0] = 0; return BCE_HIP_OK; }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate_classes"));
  if (!hit_offsets || !status || (!positions && cap)) return BCE_HIP_E_ARG;
  BCE_TRY(pattern_list_args(c, "locate_classes", reinterpret_cast<const uint8_t *>(masks), offsets, npat));
  return query_call(c, 3, [&]() -> int {
    DevBuf &hits = c->qbuf[qb::cls_hits];
    BCE_TRY(ensure(c, hits, ((size_t)npat + 1) * 8));
    BCE_TRY(stage_classes(c, masks, offsets, npat));
    return locate_classes_run(c, sa, c->qbuf[qb::cls_mask].as<uint32_t>(), c->qbuf[qb::cls_off].as<uint64_t>(), npat, max_nodes,
                              flags & BCE_HIP_LOCATE_LINEAR, hits.as<uint64_t>(), hit_offsets, c->qbuf[qb::cls_status].as<uint32_t>(), status, nullptr,
                              positions, !positions, cap, total);
  });
}

int bce_hip_locate_classes_device(bce_hip_ctx *c, const void *d_masks, const void *d_offsets, uint32_t npat, uint32_t max_nodes, uint32_t flags,
                                  void *d_hit_offsets, void *d_status, void *d_positions, uint64_t cap, uint64_t *total) {
  if (!c || !total || (flags & ~BCE_HIP_LOCATE_LINEAR) || !class_budget(max_nodes)) return BCE_HIP_E_ARG;
  *total = 0;
  if (npat == 0) {
    if (!d_hit_offsets) return BCE_HIP_OK;
    return query_call(c, 0, [&]() -> int { BCE_HIP_TRY(c, hipMemsetAsync(d_hit_offsets, 0, 8, c->stream)); return BCE_HIP_OK; });
  }
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "locate_classes"));
  if (!d_masks || !d_offsets || !d_hit_offsets || !d_status || (!d_positions && cap)) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return locate_classes_run(c, sa, static_cast<const uint32_t *>(d_masks), static_cast<const uint64_t *>(d_offsets), npat, max_nodes,
                              flags & BCE_HIP_LOCATE_LINEAR, static_cast<uint64_t *>(d_hit_offsets), nullptr, static_cast<uint32_t *>(d_status), nullptr,
                              static_cast<uint32_t *>(d_positions), nullptr, !d_positions, cap, total);
  });
}

// ---- the longest matches of a second buffer in the text (kd_match.hip) -----------------------------------------------------------
// Cyclic lengths alone need the planes only, so they work behind an injected BWT; positions, and everything in linear mode, read
// sa[sa_res] by sa_state's rule -- read: nothing here writes that array, the planes or any stage's scratch.
static int match_args(bce_hip_ctx *c, uint64_t q, uint32_t max_len, uint32_t flags) {
  if (!c || (flags & ~BCE_HIP_MATCH_LINEAR)) return BCE_HIP_E_ARG;
  BCE_TRY(length_bound(c, "match", max_len));
  if (q > 0x7FFFFFFFull) { snprintf(c->err, sizeof c->err, "match: a query of 2^31 bytes or more"); return BCE_HIP_E_ARG; }
  return BCE_HIP_OK;
}
static int match_state(bce_hip_ctx *c, bool need_sa, const uint32_t **sa) {
  *sa = nullptr;
  return need_sa ? sa_state(c, sa, "match") : planes_state(c, "match");
}

int bce_hip_match(bce_hip_ctx *c, const uint8_t *query, uint64_t q, uint32_t max_len, uint32_t flags, uint32_t *len_out, uint32_t *pos_out) {
  BCE_TRY(match_args(c, q, max_len, flags));
  if (q == 0) return BCE_HIP_OK;
  const uint32_t *sa = nullptr;
  BCE_TRY(match_state(c, (flags & BCE_HIP_MATCH_LINEAR) || pos_out, &sa));
  if (!query || !len_out) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    DevBuf &qry = c->qbuf[qb::mat_qry], &len = c->qbuf[qb::mat_len], &pos = c->qbuf[qb::mat_pos];
    const size_t words = (size_t)q * 4;
    BCE_TRY(ensure(c, len, words));
    if (pos_out) BCE_TRY(ensure(c, pos, words));
    BCE_TRY(stage(c, qry, query, (size_t)q));
    BCE_TRY(kd_match(c, sa, qry.as<uint8_t>(), (uint32_t)q, max_len, flags & BCE_HIP_MATCH_LINEAR, len.as<uint32_t>(),
                     pos_out ? pos.as<uint32_t>() : nullptr));
    BCE_TRY(copy_out(c, len_out, len, words));
    return pos_out ? copy_out(c, pos_out, pos, words) : BCE_HIP_OK;
  });
}

int bce_hip_match_device(bce_hip_ctx *c, const void *d_query, uint64_t q, uint32_t max_len, uint32_t flags, void *d_len, void *d_pos) {
  BCE_TRY(match_args(c, q, max_len, flags));
  if (q == 0) return BCE_HIP_OK;
  const uint32_t *sa = nullptr;
  BCE_TRY(match_state(c, (flags & BCE_HIP_MATCH_LINEAR) || d_pos, &sa));
  if (!d_query || !d_len) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return kd_match(c, sa, static_cast<const uint8_t *>(d_query), (uint32_t)q, max_len, flags & BCE_HIP_MATCH_LINEAR, static_cast<uint32_t *>(d_len),
                    static_cast<uint32_t *>(d_pos));
  });
}

// The search with max_len = min_len (the windows of min_len bytes that end inside a longer match cover it: DESIGN.md 4.10), then
// the reduction; of the answer only the result word reaches the host.
static int coverage_run(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_query, uint32_t q, uint32_t min_len, bool linear, uint64_t *covered) {
  DevBuf &len = c->qbuf[qb::mat_len];
  BCE_TRY(ensure(c, len, (size_t)q * 4));
  BCE_TRY(kd_match(c, sa, d_query, q, min_len, linear, len.as<uint32_t>(), nullptr));
  return kd_coverage(c, len.as<uint32_t>(), q, min_len, covered);
}
// what both coverage entry points judge: *covered = 0 and *sa once the arguments and the state have passed
static int coverage_args(bce_hip_ctx *c, uint64_t q, uint32_t min_len, uint32_t flags, uint64_t *covered, const uint32_t **sa) {
  if (!covered) return BCE_HIP_E_ARG;
  BCE_TRY(match_args(c, q, min_len, flags));
  *covered = 0;
  return q ? match_state(c, flags & BCE_HIP_MATCH_LINEAR, sa) : BCE_HIP_OK;
}

int bce_hip_coverage(bce_hip_ctx *c, const uint8_t *query, uint64_t q, uint32_t min_len, uint32_t flags, uint64_t *covered) {
  const uint32_t *sa = nullptr;
  BCE_TRY(coverage_args(c, q, min_len, flags, covered, &sa));
  if (q == 0) return BCE_HIP_OK;
  if (!query) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    BCE_TRY(stage(c, c->qbuf[qb::mat_qry], query, (size_t)q));
    return coverage_run(c, sa, c->qbuf[qb::mat_qry].as<uint8_t>(), (uint32_t)q, min_len, flags & BCE_HIP_MATCH_LINEAR, covered);
  });
}

int bce_hip_coverage_device(bce_hip_ctx *c, const void *d_query, uint64_t q, uint32_t min_len, uint32_t flags, uint64_t *covered) {
  const uint32_t *sa = nullptr;
  BCE_TRY(coverage_args(c, q, min_len, flags, covered, &sa));
  if (q == 0) return BCE_HIP_OK;
  if (!d_query) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] { return coverage_run(c, sa, static_cast<const uint8_t *>(d_query), (uint32_t)q, min_len, flags & BCE_HIP_MATCH_LINEAR, covered); });
}

// ---- what the text holds by itself: the LCP array of the sorted rotations and its reductions (kd_lcp.hip) ---------------------------
// The locate's rule PLUS the text (text_state): both sa[sa_res] and `text` are read, neither is written.  Nothing is kept from one
// call to the next: every call runs its own LCP pass, so there is nothing that a load, bce_hip_set_bwt or a decode could leave stale.
static int lcp_args(bce_hip_ctx *c, const char *what, uint32_t max_len, const uint32_t **sa) {
  if (!c) return BCE_HIP_E_ARG;
  BCE_TRY(length_bound(c, what, max_len));
  return text_state(c, sa, what);
}
// the array of the context's own, for the calls that do not bring device memory for it
static int lcp_own(bce_hip_ctx *c, const uint32_t *sa, uint32_t max_len) {
  DevBuf &lcp = c->qbuf[qb::rep_lcp];
  BCE_TRY(ensure(c, lcp, (size_t)c->n * 4));
  return kd_lcp(c, sa, max_len, lcp.as<uint32_t>());
}

int bce_hip_lcp(bce_hip_ctx *c, uint32_t max_len, uint32_t *lcp_out) {
  const uint32_t *sa = nullptr;
  BCE_TRY(lcp_args(c, "lcp", max_len, &sa));
  if (!lcp_out) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    BCE_TRY(lcp_own(c, sa, max_len));
    return copy_out(c, lcp_out, c->qbuf[qb::rep_lcp], (size_t)c->n * 4);
  });
}

int bce_hip_lcp_device(bce_hip_ctx *c, uint32_t max_len, void *d_lcp) {
  const uint32_t *sa = nullptr;
  BCE_TRY(lcp_args(c, "lcp", max_len, &sa));
  if (!d_lcp) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] { return kd_lcp(c, sa, max_len, static_cast<uint32_t *>(d_lcp)); });
}

int bce_hip_kgrams(bce_hip_ctx *c, const uint32_t *ks, uint32_t nk, bce_hip_kgram *out) {
  if (!c) return BCE_HIP_E_ARG;
  if (nk > BCE_HIP_KGRAMS_MAX) { snprintf(c->err, sizeof c->err, "kgrams: %u values of k, more than %u", nk, BCE_HIP_KGRAMS_MAX); return BCE_HIP_E_ARG; }
  if (nk == 0) return BCE_HIP_OK;
  if (!ks) return BCE_HIP_E_ARG;
  uint32_t bound = 1;                                                 // (k = 0 needs no array at all; the pass is bounded by 1 then)
  for (uint32_t i = 0; i < nk; ++i) {
    if (ks[i] > BCE_HIP_MATCH_MAX_LEN) { snprintf(c->err, sizeof c->err, "kgrams: k = %u, outside 0 .. %u", ks[i], BCE_HIP_MATCH_MAX_LEN); return BCE_HIP_E_ARG; }
    if (ks[i] > bound) bound = ks[i];
  }
  const uint32_t *sa = nullptr;
  BCE_TRY(text_state(c, &sa, "kgrams"));
  if (!out) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    BCE_TRY(lcp_own(c, sa, bound));
    return kd_kgrams(c, sa, c->qbuf[qb::rep_lcp].as<uint32_t>(), c->n, ks, nk, out);
  });
}

int bce_hip_longest_repeat(bce_hip_ctx *c, uint32_t max_len, uint32_t *len, uint32_t *pos_a, uint32_t *pos_b) {
  const uint32_t *sa = nullptr;
  BCE_TRY(lcp_args(c, "longest repeat", max_len, &sa));
  if (!len || !pos_a || !pos_b) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    uint32_t res[3];
    BCE_TRY(lcp_own(c, sa, max_len));
    BCE_TRY(kd_longest_repeat(c, sa, c->qbuf[qb::rep_lcp].as<uint32_t>(), c->n, res));
    *len = res[0]; *pos_a = res[1]; *pos_b = res[2];
    return BCE_HIP_OK;
  });
}

// ---- the most frequent k-grams of the text, as a list (kd_lcp.hip: kd_top_kgrams; top_step.h) --------------------------------------
// bce_hip_kgrams' rule and order of refusals.  found, distinct and size_hist are written once everything queued has completed.
static int top_args(bce_hip_ctx *c, uint32_t k, uint32_t limit, const void *bytes, uint64_t bytes_cap, const uint32_t *found, const uint32_t **sa) {
  if (!c) return BCE_HIP_E_ARG;
  if (k > BCE_HIP_MATCH_MAX_LEN) { snprintf(c->err, sizeof c->err, "top k-grams: k = %u, outside 0 .. %u", k, BCE_HIP_MATCH_MAX_LEN); return BCE_HIP_E_ARG; }
  if (limit < 1 || limit > BCE_HIP_TOP_MAX) { snprintf(c->err, sizeof c->err, "top k-grams: a limit of %u, outside 1 .. %u", limit, BCE_HIP_TOP_MAX); return BCE_HIP_E_ARG; }
  if (!found) { snprintf(c->err, sizeof c->err, "top k-grams: no place for the number of entries"); return BCE_HIP_E_ARG; }
  if (bytes && bytes_cap < (uint64_t)limit * k) {
    snprintf(c->err, sizeof c->err, "top k-grams: room for %llu bytes, %u entries of %u bytes need %llu", (unsigned long long)bytes_cap, limit, k,
             (unsigned long long)((uint64_t)limit * k));
    return BCE_HIP_E_ARG;
  }
  return text_state(c, sa, "top k-grams");
}

int bce_hip_top_kgrams(bce_hip_ctx *c, uint32_t k, uint32_t limit, bce_hip_top_kgram *out, uint8_t *bytes, uint64_t bytes_cap, uint32_t *found,
                       uint64_t *distinct, uint64_t size_hist[32]) {
  const uint32_t *sa = nullptr;
  BCE_TRY(top_args(c, k, limit, bytes, bytes_cap, found, &sa));
  if (!out) return BCE_HIP_E_ARG;
  uint32_t got = 0;
  uint64_t classes = 0, hist[32];
  BCE_TRY(query_call(c, 3, [&]() -> int {
    DevBuf &ent = c->qbuf[qb::top_out], &gram = c->qbuf[qb::top_bytes];
    const bool with_bytes = bytes && k;
    const uint32_t room = limit < c->n ? limit : c->n;                 // (there are at most n classes)
    BCE_TRY(lcp_own(c, sa, k ? k : 1u));
    BCE_TRY(ensure(c, ent, (size_t)room * sizeof(bce_hip_top_kgram)));
    if (with_bytes) BCE_TRY(ensure(c, gram, (size_t)room * k));
    BCE_TRY(kd_top_kgrams(c, sa, c->qbuf[qb::rep_lcp].as<uint32_t>(), c->n, c->text.as<uint8_t>(), k, limit, ent.as<bce_hip_top_kgram>(),
                          with_bytes ? gram.as<uint8_t>() : nullptr, &got, &classes, hist));
    BCE_TRY(copy_out(c, out, ent, (size_t)got * sizeof(bce_hip_top_kgram)));
    return with_bytes ? copy_out(c, bytes, gram, (size_t)got * k) : BCE_HIP_OK;
  }));
  *found = got;
  if (distinct) *distinct = classes;
  if (size_hist) memcpy(size_hist, hist, sizeof hist);
  return BCE_HIP_OK;
}

int bce_hip_top_kgrams_device(bce_hip_ctx *c, uint32_t k, uint32_t limit, void *d_out, void *d_bytes, uint64_t bytes_cap, uint32_t *found,
                              uint64_t *distinct, uint64_t size_hist[32]) {
  const uint32_t *sa = nullptr;
  BCE_TRY(top_args(c, k, limit, d_bytes, bytes_cap, found, &sa));
  if (!d_out) return BCE_HIP_E_ARG;
  uint32_t got = 0;
  uint64_t classes = 0, hist[32];
  BCE_TRY(query_call(c, 3, [&]() -> int {
    BCE_TRY(lcp_own(c, sa, k ? k : 1u));
    return kd_top_kgrams(c, sa, c->qbuf[qb::rep_lcp].as<uint32_t>(), c->n, c->text.as<uint8_t>(), k, limit, static_cast<bce_hip_top_kgram *>(d_out),
                         static_cast<uint8_t *>(d_bytes), &got, &classes, hist);
  }));
  *found = got;
  if (distinct) *distinct = classes;
  if (size_hist) memcpy(size_hist, hist, sizeof hist);
  return BCE_HIP_OK;
}

// ---- the maximal repeats of the text, as a list (kd_maxrep.hip; maxrep_step.h) -------------------------------------------------------
// bce_hip_top_kgrams' rule and order of refusals.  *info is written once everything queued has completed.
static int maxrep_list_args(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, const void *info) {
  BCE_TRY(length_bound(c, "maximal repeats", max_len));
  if (min_len < 1 || min_len > max_len) { snprintf(c->err, sizeof c->err, "maximal repeats: a least length of %u, outside 1 .. %u", min_len, max_len); return BCE_HIP_E_ARG; }
  if (order > BCE_HIP_MAXREP_BY_GAIN) { snprintf(c->err, sizeof c->err, "maximal repeats: order %u is none of len (0), count (1), gain (2)", order); return BCE_HIP_E_ARG; }
  if (limit < 1 || limit > BCE_HIP_TOP_MAX) { snprintf(c->err, sizeof c->err, "maximal repeats: a limit of %u, outside 1 .. %u", limit, BCE_HIP_TOP_MAX); return BCE_HIP_E_ARG; }
  if (!info) { snprintf(c->err, sizeof c->err, "maximal repeats: no place for the counts"); return BCE_HIP_E_ARG; }
  return BCE_HIP_OK;
}
static int maxrep_args(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, const void *bytes, uint32_t bytes_per,
                       uint64_t bytes_cap, const void *info, const uint32_t **sa) {
  if (!c) return BCE_HIP_E_ARG;
  BCE_TRY(maxrep_list_args(c, min_len, max_len, order, limit, info));
  if (bytes_per > BCE_HIP_MATCH_MAX_LEN) { snprintf(c->err, sizeof c->err, "maximal repeats: %u bytes per entry, more than %u", bytes_per, BCE_HIP_MATCH_MAX_LEN); return BCE_HIP_E_ARG; }
  if (bytes && bytes_cap < (uint64_t)limit * bytes_per) {
    snprintf(c->err, sizeof c->err, "maximal repeats: room for %llu bytes, %u entries of %u bytes need %llu", (unsigned long long)bytes_cap, limit, bytes_per,
             (unsigned long long)((uint64_t)limit * bytes_per));
    return BCE_HIP_E_ARG;
  }
  return text_state(c, sa, "maximal repeats");
}

int bce_hip_maximal_repeats(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, bce_hip_maxrep *out, uint8_t *bytes,
                            uint32_t bytes_per, uint64_t bytes_cap, bce_hip_maxrep_info *info) {
  const uint32_t *sa = nullptr;
  BCE_TRY(maxrep_args(c, min_len, max_len, order, limit, bytes, bytes_per, bytes_cap, info, &sa));
  if (!out) return BCE_HIP_E_ARG;
  bce_hip_maxrep_info got;
  BCE_TRY(query_call(c, 3, [&]() -> int {
    DevBuf &ent = c->qbuf[qb::mxr_out], &str = c->qbuf[qb::mxr_bytes];
    const bool with_bytes = bytes && bytes_per;
    const uint32_t room = limit < c->n ? limit : c->n;                 // (there are fewer intervals than rows)
    BCE_TRY(lcp_own(c, sa, max_len));
    BCE_TRY(ensure(c, ent, (size_t)room * sizeof(bce_hip_maxrep)));
    if (with_bytes) BCE_TRY(ensure(c, str, (size_t)room * bytes_per));
    BCE_TRY(kd_maxrep(c, sa, c->qbuf[qb::rep_lcp].as<uint32_t>(), c->n, c->text.as<uint8_t>(), nullptr, min_len, max_len, order, limit,
                      ent.as<bce_hip_maxrep>(), with_bytes ? str.as<uint8_t>() : nullptr, bytes_per, &got));
    BCE_TRY(copy_out(c, out, ent, (size_t)got.found * sizeof(bce_hip_maxrep)));
    return with_bytes ? copy_out(c, bytes, str, (size_t)got.found * bytes_per) : BCE_HIP_OK;
  }));
  *info = got;
  return BCE_HIP_OK;
}

int bce_hip_maximal_repeats_device(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, uint32_t order, uint32_t limit, void *d_out, void *d_bytes,
                                   uint32_t bytes_per, uint64_t bytes_cap, bce_hip_maxrep_info *info) {
  const uint32_t *sa = nullptr;
  BCE_TRY(maxrep_args(c, min_len, max_len, order, limit, d_bytes, bytes_per, bytes_cap, info, &sa));
  if (!d_out) return BCE_HIP_E_ARG;
  bce_hip_maxrep_info got;
  BCE_TRY(query_call(c, 3, [&]() -> int {
    BCE_TRY(lcp_own(c, sa, max_len));
    return kd_maxrep(c, sa, c->qbuf[qb::rep_lcp].as<uint32_t>(), c->n, c->text.as<uint8_t>(), nullptr, min_len, max_len, order, limit,
                     static_cast<bce_hip_maxrep *>(d_out), static_cast<uint8_t *>(d_bytes), bytes_per, &got);
  }));
  *info = got;
  return BCE_HIP_OK;
}

// test hook: the same launches on arrays of the caller's, phase 0 as the other hooks; the entries are staged in mxr_out
int bce_hip_maxrep_of_arrays_device(bce_hip_ctx *c, const void *d_lcp, uint32_t n, const void *d_sa, const void *d_bw, uint32_t min_len, uint32_t max_len,
                                    uint32_t order, uint32_t limit, bce_hip_maxrep *out, bce_hip_maxrep_info *info) {
  if (!c || !d_lcp || !d_sa || !d_bw || !out || n == 0 || n > 0x7FFFFFFFu) return BCE_HIP_E_ARG;
  BCE_TRY(maxrep_list_args(c, min_len, max_len, order, limit, info));
  bce_hip_maxrep_info got;
  BCE_TRY(query_call(c, 0, [&]() -> int {
    DevBuf &lcp = c->qbuf[qb::rep_lcp], &ent = c->qbuf[qb::mxr_out];
    const size_t words = (size_t)n * 4;
    BCE_TRY(ensure(c, lcp, words));
    BCE_TRY(ensure(c, ent, (size_t)(limit < n ? limit : n) * sizeof(bce_hip_maxrep)));
    BCE_HIP_TRY(c, hipMemcpyAsync(lcp.p, d_lcp, words, hipMemcpyDeviceToDevice, c->stream));
    BCE_TRY(kd_maxrep(c, static_cast<const uint32_t *>(d_sa), lcp.as<uint32_t>(), n, nullptr, static_cast<const uint8_t *>(d_bw), min_len, max_len, order,
                      limit, ent.as<bce_hip_maxrep>(), nullptr, 0, &got));
    return copy_out(c, out, ent, (size_t)got.found * sizeof(bce_hip_maxrep));
  }));
  *info = got;
  return BCE_HIP_OK;
}

// ---- a second buffer as a delta against the text: parse and patch (kd_parse.hip) ----------------------------------------------------
// The parse: the match's rule with positions (sa_state).  The query of a call with a host buffer and the statistics are staged in
// the match's mat_qry / mat_len / mat_pos; every other temporary is a par_* buffer of the feature's own.  The patch reads the text
// alone.
static int parse_args(bce_hip_ctx *c, uint64_t q, uint32_t min_len, uint32_t max_len, const void *ops, uint64_t ops_cap, const void *lits,
                      uint64_t lits_cap, bce_hip_parse_info *info) {
  if (!c || !info) return BCE_HIP_E_ARG;
  if (min_len < 1 || min_len > max_len || max_len > BCE_HIP_MATCH_MAX_LEN) {
    snprintf(c->err, sizeof c->err, "parse: bounds %u .. %u, outside 1 <= min_len <= max_len <= %u", min_len, max_len, BCE_HIP_MATCH_MAX_LEN);
    return BCE_HIP_E_ARG;
  }
  if (q > 0x7FFFFFFFull) { snprintf(c->err, sizeof c->err, "parse: a query of 2^31 bytes or more"); return BCE_HIP_E_ARG; }
  if ((!ops && ops_cap) || (!lits && lits_cap)) return BCE_HIP_E_ARG;
  if (q == 0) *info = bce_hip_parse_info{0, 0, 0, 0};
  return BCE_HIP_OK;
}
// the linear statistics of a query in device memory, with positions, into mat_len / mat_pos; then the parse from them
static int parse_run(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_query, uint32_t q, uint32_t min_len, uint32_t max_len, uint32_t *d_ops,
                     uint64_t ops_cap, uint8_t *d_lits, uint64_t lits_cap, bce_hip_parse_info *info) {
  DevBuf &len = c->qbuf[qb::mat_len], &pos = c->qbuf[qb::mat_pos];
  BCE_TRY(ensure(c, len, (size_t)q * 4));
  BCE_TRY(ensure(c, pos, (size_t)q * 4));
  BCE_TRY(kd_match(c, sa, d_query, q, max_len, true, len.as<uint32_t>(), pos.as<uint32_t>()));
  return kd_parse(c, len.as<uint32_t>(), pos.as<uint32_t>(), d_query, q, min_len, !d_ops && !d_lits, d_ops, ops_cap, d_lits, lits_cap, info);
}

int bce_hip_parse(bce_hip_ctx *c, const uint8_t *query, uint64_t q, uint32_t min_len, uint32_t max_len, bce_hip_op *ops, uint64_t ops_cap,
                  uint8_t *lits, uint64_t lits_cap, bce_hip_parse_info *info) {
  BCE_TRY(parse_args(c, q, min_len, max_len, ops, ops_cap, lits, lits_cap, info));
  if (q == 0) return BCE_HIP_OK;
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "parse"));
  if (!query) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    DevBuf &qry = c->qbuf[qb::mat_qry], &d_ops = c->qbuf[qb::par_ops], &d_lits = c->qbuf[qb::par_lits];
    BCE_TRY(stage(c, qry, query, (size_t)q));
    // Unlike the device entry, sized first: the staging of the two outputs is as large as they are, and an overflow touches neither
    BCE_TRY(parse_run(c, sa, qry.as<uint8_t>(), (uint32_t)q, min_len, max_len, nullptr, 0, nullptr, 0, info));
    if (!ops && !lits) return BCE_HIP_OK;
    BCE_TRY(ensure(c, d_ops, (size_t)info->nops * 8));
    BCE_TRY(ensure(c, d_lits, info->nlits ? (size_t)info->nlits : 1));
    BCE_TRY(kd_parse(c, c->qbuf[qb::mat_len].as<uint32_t>(), c->qbuf[qb::mat_pos].as<uint32_t>(), qry.as<uint8_t>(), (uint32_t)q, min_len, false,
                     d_ops.as<uint32_t>(), ops_cap, d_lits.as<uint8_t>(), lits_cap, info));
    BCE_TRY(copy_out(c, ops, d_ops, (size_t)info->nops * 8));
    return copy_out(c, lits, d_lits, (size_t)info->nlits);
  });
}

int bce_hip_parse_device(bce_hip_ctx *c, const void *d_query, uint64_t q, uint32_t min_len, uint32_t max_len, void *d_ops, uint64_t ops_cap,
                         void *d_lits, uint64_t lits_cap, bce_hip_parse_info *info) {
  BCE_TRY(parse_args(c, q, min_len, max_len, d_ops, ops_cap, d_lits, lits_cap, info));
  if (q == 0) return BCE_HIP_OK;
  const uint32_t *sa = nullptr;
  BCE_TRY(sa_state(c, &sa, "parse"));
  if (!d_query) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] {
    return parse_run(c, sa, static_cast<const uint8_t *>(d_query), (uint32_t)q, min_len, max_len, static_cast<uint32_t *>(d_ops), ops_cap,
                     static_cast<uint8_t *>(d_lits), lits_cap, info);
  });
}

int bce_hip_parse_of_lengths_device(bce_hip_ctx *c, const void *d_len, const void *d_pos, const void *d_query, uint64_t q, uint32_t min_len,
                                    void *d_ops, uint64_t ops_cap, void *d_lits, uint64_t lits_cap, bce_hip_parse_info *info) {
  BCE_TRY(parse_args(c, q, min_len, BCE_HIP_MATCH_MAX_LEN, d_ops, ops_cap, d_lits, lits_cap, info));
  if (q == 0) return BCE_HIP_OK;
  if (!d_len || !d_query) return BCE_HIP_E_ARG;
  return query_call(c, 0, [&] {
    return kd_parse(c, static_cast<const uint32_t *>(d_len), static_cast<const uint32_t *>(d_pos), static_cast<const uint8_t *>(d_query), (uint32_t)q,
                    min_len, !d_ops && !d_lits, static_cast<uint32_t *>(d_ops), ops_cap, static_cast<uint8_t *>(d_lits), lits_cap, info);
  });
}

// Arguments, then the state (a loaded text), then the list without ops: nothing to launch -- the empty result, and no literal byte
// may be left over.  *empty: the call is answered.
static int patch_args(bce_hip_ctx *c, const void *ops, uint64_t nops, const void *lits, uint64_t nlits, const void *out, uint64_t cap,
                      uint64_t *out_len, bool *empty) {
  if (!c || !out_len) return BCE_HIP_E_ARG;
  if (nops > 0x7FFFFFFFull) { snprintf(c->err, sizeof c->err, "patch: 2^31 ops or more, a result of 2^31 bytes or more"); return BCE_HIP_E_ARG; }
  if ((nops && !ops) || (nlits && !lits) || (cap && !out)) return BCE_HIP_E_ARG;
  if (!(c->text_loaded && c->stage >= 1 && c->text.p && c->text.cap >= (size_t)c->n)) {
    snprintf(c->err, sizeof c->err, "patch: no loaded input in this context");
    return BCE_HIP_E_STATE;
  }
  *empty = nops == 0;
  if (!*empty) return BCE_HIP_OK;
  if (const char *why = bce::patch_list_bad(0, 0, 0, nlits)) { snprintf(c->err, sizeof c->err, "%s", why); return BCE_HIP_E_ARG; }
  *out_len = 0;
  return BCE_HIP_OK;
}

int bce_hip_patch(bce_hip_ctx *c, const bce_hip_op *ops, uint64_t nops, const uint8_t *lits, uint64_t nlits, uint8_t *out, uint64_t cap,
                  uint64_t *out_len) {
  bool empty = false;
  BCE_TRY(patch_args(c, ops, nops, lits, nlits, out, cap, out_len, &empty));
  if (empty) return BCE_HIP_OK;
  return query_call(c, 3, [&]() -> int {
    DevBuf &d_ops = c->qbuf[qb::par_ops], &d_lits = c->qbuf[qb::par_lits], &d_out = c->qbuf[qb::par_out];
    BCE_TRY(stage(c, d_ops, ops, (size_t)nops * 8));
    BCE_TRY(stage(c, d_lits, lits, (size_t)nlits));
    // Unlike the device entry, validated and sized first: the staging of the result is as large as the result
    uint64_t total = 0;
    BCE_TRY(kd_patch(c, d_ops.as<uint32_t>(), (uint32_t)nops, d_lits.as<uint8_t>(), nlits, true, nullptr, 0, &total));
    *out_len = total;
    if (!out) return BCE_HIP_OK;
    if (total > cap) { snprintf(c->err, sizeof c->err, "patch: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap); return BCE_HIP_E_OVERFLOW; }
    BCE_TRY(ensure(c, d_out, (size_t)total));
    BCE_TRY(kd_patch(c, d_ops.as<uint32_t>(), (uint32_t)nops, d_lits.as<uint8_t>(), nlits, false, d_out.as<uint8_t>(), total, &total));
    return copy_out(c, out, d_out, (size_t)total);
  });
}

int bce_hip_patch_device(bce_hip_ctx *c, const void *d_ops, uint64_t nops, const void *d_lits, uint64_t nlits, void *d_out, uint64_t cap,
                         uint64_t *out_len) {
  bool empty = false;
  BCE_TRY(patch_args(c, d_ops, nops, d_lits, nlits, d_out, cap, out_len, &empty));
  if (empty) return BCE_HIP_OK;
  return query_call(c, 3, [&] {
    return kd_patch(c, static_cast<const uint32_t *>(d_ops), (uint32_t)nops, static_cast<const uint8_t *>(d_lits), nlits, !d_out,
                    static_cast<uint8_t *>(d_out), cap, out_len);
  });
}

// ---- what the text repeats of itself: longest previous factors and the self-parse (kd_self.hip) -----------------------------------
// The LCP array's rule (text_state): sa[sa_res] and `text` are read, neither is written; every temporary is a slf_* buffer of the
// feature's own, or kd_parse's par_*.  Nothing is kept from one call to the next.
int bce_hip_lpf(bce_hip_ctx *c, uint32_t max_len, uint32_t *lpf_out, uint32_t *src_out) {
  const uint32_t *sa = nullptr;
  BCE_TRY(lcp_args(c, "lpf", max_len, &sa));
  if (!lpf_out) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&]() -> int {
    DevBuf &lpf = c->qbuf[qb::slf_lpf], &src = c->qbuf[qb::slf_src];
    const size_t words = (size_t)c->n * 4;
    BCE_TRY(ensure(c, lpf, words));
    if (src_out) BCE_TRY(ensure(c, src, words));
    BCE_TRY(kd_lpf(c, sa, max_len, false, lpf.as<uint32_t>(), src_out ? src.as<uint32_t>() : nullptr));
    BCE_TRY(copy_out(c, lpf_out, lpf, words));
    return src_out ? copy_out(c, src_out, src, words) : BCE_HIP_OK;
  });
}

int bce_hip_lpf_device(bce_hip_ctx *c, uint32_t max_len, void *d_lpf, void *d_src) {
  const uint32_t *sa = nullptr;
  BCE_TRY(lcp_args(c, "lpf", max_len, &sa));
  if (!d_lpf) return BCE_HIP_E_ARG;
  return query_call(c, 3, [&] { return kd_lpf(c, sa, max_len, false, static_cast<uint32_t *>(d_lpf), static_cast<uint32_t *>(d_src)); });
}

static int self_args(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, const void *ops, uint64_t ops_cap, const void *lits, uint64_t lits_cap,
                     bce_hip_parse_info *info, const uint32_t **sa) {
  if (!c || !info) return BCE_HIP_E_ARG;
  if (min_len < 1 || min_len > max_len || max_len > BCE_HIP_MATCH_MAX_LEN) {
    snprintf(c->err, sizeof c->err, "self-parse: bounds %u .. %u, outside 1 <= min_len <= max_len <= %u", min_len, max_len, BCE_HIP_MATCH_MAX_LEN);
    return BCE_HIP_E_ARG;
  }
  if ((!ops && ops_cap) || (!lits && lits_cap)) return BCE_HIP_E_ARG;
  return text_state(c, sa, "self-parse");
}
// lpf, src and the text at their mirrors (slf_rlen / slf_rsrc / slf_rtext), ready for the chain
static int self_mirrors(bce_hip_ctx *c, const uint32_t *sa, uint32_t max_len) {
  BCE_TRY(kd_self_mirror(c, nullptr, nullptr, c->text.as<uint8_t>(), c->n));
  BCE_TRY(ensure(c, c->qbuf[qb::slf_rsrc], (size_t)c->n * 4));
  return kd_lpf(c, sa, max_len, true, c->qbuf[qb::slf_rlen].as<uint32_t>(), c->qbuf[qb::slf_rsrc].as<uint32_t>());
}

int bce_hip_self_parse(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, bce_hip_op *ops, uint64_t ops_cap, uint8_t *lits, uint64_t lits_cap,
                       bce_hip_parse_info *info) {
  const uint32_t *sa = nullptr;
  BCE_TRY(self_args(c, min_len, max_len, ops, ops_cap, lits, lits_cap, info, &sa));
  return query_call(c, 3, [&]() -> int {
    DevBuf &d_ops = c->qbuf[qb::slf_ops], &d_lits = c->qbuf[qb::slf_lits];
    BCE_TRY(self_mirrors(c, sa, max_len));
    // as bce_hip_parse: sized first, the staging of the two outputs is as large as they are, and an overflow touches neither
    BCE_TRY(kd_self_parse(c, c->n, min_len, true, true, nullptr, 0, nullptr, 0, info));
    if (!ops && !lits) return BCE_HIP_OK;
    BCE_TRY(ensure(c, d_ops, (size_t)info->nops * 8));
    BCE_TRY(ensure(c, d_lits, info->nlits ? (size_t)info->nlits : 1));
    BCE_TRY(kd_self_parse(c, c->n, min_len, true, false, d_ops.as<uint32_t>(), ops_cap, d_lits.as<uint8_t>(), lits_cap, info));
    BCE_TRY(copy_out(c, ops, d_ops, (size_t)info->nops * 8));
    return copy_out(c, lits, d_lits, (size_t)info->nlits);
  });
}

int bce_hip_self_parse_device(bce_hip_ctx *c, uint32_t min_len, uint32_t max_len, void *d_ops, uint64_t ops_cap, void *d_lits, uint64_t lits_cap,
                              bce_hip_parse_info *info) {
  const uint32_t *sa = nullptr;
  BCE_TRY(self_args(c, min_len, max_len, d_ops, ops_cap, d_lits, lits_cap, info, &sa));
  return query_call(c, 3, [&]() -> int {
    BCE_TRY(self_mirrors(c, sa, max_len));
    return kd_self_parse(c, c->n, min_len, true, !d_ops && !d_lits, static_cast<uint32_t *>(d_ops), ops_cap, static_cast<uint8_t *>(d_lits), lits_cap, info);
  });
}

// ---- the suffix array as a product, and a checker for one (k1_bwt.hip: k1_suffix_array; kd_sufsort.hip) ---------------------------
// The sort is bce_hip_divbwt's: phase 1, the coder drained, the compression state dropped.  The checker is a hook's equal: phase 0,
// only its own sfc_* buffers written, valid in any state.
int bce_hip_suffix_array(bce_hip_ctx *c, const uint8_t *in, uint32_t n, uint32_t *sa_out, uint32_t *isa_out) {
  if (!c || !in || !sa_out || n == 0 || n >= 0x7FFFFFFFu) return BCE_HIP_E_ARG;
  return query_call(c, 1, [&]() -> int {
    c->coder->drain();
    DevBuf &sa = c->qbuf[qb::sfa_sa], &isa = c->qbuf[qb::sfa_isa];
    const size_t words = (size_t)n * 4;
    BCE_TRY(ensure(c, sa, words));
    if (isa_out) BCE_TRY(ensure(c, isa, words));
    BCE_TRY(k1_suffix_array(c, in, false, n, sa.as<uint32_t>(), isa_out ? isa.as<uint32_t>() : nullptr));
    BCE_TRY(copy_out(c, sa_out, sa, words));
    return isa_out ? copy_out(c, isa_out, isa, words) : BCE_HIP_OK;
  });
}

int bce_hip_suffix_array_device(bce_hip_ctx *c, const void *d_in, uint32_t n, void *d_sa, void *d_isa) {
  if (!c || !d_in || !d_sa || n == 0 || n >= 0x7FFFFFFFu) return BCE_HIP_E_ARG;
  return query_call(c, 1, [&]() -> int {
    c->coder->drain();
    return k1_suffix_array(c, static_cast<const uint8_t *>(d_in), true, n, static_cast<uint32_t *>(d_sa), static_cast<uint32_t *>(d_isa));
  });
}

int bce_hip_sufcheck(bce_hip_ctx *c, const uint8_t *in, const uint32_t *sa, uint32_t n, uint64_t *bad, uint32_t *reason) {
  if (!c || !in || !sa || !bad || !reason || n == 0 || n >= 0x80000000u) return BCE_HIP_E_ARG;
  uint64_t at = UINT64_MAX;
  uint32_t why = BCE_HIP_SUFCHECK_OK;
  BCE_TRY(query_call(c, 0, [&]() -> int {
    DevBuf &text = c->qbuf[qb::sfc_text], &arr = c->qbuf[qb::sfc_sa];
    BCE_TRY(stage(c, text, in, (size_t)n));
    BCE_TRY(stage(c, arr, sa, (size_t)n * 4));
    return kd_sufcheck(c, text.as<uint8_t>(), arr.as<uint32_t>(), n, &at, &why);
  }));
  *bad = at; *reason = why;
  return BCE_HIP_OK;
}

int bce_hip_sufcheck_device(bce_hip_ctx *c, const void *d_in, const void *d_sa, uint32_t n, uint64_t *bad, uint32_t *reason) {
  if (!c || !d_in || !d_sa || !bad || !reason || n == 0 || n >= 0x80000000u) return BCE_HIP_E_ARG;
  uint64_t at = UINT64_MAX;
  uint32_t why = BCE_HIP_SUFCHECK_OK;
  BCE_TRY(query_call(c, 0, [&] { return kd_sufcheck(c, static_cast<const uint8_t *>(d_in), static_cast<const uint32_t *>(d_sa), n, &at, &why); }));
  *bad = at; *reason = why;
  return BCE_HIP_OK;
}

// test hooks: phase 0, as the scans' hooks above
int bce_hip_nsv_device(bce_hip_ctx *c, const void *d_vals, uint32_t n, void *d_psv, void *d_nsv) {
  if (!c || !d_vals || !d_psv || !d_nsv || n == 0 || n > 0x7FFFFFFFu) return BCE_HIP_E_ARG;
  return query_call(c, 0, [&] { return kd_nsv(c, static_cast<const uint32_t *>(d_vals), n, static_cast<uint32_t *>(d_psv), static_cast<uint32_t *>(d_nsv)); });
}

int bce_hip_self_parse_of_lpf_device(bce_hip_ctx *c, const void *d_lpf, const void *d_src, const void *d_text, uint64_t n, uint32_t min_len,
                                     void *d_ops, uint64_t ops_cap, void *d_lits, uint64_t lits_cap, bce_hip_parse_info *info) {
  BCE_TRY(parse_args(c, n, min_len, BCE_HIP_MATCH_MAX_LEN, d_ops, ops_cap, d_lits, lits_cap, info));
  if (n == 0) return BCE_HIP_OK;
  if (!d_lpf || !d_text) return BCE_HIP_E_ARG;
  return query_call(c, 0, [&]() -> int {
    BCE_TRY(kd_self_mirror(c, static_cast<const uint32_t *>(d_lpf), static_cast<const uint32_t *>(d_src), static_cast<const uint8_t *>(d_text), (uint32_t)n));
    return kd_self_parse(c, (uint32_t)n, min_len, d_src != nullptr, !d_ops && !d_lits, static_cast<uint32_t *>(d_ops), ops_cap,
                         static_cast<uint8_t *>(d_lits), lits_cap, info);
  });
}

}  // extern "C"
