// kd_edit.hip -- how often, and where, byte strings occur in the text within k edits (substitutions, insertions and deletions;
// the anchored edit distance of include/bce_hip.h), from the K2 planes and K1's suffix array (bce_hip_count_edit / _locate_edit and
// their _device forms, `bce -gw` / `-gwl`).
//
// The search is edit_step.h's: backward search that branches three ways.  A WAVE walks one pattern's tree, as kd_near.hip's does:
//   - The frames (a node with budget left: interval, position, length offset, what brought it there) are wave-uniform.  At a
//     frame's position the 64 lanes share the 256 candidate bytes, four near_child steps each; the substitution child and the
//     insertion child of a byte are that one step.
//   - The edit that spends the budget (k = 1, or the second edit of k = 2; edit_last_branch, written once for both): each lane
//     finishes its own children, the substitution from pos - 1 and the insertion from pos, as two chains that run together
//     (edit_finish2: after the insertion's first step both read the same pattern bytes).  The deletion is one more chain from the
//     node's own interval at pos - 1: the lane whose candidate byte is the pattern's own has no substitution child, so its first
//     chain carries the deletion.  Each kind is handed to emit on its own: (distance, length) is wave-uniform in every emit.
//   - Budget left (k = 2, the first edit): the surviving children become the next frame one by one, read from their lane's
//     registers by the ballot's order, substitutions, then insertions, then the deletion.  Memory per wave does not depend on n, m
//     or the number of answers.
//   - k = 0 is near_finish from the root.
// What the walk finds are CANDIDATES (row interval, edits, length): different scripts reach one string and strings of different
// lengths nest, so a position comes up many times.  The answer is the least (edits, length) per position:
//   size     the walk; candidate rows per pattern, kd_locate.hip's scan (locate_scan) to candidate segments.
//   fill     the walk again; the wave writes (sa[row], pattern id << 4 | code) of every candidate row at a cursor of its own inside
//            the pattern's segment -- plain stores, no atomics.  code = edit_code(edits, length offset); in linear mode a candidate
//            that ends past the text's end gets BCE_EDIT_DEAD, which sorts after every live code.
//   order    three stable radix_sort_pairs: the code's four bits, the position bits, the pattern-id bits.  Pattern p's records
//            stand in its segment again, by position, and within a position the least (edits, length) first, dead ones last.
//   reduce   a record is a HEAD when it is live and the first of its position.  One wave per pattern counts its heads, in all and
//            per distance; locate_scan turns the counts into hit_offsets; one wave per pattern writes its heads out in order.
// Everything written is the locate's scratch (qb::loc_* of c->qbuf: calls of one context never run together), edit_res, edit_cnt
// or the caller's outputs.
#include "common.h"
#include "edit_step.h"
#include "scan_util.h"
#include "wave_walk.h"

namespace bce {

namespace {

constexpr int EDIT_T = 256;                  // lanes per workgroup (4 waves = 4 patterns)
constexpr uint32_t EDIT_WAVES = EDIT_T / 64;
constexpr uint64_t EDIT_MAXROWS = 0x7FFFFFFFull;
constexpr uint32_t EDIT_BAD_ORDER = 1u, EDIT_BAD_LEN = 2u, EDIT_BAD_ROWS = 4u;   // bits of the flag word
constexpr uint32_t EDIT_CODE_MASK = (1u << BCE_EDIT_CODE_BITS) - 1u;

static_assert(BCE_EDIT_MAX_K == BCE_HIP_EDIT_MAX_K, "edit_step.h and bce_hip.h name one bound");
static_assert(BCE_HIP_EDIT_MAX_PATTERNS <= (1u << (32u - BCE_EDIT_CODE_BITS)), "the pattern id rides above the code");
static_assert(BCE_HIP_EDIT_MAX_LEN + BCE_HIP_EDIT_MAX_K <= 0xFFFFu, "a length is 16 bits");

// pat[0, pos) to the left of two intervals together: near_finish twice, the two chains of ranks in flight side by side.  An empty
// interval stays empty under a step (both ends move monotonically), so neither needs a guard; the loop ends when both are empty.
__device__ __forceinline__ void edit_finish2(const PlaneRank &R, const Zeros8 &z, const uint8_t *pat, uint64_t pos, uint32_t &a1, uint32_t &b1,
                                             uint32_t &a2, uint32_t &b2) {
  uint32_t c = pos ? pat[pos - 1] : 0u;
  for (uint64_t j = pos; j > 0 && (a1 < b1 || a2 < b2); --j) {
    const uint32_t next = j > 1 ? pat[j - 2] : 0u;
    fm_step(c, z.v, a1, b1, R);
    fm_step(c, z.v, a2, b2, R);
    c = next;
  }
}

// The branch whose edit spends the budget, at the wave-uniform node (lo, hi, pos), pos > 0, reached by `came`: every lane takes
// four candidate bytes and finishes their children; the wave emits the substitutions, the insertions and (in the round of the
// pattern's own byte) the deletion, at distance d.
template <class Emit>
__device__ __forceinline__ void edit_last_branch(const PlaneRank &R, const Zeros8 &z, const uint8_t *pat, uint64_t m, uint32_t lo, uint32_t hi,
                                                 uint64_t pos, uint32_t d, uint32_t loff, uint32_t came, uint32_t lane, Emit &&emit) {
  const uint32_t own = pat[pos - 1];
  const bool ins_ok = edit_may_insert(pos, m) && came != EDIT_BY_DEL, del_ok = edit_may_delete(pos, m) && came != EDIT_BY_INS;
  for (uint32_t q = 0; q < 4u; ++q) {
    const uint32_t c = lane + 64u * q;
    const bool mine = c == own;
    uint32_t a, b, a1 = 0, b1 = 0, a2 = 0, b2 = 0;
    const bool live = near_child(c, z.v, lo, hi, a, b, R);
    if (live && !mine) { a1 = a; b1 = b; }
    if (mine && del_ok) { a1 = lo; b1 = hi; }                        // the deletion: the node's own interval, P[pos - 1] skipped
    if (live && ins_ok) { a2 = a; b2 = b; fm_step(own, z.v, a2, b2, R); }   // the insertion: P[pos - 1] is still to come
    edit_finish2(R, z, pat, pos - 1, a1, b1, a2, b2);
    const uint32_t r1 = b1 > a1 ? b1 - a1 : 0u;
    emit(a1, mine ? 0u : r1, d, loff);
    if (ins_ok) emit(a2, b2 > a2 ? b2 - a2 : 0u, d, loff + 1u);
    if (del_ok && (own >> 6) == q) emit(a1, mine ? r1 : 0u, d, loff - 1u);
  }
}

// One pattern by one wave.  emit(lo, rows, d, loff) is called by all 64 lanes together: lane l brings the candidate rows
// [lo, lo + rows) at distance d and length m + loff - k (rows == 0: nothing); d and loff are wave-uniform.
template <class Emit>
__device__ __forceinline__ void edit_wave(const PlaneRank &R, const Zeros8 &z, const uint8_t *pat, uint64_t m, uint32_t n, uint32_t k, uint32_t lane,
                                          Emit &&emit) {
  uint32_t lo0 = 0, hi0 = n;
  uint64_t pos0 = m;
  if (k == 0) { near_finish(pat, m, z.v, lo0, hi0, R); pos0 = 0; }
  while (pos0 > 0 && lo0 < hi0) {
    const uint32_t own = pat[pos0 - 1];
    if (k == 1) {
      edit_last_branch(R, z, pat, m, lo0, hi0, pos0, 1u, k, EDIT_BY_STEP, lane, emit);
    } else {
      const bool ins_ok = edit_may_insert(pos0, m), del_ok = edit_may_delete(pos0, m);
      for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t c = lane + 64u * q;
        uint32_t a = 0, b = 0;
        const bool live = near_child(c, z.v, lo0, hi0, a, b, R);
        const uint64_t subs = __ballot(live && c != own), inss = __ballot(live);
        for (uint32_t kind = EDIT_BY_STEP; kind <= EDIT_BY_DEL; ++kind) {   // the children by kind: each the next frame, one edit in
          uint64_t todo = kind == EDIT_BY_STEP ? subs : kind == EDIT_BY_INS ? (ins_ok ? inss : 0ull) : (del_ok && q == 0 ? 1ull : 0ull);
          for (; todo; todo &= todo - 1) {
            const int l = __ffsll((unsigned long long)todo) - 1;
            const uint32_t la = from_lane(a, l), lb = from_lane(b, l);
            uint32_t lo1 = kind == EDIT_BY_DEL ? lo0 : la, hi1 = kind == EDIT_BY_DEL ? hi0 : lb;
            uint64_t pos1 = kind == EDIT_BY_INS ? pos0 : pos0 - 1;
            const uint32_t loff1 = kind == EDIT_BY_INS ? k + 1u : kind == EDIT_BY_DEL ? k - 1u : k;
            uint32_t came = kind;
            while (pos1 > 0 && lo1 < hi1) {
              edit_last_branch(R, z, pat, m, lo1, hi1, pos1, 2u, loff1, came, lane, emit);
              fm_step(pat[pos1 - 1], z.v, lo1, hi1, R);
              lo1 = uni(lo1); hi1 = uni(hi1);
              --pos1;
              came = EDIT_BY_STEP;
            }
            emit(lo1, lane == 0 && hi1 > lo1 ? hi1 - lo1 : 0u, 1u, loff1);
          }
        }
      }
    }
    fm_step(own, z.v, lo0, hi0, R);
    lo0 = uni(lo0); hi0 = uni(hi0);
    --pos0;
  }
  emit(lo0, lane == 0 && hi0 > lo0 ? hi0 - lo0 : 0u, 0u, k);
}

// the wave's pattern: false when there is none, or its offsets are refused (then the flag word says why)
__device__ __forceinline__ bool edit_pattern(const uint64_t *off, uint32_t npat, uint32_t *bad, uint32_t &p, uint64_t &b, uint64_t &m) {
  p = blockIdx.x * EDIT_WAVES + (threadIdx.x >> 6);
  if (p >= npat) return false;
  b = off[p];
  const uint64_t e = off[(size_t)p + 1];
  m = e - b;
  if (e < b) { if ((threadIdx.x & 63u) == 0) atomicOr(bad, EDIT_BAD_ORDER); return false; }
  if (m > BCE_HIP_EDIT_MAX_LEN) { if ((threadIdx.x & 63u) == 0) atomicOr(bad, EDIT_BAD_LEN); return false; }
  return true;
}

// cnt[p] = the candidate rows of pattern p (more than 2^32 - 1: the flag word says so)
__global__ __launch_bounds__(EDIT_T) void edit_size_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                           const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint32_t npat,
                                                           uint32_t k, uint32_t *__restrict__ cnt, uint32_t *__restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p;
  uint64_t b, m;
  const bool run = edit_pattern(off, npat, bad, p, b, m);
  if (p >= npat) return;
  uint64_t mine = 0;
  if (run) edit_wave(PlaneRank{gran, ngran}, z, pat + b, m, n, k, lane, [&](uint32_t, uint32_t rows, uint32_t, uint32_t) { mine += rows; });
  const uint64_t rows = wave_sum64(mine);
  if (lane == 0) {
    cnt[p] = (uint32_t)rows;
    if (rows > 0xFFFFFFFFull) atomicOr(bad, EDIT_BAD_ROWS);
  }
}

// key[r], val[r] = (position, p << 4 | code) of every candidate row r of pattern p's segment [start[p], start[p + 1]), in the order
// of the walk.  sa == nullptr: the text of one byte, whose only rotation starts at 0.
__global__ __launch_bounds__(EDIT_T) void edit_fill_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                           const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint32_t npat,
                                                           uint32_t k, uint32_t linear, const uint32_t *__restrict__ sa,
                                                           const uint64_t *__restrict__ start, uint32_t *__restrict__ key,
                                                           uint32_t *__restrict__ val) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * EDIT_WAVES + (threadIdx.x >> 6);
  if (p >= npat) return;
  const uint64_t b = off[p], e = off[(size_t)p + 1], m = e - b;
  if (e < b || m > BCE_HIP_EDIT_MAX_LEN) return;                       // (the size pass has refused such a batch: never taken, and no flag to raise)
  uint64_t cur = start[p];
  const uint64_t end = start[(size_t)p + 1];                          // (the size pass found as many rows: nothing is written past it)
  edit_wave(PlaneRank{gran, ngran}, z, pat + b, m, n, k, lane, [&](uint32_t lo, uint32_t rows, uint32_t d, uint32_t loff) {
    const uint64_t len = edit_length(m, k, loff);
    const uint32_t code = edit_code(d, loff);
    cur += wave_rows(lo, rows, lane, [&](uint32_t o, uint32_t row) {
      const uint64_t r = cur + o;
      const uint32_t pos = sa ? sa[row] : 0u;
      if (r < end) { key[r] = pos; val[r] = p << BCE_EDIT_CODE_BITS | (linear && pos + len > n ? BCE_EDIT_DEAD : code); }
    });
  });
}

// is the sorted record r of the segment that begins at s a head: live, and the first of its position
__device__ __forceinline__ bool edit_head(const uint32_t *pos, const uint32_t *tag, uint64_t s, uint64_t r, uint32_t &code) {
  code = tag[r] & EDIT_CODE_MASK;
  return code != BCE_EDIT_DEAD && (r == s || pos[r - 1] != pos[r]);
}

// hitcnt[p] (unless null) = the heads of pattern p's sorted segment; counts[p * (k + 1) + d] (unless null) = those at distance d
__global__ __launch_bounds__(EDIT_T) void edit_heads_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ tag,
                                                            const uint64_t *__restrict__ seg, uint32_t npat, uint32_t k,
                                                            uint32_t *__restrict__ hitcnt, uint64_t *__restrict__ counts) {
  const uint32_t lane = threadIdx.x & 63u, p = blockIdx.x * EDIT_WAVES + (threadIdx.x >> 6);
  if (p >= npat) return;
  const uint64_t s = seg[p], e = seg[(size_t)p + 1];
  uint64_t per[BCE_EDIT_MAX_K + 1] = {0, 0, 0};
  for (uint64_t r = s + lane; r < e; r += 64u) {
    uint32_t code;
    if (edit_head(pos, tag, s, r, code)) near_tally(per, edit_code_dist(code), 1u);
  }
  uint64_t all = 0;
#pragma unroll
  for (uint32_t d = 0; d <= BCE_EDIT_MAX_K; ++d) {
    const uint64_t sum = wave_sum64(per[d]);
    all += sum;
    if (lane == 0 && d <= k && counts) counts[(size_t)p * (k + 1) + d] = sum;
  }
  if (lane == 0 && hitcnt) hitcnt[p] = (uint32_t)all;                  // (at most n: a position is a head once)
}

// the heads of pattern p's sorted segment, in order, to hits[p] and on: positions, lengths, distances
__global__ __launch_bounds__(EDIT_T) void edit_out_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ tag,
                                                          const uint64_t *__restrict__ seg, const uint64_t *__restrict__ hits,
                                                          const uint64_t *__restrict__ off, uint32_t npat, uint32_t k,
                                                          uint32_t *__restrict__ out_pos, uint16_t *__restrict__ out_len,
                                                          uint8_t *__restrict__ out_dist) {
  const uint32_t lane = threadIdx.x & 63u, p = blockIdx.x * EDIT_WAVES + (threadIdx.x >> 6);
  if (p >= npat) return;
  const uint64_t s = seg[p], e = seg[(size_t)p + 1], m = off[(size_t)p + 1] - off[p];
  uint64_t cur = hits[p];
  const uint64_t end = hits[(size_t)p + 1];                           // (the heads kernel counted as many: nothing is written past it)
  for (uint64_t base = s; base < e; base += 64u) {
    const uint64_t r = base + lane;
    uint32_t code = 0;
    const bool head = r < e && edit_head(pos, tag, s, r, code);
    const uint64_t mask = __ballot(head);
    const uint64_t o = cur + __popcll(mask & ((1ull << lane) - 1ull));
    if (head && o < end) {
      out_pos[o] = pos[r];
      out_len[o] = (uint16_t)edit_length(m, k, edit_code_loff(code));
      out_dist[o] = (uint8_t)edit_code_dist(code);
    }
    cur += __popcll(mask);
  }
}

uint32_t wave_grid(uint32_t npat) { return (uint32_t)(((uint64_t)npat + EDIT_WAVES - 1) / EDIT_WAVES); }

// the flag word after a kernel: which refusal, if any (waits for the stream)
int edit_verdict(bce_hip_ctx *c, const uint32_t *d_bad, const char *what) {
  uint32_t bad = 0;
  BCE_TRY(read_back(c, &bad, d_bad, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  if (bad & EDIT_BAD_ORDER) { snprintf(c->err, sizeof c->err, "%s: pattern offsets decrease", what); return BCE_HIP_E_ARG; }
  if (bad & EDIT_BAD_LEN) { snprintf(c->err, sizeof c->err, "%s: a pattern of more than %u bytes", what, BCE_HIP_EDIT_MAX_LEN); return BCE_HIP_E_ARG; }
  if (bad & EDIT_BAD_ROWS) { snprintf(c->err, sizeof c->err, "%s: a pattern has more than 2^32 - 1 candidate rows", what); return BCE_HIP_E_OVERFLOW; }
  return BCE_HIP_OK;
}

int edit_flag(bce_hip_ctx *c, uint32_t **d_bad) {
  BCE_TRY(ensure(c, c->qbuf[qb::edit_res], 8));
  *d_bad = c->qbuf[qb::edit_res].as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(*d_bad, 0, 8, c->stream));
  return BCE_HIP_OK;
}

// size, fill and order: the batch's candidates sorted, pattern p's in [seg[p], seg[p + 1]) of (*pos, *tag), seg = loc_start.
// Offsets that decrease, a pattern of more than BCE_HIP_EDIT_MAX_LEN bytes: BCE_HIP_E_ARG; more than 2^31 - 1 candidate rows in the
// batch: BCE_HIP_E_OVERFLOW.
int edit_candidates(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                    const char *what, const uint32_t **pos, const uint32_t **tag) {
  BCE_TRY(ensure(c, c->qbuf[qb::loc_res], 16));                                // (locate_scan's total word)
  BCE_TRY(ensure(c, c->qbuf[qb::loc_cnt], (size_t)npat * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::loc_start], ((size_t)npat + 1) * 8));
  uint32_t *cnt = c->qbuf[qb::loc_cnt].as<uint32_t>();
  uint64_t *seg = c->qbuf[qb::loc_start].as<uint64_t>();
  uint32_t *d_bad = nullptr;
  BCE_TRY(edit_flag(c, &d_bad));
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  hipLaunchKernelGGL(edit_size_kernel, dim3(wave_grid(npat)), dim3(EDIT_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off,
                     npat, k, cnt, d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(edit_verdict(c, d_bad, what));
  uint64_t rows = 0;
  BCE_TRY(locate_scan(c, cnt, nullptr, npat, seg, &rows));
  if (rows > EDIT_MAXROWS) {
    snprintf(c->err, sizeof c->err, "%s: the batch has %llu candidate rows, one call reduces at most 2^31 - 1", what, (unsigned long long)rows);
    return BCE_HIP_E_OVERFLOW;
  }
  const uint32_t nrows = (uint32_t)rows;
  const size_t rbytes = (size_t)nrows * 4;
  for (DevBuf *b : {&c->qbuf[qb::loc_key0], &c->qbuf[qb::loc_key1], &c->qbuf[qb::loc_val0], &c->qbuf[qb::loc_val1]}) BCE_TRY(ensure(c, *b, rbytes ? rbytes : 4));
  uint32_t *key[2] = {c->qbuf[qb::loc_key0].as<uint32_t>(), c->qbuf[qb::loc_key1].as<uint32_t>()};
  uint32_t *val[2] = {c->qbuf[qb::loc_val0].as<uint32_t>(), c->qbuf[qb::loc_val1].as<uint32_t>()};
  *pos = key[0]; *tag = val[0];
  if (nrows == 0) return BCE_HIP_OK;
  hipLaunchKernelGGL(edit_fill_kernel, dim3(wave_grid(npat)), dim3(EDIT_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off,
                     npat, k, linear ? 1u : 0u, sa, seg, key[0], val[0]);
  BCE_HIP_TRY(c, hipGetLastError());
  uint32_t *t1[2] = {val[0], val[1]}, *p1[2] = {key[0], key[1]};
  int r1 = 0;
  BCE_TRY(radix_sort_pairs(c, t1, p1, nrows, 0, BCE_EDIT_CODE_BITS, &r1, 9));               // the least (edits, length) first
  uint32_t *p2[2] = {p1[r1], p1[r1 ^ 1]}, *t2[2] = {t1[r1], t1[r1 ^ 1]};
  int r2 = 0;
  BCE_TRY(radix_sort_pairs(c, p2, t2, nrows, 0, ceil_log2(c->n), &r2, 9));                  // positions ascending
  *pos = p2[r2]; *tag = t2[r2];
  if (npat > 1) {                                                    // stably back into patterns, on the bits above the code
    uint32_t *t3[2] = {t2[r2], t2[r2 ^ 1]}, *p3[2] = {p2[r2], p2[r2 ^ 1]};
    int r3 = 0;
    BCE_TRY(radix_sort_pairs(c, t3, p3, nrows, BCE_EDIT_CODE_BITS, ceil_log2(npat), &r3, 9));
    *pos = p3[r3]; *tag = t3[r3];
  }
  return BCE_HIP_OK;
}

}  // namespace

// d_out[p * (k + 1) + d] = the hits at distance exactly d <= k of d_pat[d_off[p], d_off[p + 1]), p < npat: the positions of the text
// of the context's planes and suffix array (sa: K1's, or null for a text of one byte) whose least anchored edit distance is d,
// in linear mode over the alignments that end inside the text.  All three arrays: device memory of the context's device.  Queued
// on the context's stream; the caller waits.  k <= BCE_HIP_EDIT_MAX_K and npat <= BCE_HIP_EDIT_MAX_PATTERNS are the caller's to check.
int kd_edit_count(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                  uint64_t *d_out) {
  if (npat == 0) return BCE_HIP_OK;
  const uint32_t *pos = nullptr, *tag = nullptr;
  BCE_TRY(edit_candidates(c, sa, d_pat, d_off, npat, k, linear, "count_edit", &pos, &tag));
  hipLaunchKernelGGL(edit_heads_kernel, dim3(wave_grid(npat)), dim3(EDIT_T), 0, c->stream, pos, tag, c->qbuf[qb::loc_start].as<uint64_t>(), npat, k,
                     (uint32_t *)nullptr, d_out);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// First half of a locate: the whole search and the reduce's counts.  d_hits[0, npat] receives the CSR offsets of the hits, *total
// their last word, exact in both modes.  Complete on return.  Leaves the sorted candidates for kd_edit_fill in the loc_* buffers.
int kd_edit_size(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                 uint64_t *d_hits, uint64_t *total, const uint32_t **pos, const uint32_t **tag) {
  BCE_TRY(edit_candidates(c, sa, d_pat, d_off, npat, k, linear, "locate_edit", pos, tag));
  BCE_TRY(ensure(c, c->qbuf[qb::edit_cnt], (size_t)npat * 4));
  uint32_t *hitcnt = c->qbuf[qb::edit_cnt].as<uint32_t>();
  hipLaunchKernelGGL(edit_heads_kernel, dim3(wave_grid(npat)), dim3(EDIT_T), 0, c->stream, *pos, *tag, c->qbuf[qb::loc_start].as<uint64_t>(), npat, k,
                     hitcnt, (uint64_t *)nullptr);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(locate_scan(c, hitcnt, nullptr, npat, d_hits, total));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BCE_HIP_OK;
}

// Second half, straight after kd_edit_size of the same batch (its pos, tag and total, d_hits unchanged): d_pos, d_len,
// d_dist[0, total) receive the hits, each pattern's by ascending position.  Complete on return.
int kd_edit_fill(bce_hip_ctx *c, const uint64_t *d_off, uint32_t npat, uint32_t k, const uint64_t *d_hits, uint64_t total, const uint32_t *pos,
                 const uint32_t *tag, uint32_t *d_pos, uint16_t *d_len, uint8_t *d_dist) {
  if (total == 0) return BCE_HIP_OK;
  hipLaunchKernelGGL(edit_out_kernel, dim3(wave_grid(npat)), dim3(EDIT_T), 0, c->stream, pos, tag, c->qbuf[qb::loc_start].as<uint64_t>(), d_hits, d_off,
                     npat, k, d_pos, d_len, d_dist);
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
