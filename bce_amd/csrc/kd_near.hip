// kd_near.hip -- how often, and where, byte strings occur in the circular text within k mismatches (Hamming distance), from the K2
// planes and K1's suffix array (bce_hip_count_near / _locate_near and their _device forms, `bce -gn` / `-gnl`).
//
// The search is near_step.h's: backward search that branches.  Here a WAVE walks one pattern's tree:
//   - The frames (a node with budget left: interval, position) are wave-uniform.  At a frame's position the 64 lanes share the 256
//     candidate bytes, four near_child steps each: 64 independent gather chains in flight, so the rank latency is hidden by the
//     wave's own width, not by occupancy as in count_kernel.  A ballot keeps the children that have rows.
//   - Budget spent by that mismatch (k = 1, or the second mismatch of k = 2): each lane finishes its own child with near_finish
//     and the wave hands the 64 intervals to the kernel's emit together.
//   - Budget left (k = 2 after the first mismatch): the surviving children become the next frame one by one, read from their
//     lane's registers by the ballot's order.  All children of one branch stand at the same position, so a child is two words
//     in the lane that found it: the queue of at most 255 children is the wave's registers, and needs neither LDS nor a fence
//     (DESIGN.md 4.17).  Memory per wave does not depend on n, m or the number of answers.
//   - k = 0 is near_finish from the root: count_kernel's chain, one wave wide.
// lo and hi stay in [0, n] on every level, as in count_kernel: every granule index is below ngran whatever the pattern's bytes.
//
// Kernels, all one wave per pattern, four patterns a workgroup:
//   count   per[d] = rows at distance d, reduced over the wave: counts[p * (k + 1) + d].
//   size    the pattern's rows, and in linear mode those whose hit runs across the end of the text (read from sa over the
//           intervals found, as kd_locate.hip's sizing pass).  kd_locate.hip's scan (locate_scan) makes the CSR offsets of both.
//   fill    the search again; the wave writes (sa[row], pattern id << 2 | d) of every answer at a cursor of its own inside the
//           pattern's segment: no atomics.  Then the locate's order -- two stable radix_sort_pairs, on the position bits and on
//           the pattern-id bits above the distance's two -- and one pass that splits the pairs into positions and distances,
//           keeping in linear mode the first rows of each sorted segment (those across the end are its largest positions).
// Intervals of up to WAVE_SERIAL rows (wave_walk.h) are read by the lane that found them, wider ones by the whole wave, 64 neighbouring words at a time.
// Everything written is the locate's scratch (qb::loc_* of c->qbuf: the two calls never run together), near_res or the caller's outputs.
#include "common.h"
#include "near_step.h"
#include "scan_util.h"
#include "wave_walk.h"

namespace bce {

namespace {

constexpr int NEAR_T = 256;                  // lanes per workgroup (4 waves = 4 patterns)
constexpr uint32_t NEAR_WAVES = NEAR_T / 64;
constexpr uint32_t NEAR_MAXGRID = 8192;      // grid-stride kernels: workgroups at most
constexpr uint64_t NEAR_MAXROWS = 0x7FFFFFFFull;
constexpr uint32_t NEAR_BAD_ORDER = 1u, NEAR_BAD_LEN = 2u;   // bits of the flag word

static_assert(BCE_NEAR_MAX_K == BCE_HIP_NEAR_MAX_K, "near_step.h and bce_hip.h name one bound");

// The branch whose mismatch spends the budget, at the wave-uniform node (lo, hi, pos), pos > 0: every lane takes four candidate
// bytes, finishes the children that have rows, and the wave emits 64 intervals (most of them empty) four times, at distance d.
template <class Emit>
__device__ __forceinline__ void near_last_branch(const PlaneRank &R, const Zeros8 &z, const uint8_t *pat, uint32_t lo, uint32_t hi, uint64_t pos,
                                                 uint32_t d, uint32_t lane, Emit &&emit) {
  const uint32_t own = pat[pos - 1];
  for (uint32_t q = 0; q < 4u; ++q) {
    const uint32_t c = lane + 64u * q;
    uint32_t a = 0, b = 0;
    if (c != own && near_child(c, z.v, lo, hi, a, b, R)) near_finish(pat, pos - 1, z.v, a, b, R);
    emit(a, b > a ? b - a : 0u, d);
  }
}

// One pattern by one wave.  emit(lo, rows, d) is called by all 64 lanes together: lane l brings the rows [lo, lo + rows) at
// distance d (rows == 0: nothing); d is wave-uniform.
template <class Emit>
__device__ __forceinline__ void near_wave(const PlaneRank &R, const Zeros8 &z, const uint8_t *pat, uint64_t m, uint32_t n, uint32_t k, uint32_t lane,
                                          Emit &&emit) {
  uint32_t lo0 = 0, hi0 = n;
  uint64_t pos0 = m;
  if (k == 0) { near_finish(pat, m, z.v, lo0, hi0, R); pos0 = 0; }
  while (pos0 > 0 && lo0 < hi0) {
    const uint32_t own = pat[pos0 - 1];
    if (k == 1) {
      near_last_branch(R, z, pat, lo0, hi0, pos0, 1u, lane, emit);
    } else {
      for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t c = lane + 64u * q;
        uint32_t a = 0, b = 0;
        const bool live = c != own && near_child(c, z.v, lo0, hi0, a, b, R);
        for (uint64_t todo = __ballot(live); todo; todo &= todo - 1) {   // each child with rows: the next frame, one mismatch in
          const int l = __ffsll((unsigned long long)todo) - 1;
          uint32_t lo1 = from_lane(a, l), hi1 = from_lane(b, l);
          uint64_t pos1 = pos0 - 1;
          while (pos1 > 0 && lo1 < hi1) {
            near_last_branch(R, z, pat, lo1, hi1, pos1, 2u, lane, emit);
            fm_step(pat[pos1 - 1], z.v, lo1, hi1, R);
            lo1 = uni(lo1); hi1 = uni(hi1);
            --pos1;
          }
          emit(lo1, lane == 0 && hi1 > lo1 ? hi1 - lo1 : 0u, 1u);
        }
      }
    }
    fm_step(own, z.v, lo0, hi0, R);
    lo0 = uni(lo0); hi0 = uni(hi0);
    --pos0;
  }
  emit(lo0, lane == 0 && hi0 > lo0 ? hi0 - lo0 : 0u, 0u);
}

// the wave's pattern: false when there is none, or its offsets are refused (then the flag word says why)
__device__ __forceinline__ bool near_pattern(const uint64_t *off, uint32_t npat, uint32_t *bad, uint32_t &p, uint64_t &b, uint64_t &m) {
  p = blockIdx.x * NEAR_WAVES + (threadIdx.x >> 6);
  if (p >= npat) return false;
  b = off[p];
  const uint64_t e = off[(size_t)p + 1];
  m = e - b;
  if (e < b) { if ((threadIdx.x & 63u) == 0) atomicOr(bad, NEAR_BAD_ORDER); return false; }
  if (m > BCE_HIP_NEAR_MAX_LEN) { if ((threadIdx.x & 63u) == 0) atomicOr(bad, NEAR_BAD_LEN); return false; }
  return true;
}

__global__ __launch_bounds__(NEAR_T) void near_count_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                            const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint32_t npat,
                                                            uint32_t k, uint64_t *__restrict__ out, uint32_t *__restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p;
  uint64_t b, m;
  uint64_t per[BCE_NEAR_MAX_K + 1] = {0, 0, 0};
  const bool run = near_pattern(off, npat, bad, p, b, m);
  if (p >= npat) return;
  if (run) near_wave(PlaneRank{gran, ngran}, z, pat + b, m, n, k, lane, [&](uint32_t, uint32_t rows, uint32_t d) { near_tally(per, d, rows); });
#pragma unroll
  for (uint32_t d = 0; d <= BCE_NEAR_MAX_K; ++d) {
    const uint64_t s = wave_sum64(per[d]);
    if (lane == 0 && d <= k) out[(size_t)p * (k + 1) + d] = s;
  }
}

// cnt[p] = the rows of pattern p; drop != nullptr (linear mode): drop[p] = those whose hit does not end inside the text.
// sa == nullptr: the text of one byte, whose only rotation starts at 0.
__global__ __launch_bounds__(NEAR_T) void near_size_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                           const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint32_t npat,
                                                           uint32_t k, const uint32_t *__restrict__ sa, uint32_t *__restrict__ cnt,
                                                           uint32_t *__restrict__ drop, uint32_t *__restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p;
  uint64_t b, m;
  const bool run = near_pattern(off, npat, bad, p, b, m);
  if (p >= npat) return;
  uint32_t mine = 0, out = 0;                                         // this lane's rows, and those of them across the end
  if (run) near_wave(PlaneRank{gran, ngran}, z, pat + b, m, n, k, lane, [&](uint32_t lo, uint32_t rows, uint32_t) {
    mine += rows;
    if (drop) wave_rows(lo, rows, lane, [&](uint32_t, uint32_t row) { out += !fm_linear_hit(sa ? sa[row] : 0u, m, n); });
  });
  const uint64_t rows = wave_sum64(mine), across = wave_sum64(out);
  if (lane == 0) { cnt[p] = (uint32_t)rows; if (drop) drop[p] = (uint32_t)across; }
}

// key[r], val[r] = (position, p << 2 | distance) of every row r of pattern p's segment [start[p], start[p + 1]), in the order of the walk
__global__ __launch_bounds__(NEAR_T) void near_fill_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                           const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint32_t npat,
                                                           uint32_t k, const uint32_t *__restrict__ sa, const uint64_t *__restrict__ start,
                                                           uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint32_t *__restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p;
  uint64_t b, m;
  if (!near_pattern(off, npat, bad, p, b, m)) return;
  uint64_t cur = start[p];
  const uint64_t end = start[(size_t)p + 1];                          // (the size pass found as many rows: nothing is written past it)
  near_wave(PlaneRank{gran, ngran}, z, pat + b, m, n, k, lane, [&](uint32_t lo, uint32_t rows, uint32_t d) {
    cur += wave_rows(lo, rows, lane, [&](uint32_t o, uint32_t row) {
      const uint64_t r = cur + o;
      if (r < end) { key[r] = sa ? sa[row] : 0u; val[r] = p << 2 | d; }
    });
  });
}

// After the sorts: hit o < total of pattern p is the (o - hits[p])-th of p's sorted segment, which begins at cyc[p] (hits ==
// nullptr: cyclic mode, every row is a hit and o is its place).
__global__ __launch_bounds__(NEAR_T) void near_out_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ val,
                                                          const uint64_t *__restrict__ cyc, const uint64_t *__restrict__ hits, uint32_t npat,
                                                          uint64_t total, uint32_t *__restrict__ out_pos, uint8_t *__restrict__ out_dist) {
  for (uint64_t o = (uint64_t)blockIdx.x * NEAR_T + threadIdx.x; o < total; o += (uint64_t)gridDim.x * NEAR_T) {
    uint64_t s = o;
    if (hits) { const uint32_t p = fm_row_pattern(hits, npat, o); s = cyc[p] + (o - hits[p]); }
    out_pos[o] = pos[s];
    out_dist[o] = (uint8_t)(val[s] & 3u);
  }
}

uint32_t wave_grid(uint32_t npat) { return (uint32_t)(((uint64_t)npat + NEAR_WAVES - 1) / NEAR_WAVES); }

// the flag word after a kernel: which refusal, if any (waits for the stream)
int near_verdict(bce_hip_ctx *c, const uint32_t *d_bad, const char *what) {
  uint32_t bad = 0;
  BCE_TRY(read_back(c, &bad, d_bad, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  if (bad & NEAR_BAD_ORDER) { snprintf(c->err, sizeof c->err, "%s: pattern offsets decrease", what); return BCE_HIP_E_ARG; }
  if (bad & NEAR_BAD_LEN) { snprintf(c->err, sizeof c->err, "%s: a pattern of more than %u bytes", what, BCE_HIP_NEAR_MAX_LEN); return BCE_HIP_E_ARG; }
  return BCE_HIP_OK;
}

int near_flag(bce_hip_ctx *c, uint32_t **d_bad) {
  BCE_TRY(ensure(c, c->qbuf[qb::near_res], 8));
  *d_bad = c->qbuf[qb::near_res].as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(*d_bad, 0, 8, c->stream));
  return BCE_HIP_OK;
}

}  // namespace

// d_out[p * (k + 1) + d] = the i in [0, n) at Hamming distance exactly d <= k of d_pat[d_off[p], d_off[p + 1]), p < npat, in the
// circular text of the context's planes.  All three arrays: device memory of the context's device.  Queued on the context's stream;
// returns when the kernel is through (the flag word's way back is the wait).  Offsets that decrease, a pattern of more than
// BCE_HIP_NEAR_MAX_LEN bytes: BCE_HIP_E_ARG.  k <= BCE_HIP_NEAR_MAX_K is the caller's to check.
int kd_near_count(bce_hip_ctx *c, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, uint64_t *d_out) {
  if (npat == 0) return BCE_HIP_OK;
  uint32_t *d_bad = nullptr;
  BCE_TRY(near_flag(c, &d_bad));
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  hipLaunchKernelGGL(near_count_kernel, dim3(wave_grid(npat)), dim3(NEAR_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off,
                     npat, k, d_out, d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  return near_verdict(c, d_bad, "count_near");
}

// First half of a locate, as kd_locate_size: d_hits[0, npat] receives the CSR offsets of the hits, *total their last word -- exact
// in both modes -- and *rows the batch's cyclic rows.  Complete on return.  The refusals of kd_near_count; more than 2^31 - 1 rows:
// BCE_HIP_E_OVERFLOW, with d_hits and *total written.  Leaves what kd_near_fill needs in loc_start / loc_lin.
int kd_near_size(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                 uint64_t *d_hits, uint64_t *rows, uint64_t *total) {
  const size_t words = (size_t)npat * 4, starts = ((size_t)npat + 1) * 8;
  BCE_TRY(ensure(c, c->qbuf[qb::loc_res], 16));                                // (locate_scan's total word)
  BCE_TRY(ensure(c, c->qbuf[qb::loc_cnt], words));
  BCE_TRY(ensure(c, c->qbuf[qb::loc_start], starts));
  uint32_t *cnt = c->qbuf[qb::loc_cnt].as<uint32_t>(), *drop = nullptr;
  uint64_t *cyc = c->qbuf[qb::loc_start].as<uint64_t>();
  if (linear) {
    BCE_TRY(ensure(c, c->qbuf[qb::loc_drop], words));
    BCE_TRY(ensure(c, c->qbuf[qb::loc_lin], starts));
    drop = c->qbuf[qb::loc_drop].as<uint32_t>();
  }
  uint32_t *d_bad = nullptr;
  BCE_TRY(near_flag(c, &d_bad));
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  hipLaunchKernelGGL(near_size_kernel, dim3(wave_grid(npat)), dim3(NEAR_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off,
                     npat, k, sa, cnt, drop, d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(near_verdict(c, d_bad, "locate_near"));
  BCE_TRY(locate_scan(c, cnt, nullptr, npat, cyc, rows));
  const uint64_t *hits = cyc;
  *total = *rows;
  if (linear) {
    hits = c->qbuf[qb::loc_lin].as<uint64_t>();
    BCE_TRY(locate_scan(c, cnt, drop, npat, c->qbuf[qb::loc_lin].as<uint64_t>(), total));
  }
  BCE_HIP_TRY(c, hipMemcpyAsync(d_hits, hits, starts, hipMemcpyDeviceToDevice, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*rows > NEAR_MAXROWS) {
    snprintf(c->err, sizeof c->err, "locate_near: the batch has %llu rows, one call gathers at most 2^31 - 1", (unsigned long long)*rows);
    return BCE_HIP_E_OVERFLOW;
  }
  return BCE_HIP_OK;
}

// Second half, straight after kd_near_size of the same batch (its rows <= 2^31 - 1 and total): d_pos[0, total) receives the
// positions, each pattern's ascending, d_dist[0, total) their distances.  npat <= 2^30: the distance rides in the two low bits of
// the pattern-id word through the sorts.  Complete on return.
int kd_near_fill(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint32_t k, bool linear,
                 uint64_t rows, uint64_t total, uint32_t *d_pos, uint8_t *d_dist) {
  if (total == 0) return BCE_HIP_OK;
  const uint32_t nrows = (uint32_t)rows;
  const size_t rbytes = (size_t)nrows * 4;
  for (DevBuf *b : {&c->qbuf[qb::loc_key0], &c->qbuf[qb::loc_key1], &c->qbuf[qb::loc_val0], &c->qbuf[qb::loc_val1]}) BCE_TRY(ensure(c, *b, rbytes));
  uint32_t *key[2] = {c->qbuf[qb::loc_key0].as<uint32_t>(), c->qbuf[qb::loc_key1].as<uint32_t>()};
  uint32_t *val[2] = {c->qbuf[qb::loc_val0].as<uint32_t>(), c->qbuf[qb::loc_val1].as<uint32_t>()};
  const uint64_t *cyc = c->qbuf[qb::loc_start].as<uint64_t>();
  uint32_t *d_bad = nullptr;
  BCE_TRY(near_flag(c, &d_bad));
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  hipLaunchKernelGGL(near_fill_kernel, dim3(wave_grid(npat)), dim3(NEAR_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off,
                     npat, k, sa, cyc, key[0], val[0], d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  int res = 0;
  BCE_TRY(radix_sort_pairs(c, key, val, nrows, 0, ceil_log2(c->n), &res, 9));     // positions ascending
  const uint32_t *pos = key[res], *tag = val[res];
  if (npat > 1) {                                                    // stably back into patterns, on the bits above the distance
    uint32_t *k2[2] = {val[res], val[res ^ 1]}, *v2[2] = {key[res], key[res ^ 1]};
    int r2 = 0;
    BCE_TRY(radix_sort_pairs(c, k2, v2, nrows, 2, ceil_log2(npat), &r2, 9));
    pos = v2[r2]; tag = k2[r2];
  }
  const uint64_t g = (total + NEAR_T - 1) / NEAR_T;
  hipLaunchKernelGGL(near_out_kernel, dim3((uint32_t)(g < NEAR_MAXGRID ? g : NEAR_MAXGRID)), dim3(NEAR_T), 0, c->stream, pos, tag, cyc,
                     linear ? c->qbuf[qb::loc_lin].as<uint64_t>() : (const uint64_t *)nullptr, npat, total, d_pos, d_dist);
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
