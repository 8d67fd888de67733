// kd_locate.hip -- where byte strings occur in the text, from the K2 planes and K1's suffix array (bce_hip_locate / _locate_device,
// `bce -gl`).
//
// Backward search (fm_step.h) ends at an interval [lo, hi) of rows of the sorted rotations, and K1 leaves the order of those
// rotations in device memory, c->sa[c->sa_res]: the rotations that start with the pattern start at sa[lo .. hi).  No samples, no
// LF walk: one gather.  What the kernels here add is the batch around that identity:
//   range    one lane per pattern, the search of count_kernel (fm_range: both granules of a level issued together, the next
//            byte loaded off the chain); stores lo and hi - lo.
//   scan     exclusive u64 scan of the per-pattern row counts: three launches (sums of 2048-element blocks, one workgroup over
//            those sums -- scan_util.h's carried pass, as in kd_match / kd_lcp / kd_parse.hip -- the blocks again).  Its last word is the batch's row total, read back through a word of the locate's own.
//   gather   one lane per row: its pattern by binary search in the starts (fm_row_pattern), position sa[lo_p + k] -- the rows of
//            one interval are neighbouring words.  Stores (position, pattern id); or, asked to, only counts per pattern the rows
//            whose match runs across the end of the text (fm_linear_hit): at most m - 1 per pattern, so the atomics are few.
//   order    two stable radix_sort_pairs: on the position bits, then on the pattern-id bits (skipped for one pattern).  After
//            them pattern p's rows stand where they stood, ascending.
//   compact  linear mode: the rows that run across the end have the largest positions of their pattern, so the kept ones are
//            the first of its sorted segment: one lane per kept row copies it to its place.
// Everything written is the locate's own (qb::loc_* of c->qbuf) or the caller's two outputs; the sort's histograms are c->rs_hist on the
// context's stream, as the sort hooks use them.  Row indices and totals are u64; a batch of more than 2^31 - 1 rows is sized
// but not gathered (the sort's length is a u32, positions are below 2^31 anyway).
#include "common.h"
#include "fm_step.h"
#include "scan_util.h"

namespace bce {

namespace {

constexpr int LOC_T = 256;                   // lanes per workgroup (4 waves)
constexpr int LOC_ITEMS = 8;                 // scan: elements per lane
constexpr uint32_t LOC_BLOCK = LOC_T * LOC_ITEMS;
constexpr uint32_t LOC_MAXGRID = 8192;       // grid-stride kernels: workgroups at most
constexpr uint64_t LOC_MAXROWS = 0x7FFFFFFFull;

struct Zeros8 { uint32_t v[8]; };

__global__ __launch_bounds__(LOC_T) void locate_range_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                             const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off,
                                                             uint32_t npat, uint32_t *__restrict__ lo_out, uint32_t *__restrict__ cnt_out,
                                                             uint32_t *__restrict__ bad) {
  const uint32_t p = blockIdx.x * LOC_T + threadIdx.x;
  if (p >= npat) return;
  const uint64_t b = off[p], e = off[(size_t)p + 1];
  if (e < b) { *bad = 1u; lo_out[p] = 0; cnt_out[p] = 0; return; }   // (every lane that sees it stores the same word)
  uint32_t lo, hi;
  fm_range(pat + b, e - b, n, z.v, lo, hi, [&](int j, uint32_t ia, uint32_t ib, uint32_t &ra, uint32_t &rb) {
    const Granule *G = gran + (size_t)j * ngran;                     // (64-bit, as count_kernel)
    const uint32_t ga = div96(ia), gb = div96(ib);
    const Granule qa = G[ga], qb = G[gb];                            // both loads go out before either rank
    ra = granule_rank1(qa, ia - ga * 96u);
    rb = granule_rank1(qb, ib - gb * 96u);
  });
  lo_out[p] = lo;
  cnt_out[p] = hi - lo;
}

// element i of the scanned sequence: cnt[i], less drop[i] where there is one
__device__ __forceinline__ uint64_t scan_elem(const uint32_t *cnt, const uint32_t *drop, uint64_t i, uint32_t npat) {
  return i < npat ? (uint64_t)(cnt[i] - (drop ? drop[i] : 0u)) : 0ull;
}

__global__ __launch_bounds__(LOC_T) void locate_scan_sums_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ drop,
                                                                 uint32_t npat, uint64_t *__restrict__ bsum) {
  const uint64_t base = (uint64_t)blockIdx.x * LOC_BLOCK + (uint64_t)threadIdx.x * LOC_ITEMS;
  uint64_t s = 0;
#pragma unroll
  for (int q = 0; q < LOC_ITEMS; ++q) s += scan_elem(cnt, drop, base + q, npat);
  const uint64_t tot = block_reduce_sum64<LOC_T>(s);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one workgroup: bsum[0, nb) -> its exclusive scan, in place; the grand total -> *total and start[npat]
__global__ __launch_bounds__(LOC_T) void locate_scan_top_kernel(uint64_t *__restrict__ bsum, uint32_t nb, uint64_t *__restrict__ start,
                                                                uint32_t npat, uint64_t *__restrict__ total) {
  const uint64_t sum = block_carried_scan_sum64<LOC_T>(bsum, nb);
  if (threadIdx.x == 0) { start[npat] = sum; *total = sum; }
}

__global__ __launch_bounds__(LOC_T) void locate_scan_fill_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ drop,
                                                                 uint32_t npat, const uint64_t *__restrict__ bsum,
                                                                 uint64_t *__restrict__ start) {
  const uint64_t base = (uint64_t)blockIdx.x * LOC_BLOCK + (uint64_t)threadIdx.x * LOC_ITEMS;
  uint64_t v[LOC_ITEMS], s = 0;
#pragma unroll
  for (int q = 0; q < LOC_ITEMS; ++q) { v[q] = scan_elem(cnt, drop, base + q, npat); s += v[q]; }
  uint64_t tot;
  uint64_t run = bsum[blockIdx.x] + block_excl_scan_sum64<LOC_T>(s, &tot);
#pragma unroll
  for (int q = 0; q < LOC_ITEMS; ++q) {
    if (base + q < npat) start[base + q] = run;
    run += v[q];
  }
}

// One lane per row r < rows of the batch.  sa == nullptr: the text of one byte, whose only rotation starts at 0 (K1 keeps no
// array for it).  key != nullptr: (position, pattern) -> key[r], val[r].  drop != nullptr: drop[p] += 1 for every row of p whose
// match does not end inside the text.
__global__ __launch_bounds__(LOC_T) void locate_gather_kernel(const uint32_t *__restrict__ sa, uint32_t n, const uint64_t *__restrict__ off,
                                                              const uint32_t *__restrict__ lo, const uint64_t *__restrict__ start,
                                                              uint32_t npat, uint64_t rows, uint32_t *__restrict__ key,
                                                              uint32_t *__restrict__ val, uint32_t *__restrict__ drop) {
  for (uint64_t r = (uint64_t)blockIdx.x * LOC_T + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * LOC_T) {
    const uint32_t p = fm_row_pattern(start, npat, r);
    const uint64_t row = (uint64_t)lo[p] + (r - start[p]);          // < n: inside pattern p's interval
    const uint32_t pos = sa ? sa[row] : 0u;
    if (key) { key[r] = pos; val[r] = p; }
    if (drop && !fm_linear_hit(pos, off[(size_t)p + 1] - off[p], n)) atomicAdd(&drop[p], 1u);
  }
}

// Linear mode, after the sorts: kept row o < total of pattern p is the (o - lin[p])-th of p's sorted segment, which begins at cyc[p].
__global__ __launch_bounds__(LOC_T) void locate_compact_kernel(const uint32_t *__restrict__ sorted, const uint64_t *__restrict__ cyc,
                                                               const uint64_t *__restrict__ lin, uint32_t npat, uint64_t total,
                                                               uint32_t *__restrict__ out) {
  for (uint64_t o = (uint64_t)blockIdx.x * LOC_T + threadIdx.x; o < total; o += (uint64_t)gridDim.x * LOC_T) {
    const uint32_t p = fm_row_pattern(lin, npat, o);
    out[o] = sorted[cyc[p] + (o - lin[p])];
  }
}

uint32_t stride_grid(uint64_t items) {
  const uint64_t g = (items + LOC_T - 1) / LOC_T;
  return (uint32_t)(g < LOC_MAXGRID ? g : LOC_MAXGRID);
}

}  // namespace

// start[0, npat] = exclusive scan of cnt[i] - drop[i] (drop may be null); *total = its last word, read back through loc_res's
// second word (the caller has made loc_res).  Also kd_near.hip's scan.
int locate_scan(bce_hip_ctx *c, const uint32_t *cnt, const uint32_t *drop, uint32_t npat, uint64_t *start, uint64_t *total) {
  const uint32_t nb = (uint32_t)(((uint64_t)npat + LOC_BLOCK - 1) / LOC_BLOCK);
  BCE_TRY(ensure(c, c->qbuf[qb::loc_bsum], (size_t)nb * 8));
  uint64_t *bsum = c->qbuf[qb::loc_bsum].as<uint64_t>();
  uint64_t *d_total = c->qbuf[qb::loc_res].as<uint64_t>() + 1;
  hipLaunchKernelGGL(locate_scan_sums_kernel, dim3(nb), dim3(LOC_T), 0, c->stream, cnt, drop, npat, bsum);
  hipLaunchKernelGGL(locate_scan_top_kernel, dim3(1), dim3(LOC_T), 0, c->stream, bsum, nb, start, npat, d_total);
  hipLaunchKernelGGL(locate_scan_fill_kernel, dim3(nb), dim3(LOC_T), 0, c->stream, cnt, drop, npat, bsum, start);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(read_back(c, total, d_total, 8));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// First half of a locate: the search, the row counts and the CSR offsets.  d_hits[0, npat] receives the offsets of the hits of
// d_pat[d_off[p], d_off[p + 1]), p < npat, in the text of the context's planes and suffix array (sa: K1's, or null for a text of one
// byte), *total their last word -- exact in both modes -- and *rows the batch's cyclic rows.  All arrays: device memory of the
// context's device.  Queued on the context's stream; complete on return.  Offsets that decrease: BCE_HIP_E_ARG; more than
// 2^31 - 1 rows: BCE_HIP_E_OVERFLOW, with d_hits and *total written.  Leaves what kd_locate_fill needs in the loc_* buffers.
int kd_locate_size(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, bool linear,
                   uint64_t *d_hits, uint64_t *rows, uint64_t *total) {
  const size_t words = (size_t)npat * 4, starts = ((size_t)npat + 1) * 8;
  BCE_TRY(ensure(c, c->qbuf[qb::loc_res], 16));                                // [0] the flag word, [1] a scan's total
  BCE_TRY(ensure(c, c->qbuf[qb::loc_lo], words));
  BCE_TRY(ensure(c, c->qbuf[qb::loc_cnt], words));
  BCE_TRY(ensure(c, c->qbuf[qb::loc_start], starts));
  uint32_t *d_bad = c->qbuf[qb::loc_res].as<uint32_t>();
  uint32_t *lo = c->qbuf[qb::loc_lo].as<uint32_t>(), *cnt = c->qbuf[qb::loc_cnt].as<uint32_t>();
  uint64_t *cyc = c->qbuf[qb::loc_start].as<uint64_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(d_bad, 0, 16, c->stream));
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  const uint32_t grid = (uint32_t)(((uint64_t)npat + LOC_T - 1) / LOC_T);
  hipLaunchKernelGGL(locate_range_kernel, dim3(grid), dim3(LOC_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off,
                     npat, lo, cnt, d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(locate_scan(c, cnt, nullptr, npat, cyc, rows));
  uint32_t bad = 0;
  BCE_TRY(read_back(c, &bad, d_bad, 4));
  if (bad) { snprintf(c->err, sizeof c->err, "locate: pattern offsets decrease"); return BCE_HIP_E_ARG; }
  const uint64_t *hits = cyc;
  *total = *rows;
  if (linear) {                                                      // the exact linear offsets, before anything is gathered
    BCE_TRY(ensure(c, c->qbuf[qb::loc_drop], words));
    BCE_TRY(ensure(c, c->qbuf[qb::loc_lin], starts));
    uint32_t *drop = c->qbuf[qb::loc_drop].as<uint32_t>();
    BCE_HIP_TRY(c, hipMemsetAsync(drop, 0, words, c->stream));
    if (*rows) {
      hipLaunchKernelGGL(locate_gather_kernel, dim3(stride_grid(*rows)), dim3(LOC_T), 0, c->stream, sa, c->n, d_off, lo, cyc, npat, *rows,
                         (uint32_t *)nullptr, (uint32_t *)nullptr, drop);
      BCE_HIP_TRY(c, hipGetLastError());
    }
    hits = c->qbuf[qb::loc_lin].as<uint64_t>();
    BCE_TRY(locate_scan(c, cnt, drop, npat, c->qbuf[qb::loc_lin].as<uint64_t>(), total));
  }
  BCE_HIP_TRY(c, hipMemcpyAsync(d_hits, hits, starts, hipMemcpyDeviceToDevice, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*rows > LOC_MAXROWS) {
    snprintf(c->err, sizeof c->err, "locate: the batch has %llu rows, one call gathers at most 2^31 - 1", (unsigned long long)*rows);
    return BCE_HIP_E_OVERFLOW;
  }
  return BCE_HIP_OK;
}

// Second half, straight after kd_locate_size of the same batch (its rows <= 2^31 - 1 and total): d_pos[0, total) receives the
// positions, each pattern's ascending.  Complete on return.
int kd_locate_fill(bce_hip_ctx *c, const uint32_t *sa, const uint64_t *d_off, uint32_t npat, bool linear, uint64_t rows, uint64_t total,
                   uint32_t *d_pos) {
  if (total == 0) return BCE_HIP_OK;
  const uint32_t nrows = (uint32_t)rows;
  const size_t rbytes = (size_t)nrows * 4;
  for (DevBuf *b : {&c->qbuf[qb::loc_key0], &c->qbuf[qb::loc_key1], &c->qbuf[qb::loc_val0], &c->qbuf[qb::loc_val1]}) BCE_TRY(ensure(c, *b, rbytes));
  uint32_t *key[2] = {c->qbuf[qb::loc_key0].as<uint32_t>(), c->qbuf[qb::loc_key1].as<uint32_t>()};
  uint32_t *val[2] = {c->qbuf[qb::loc_val0].as<uint32_t>(), c->qbuf[qb::loc_val1].as<uint32_t>()};
  const uint64_t *cyc = c->qbuf[qb::loc_start].as<uint64_t>();
  hipLaunchKernelGGL(locate_gather_kernel, dim3(stride_grid(rows)), dim3(LOC_T), 0, c->stream, sa, c->n, d_off, c->qbuf[qb::loc_lo].as<uint32_t>(), cyc,
                     npat, rows, key[0], val[0], (uint32_t *)nullptr);
  BCE_HIP_TRY(c, hipGetLastError());
  int res = 0;
  BCE_TRY(radix_sort_pairs(c, key, val, nrows, 0, ceil_log2(c->n), &res, 9));     // positions ascending
  const uint32_t *sorted = key[res];
  if (npat > 1) {                                                    // stably back into patterns: (pattern id, position) pairs
    uint32_t *k2[2] = {val[res], val[res ^ 1]}, *v2[2] = {key[res], key[res ^ 1]};
    int r2 = 0;
    BCE_TRY(radix_sort_pairs(c, k2, v2, nrows, 0, ceil_log2(npat), &r2, 9));
    sorted = v2[r2];
  }
  if (linear) {
    hipLaunchKernelGGL(locate_compact_kernel, dim3(stride_grid(total)), dim3(LOC_T), 0, c->stream, sorted, cyc, c->qbuf[qb::loc_lin].as<uint64_t>(), npat,
                       total, d_pos);
    BCE_HIP_TRY(c, hipGetLastError());
  } else {
    BCE_HIP_TRY(c, hipMemcpyAsync(d_pos, sorted, rbytes, hipMemcpyDeviceToDevice, c->stream));
  }
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
