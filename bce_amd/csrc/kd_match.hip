// kd_match.hip -- the longest matches of a second buffer in the indexed text: its matching statistics against the K2 planes and
// K1's suffix array (bce_hip_match / _match_device, bce_hip_coverage / _coverage_device, `bce -gm`).
//
// For every end position i of the query, len[i] is the length of the longest string that ends at query[i] and occurs in the text
// (at most max_len, a work bound), pos[i] the start of one such occurrence.  Backward search (fm_step.h: fm_match_end) gives
// both with the step the count runs: it starts from the empty match at i and extends to the left until the interval of rows is
// empty -- or, in linear mode, until no row of it lies inside the text.
//   match     one lane per end position.  Per level both granules of lo and hi leave together (count_kernel's fetch), the byte
//             to the left is loaded off the chain.  A lane stops at its first miss; its wave goes on until all its lanes are
//             done.  Linear mode reads suffix-array words only while an interval is narrower than the match is long (fm_step.h).
//             Stores len[i] and, asked to, pos[i] = sa[row] (0xFFFFFFFF where len[i] == 0): plain stores, no LDS, no atomics.
//   coverage  the bytes of the query that lie in a match of min_len bytes or more: j is covered when some i >= j has
//             len[i] >= min_len and i - len[i] + 1 <= j.  A reverse running minimum of s'[i] = i - len[i] + 1 (+inf where the
//             match is too short) over i >= j, then the j with minimum <= j are counted.  Block-wise: maxima of 2048-element
//             blocks (the minimum of s' is the maximum of ~s', and 0 stands for +inf: s' is below 2^31), one workgroup over
//             those maxima from the last block to the first (scan_util.h's carried pass), the blocks again with their carry,
//             one workgroup that adds the blocks' counts into the result word.  No atomics: the count is the same sum every time.
// Everything written is the match's own (qb::mat_* of c->qbuf) or the caller's two outputs.  The planes and sa[sa_res] are only read.
#include "common.h"
#include "fm_step.h"
#include "scan_util.h"

namespace bce {

namespace {

constexpr int MAT_T = 256;                   // lanes per workgroup (4 waves)
constexpr int MAT_ITEMS = 8;                 // coverage: elements per lane
constexpr uint32_t MAT_BLOCK = MAT_T * MAT_ITEMS;

struct Zeros8 { uint32_t v[8]; };

// sa == nullptr: the text of one byte, whose only rotation starts at 0 (fm_match_end never reads an entry for it).
template <bool Linear>
__global__ __launch_bounds__(MAT_T) void match_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                      const uint32_t *__restrict__ sa, const uint8_t *__restrict__ query, uint32_t q,
                                                      uint32_t max_len, uint32_t *__restrict__ len_out, uint32_t *__restrict__ pos_out) {
  const uint32_t i = blockIdx.x * MAT_T + threadIdx.x;
  if (i >= q) return;
  uint32_t len, row;
  fm_match_end<Linear>(
      query, i, max_len, n, z.v, pos_out != nullptr, len, row,
      [&](int j, uint32_t ia, uint32_t ib, uint32_t &ra, uint32_t &rb) {
        const Granule *G = gran + (size_t)j * ngran;                  // (64-bit, as count_kernel)
        const uint32_t ga = div96(ia), gb = div96(ib);
        const Granule qa = G[ga], qb = G[gb];                         // both loads go out before either rank
        ra = granule_rank1(qa, ia - ga * 96u);
        rb = granule_rank1(qb, ib - gb * 96u);
      },
      [&](uint32_t r) { return sa[r]; });
  len_out[i] = len;
  if (pos_out) pos_out[i] = len ? (sa ? sa[row] : 0u) : 0xFFFFFFFFu;
}

// ---- coverage ---------------------------------------------------------------------------------------------------------------------
// element e of the scanned sequence: ~s'[e] where the match that ends at e is long enough, else 0
__device__ __forceinline__ uint32_t cover_elem(const uint32_t *len, uint32_t e, uint32_t q, uint32_t min_len) {
  if (e >= q) return 0u;
  const uint32_t l = len[e];
  return l >= min_len ? ~(e - l + 1u) : 0u;                           // (l <= e + 1: the start is not negative)
}

// Lane t of a workgroup owns the elements base + MAT_BLOCK - 1 - (t * MAT_ITEMS + k), k < MAT_ITEMS: the block from its last
// element to its first, so that a forward scan over the lanes is a running maximum over the elements behind.
__device__ __forceinline__ uint32_t cover_index(uint32_t base, int k) { return base + (MAT_BLOCK - 1u) - (threadIdx.x * MAT_ITEMS + (uint32_t)k); }

__global__ __launch_bounds__(MAT_T) void cover_max_kernel(const uint32_t *__restrict__ len, uint32_t q, uint32_t min_len,
                                                          uint32_t *__restrict__ bmax) {
  const uint32_t base = blockIdx.x * MAT_BLOCK;
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < MAT_ITEMS; ++k) { const uint32_t v = cover_elem(len, cover_index(base, k), q, min_len); m = m > v ? m : v; }
  m = block_reduce_max<MAT_T>(m);
  if (threadIdx.x == 0) bmax[blockIdx.x] = m;
}

// one workgroup: bmax[0, nb) -> for every block the maximum of the blocks behind it, in place
__global__ __launch_bounds__(MAT_T) void cover_top_kernel(uint32_t *__restrict__ bmax, uint32_t nb) {
  block_carried_scan_max<MAT_T, true>(bmax, nb);                      // blocks from the last to the first
}

__global__ __launch_bounds__(MAT_T) void cover_fill_kernel(const uint32_t *__restrict__ len, uint32_t q, uint32_t min_len,
                                                           const uint32_t *__restrict__ bmax, uint32_t *__restrict__ bcnt) {
  const uint32_t base = blockIdx.x * MAT_BLOCK;
  uint32_t v[MAT_ITEMS], m = 0;
#pragma unroll
  for (int k = 0; k < MAT_ITEMS; ++k) { v[k] = cover_elem(len, cover_index(base, k), q, min_len); m = m > v[k] ? m : v[k]; }
  uint32_t tot;
  const uint32_t ex = block_excl_scan_max<MAT_T>(m, &tot), behind = bmax[blockIdx.x];
  uint32_t run = ex > behind ? ex : behind, covered = 0;
#pragma unroll
  for (int k = 0; k < MAT_ITEMS; ++k) {
    run = run > v[k] ? run : v[k];                                    // ~ the smallest start of a long match that ends at or behind j
    const uint32_t j = cover_index(base, k);
    covered += j < q && run != 0u && ~run <= j;
  }
  covered = block_reduce_sum<MAT_T>(covered);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = covered;
}

// one workgroup: *total = the sum of bcnt[0, nb)
__global__ __launch_bounds__(MAT_T) void cover_sum_kernel(const uint32_t *__restrict__ bcnt, uint32_t nb, uint64_t *__restrict__ total) {
  uint64_t s = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += MAT_T) s += bcnt[b];
  s = block_reduce_sum64<MAT_T>(s);
  if (threadIdx.x == 0) *total = s;
}

}  // namespace

// d_len[i] = the length of the longest string that ends at d_query[i] and occurs in the text of the context's planes, at most
// max_len, i < q; d_pos[i] (d_pos may be null) = the start of one occurrence, 0xFFFFFFFF where d_len[i] == 0.  sa: K1's suffix
// array; null for a text of one byte, and where nothing reads it (cyclic, no positions).  All arrays: device memory of the
// context's device.  Queued on the context's stream behind whatever wrote them; the caller waits.
int kd_match(bce_hip_ctx *c, const uint32_t *sa, const uint8_t *d_query, uint32_t q, uint32_t max_len, bool linear, uint32_t *d_len,
             uint32_t *d_pos) {
  if (q == 0) return BCE_HIP_OK;
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  const uint32_t grid = (uint32_t)(((uint64_t)q + MAT_T - 1) / MAT_T);
  if (linear)
    hipLaunchKernelGGL(match_kernel<true>, dim3(grid), dim3(MAT_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, sa, d_query, q,
                       max_len, d_len, d_pos);
  else
    hipLaunchKernelGGL(match_kernel<false>, dim3(grid), dim3(MAT_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, sa, d_query, q,
                       max_len, d_len, d_pos);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// *covered = the j < q for which some i >= j has d_len[i] >= min_len and i - d_len[i] + 1 <= j (d_len: as kd_match left it, any
// max_len >= min_len).  Queued on the context's stream; the result word's way back is the wait.
int kd_coverage(bce_hip_ctx *c, const uint32_t *d_len, uint32_t q, uint32_t min_len, uint64_t *covered) {
  *covered = 0;
  if (q == 0) return BCE_HIP_OK;
  const uint32_t nb = (uint32_t)(((uint64_t)q + MAT_BLOCK - 1) / MAT_BLOCK);
  BCE_TRY(ensure(c, c->qbuf[qb::mat_res], 8));
  BCE_TRY(ensure(c, c->qbuf[qb::mat_bsum], (size_t)nb * 8));                    // the blocks' maxima, then their counts
  uint32_t *bmax = c->qbuf[qb::mat_bsum].as<uint32_t>(), *bcnt = bmax + nb;
  uint64_t *d_total = c->qbuf[qb::mat_res].as<uint64_t>();
  hipLaunchKernelGGL(cover_max_kernel, dim3(nb), dim3(MAT_T), 0, c->stream, d_len, q, min_len, bmax);
  hipLaunchKernelGGL(cover_top_kernel, dim3(1), dim3(MAT_T), 0, c->stream, bmax, nb);
  hipLaunchKernelGGL(cover_fill_kernel, dim3(nb), dim3(MAT_T), 0, c->stream, d_len, q, min_len, bmax, bcnt);
  hipLaunchKernelGGL(cover_sum_kernel, dim3(1), dim3(MAT_T), 0, c->stream, bcnt, nb, d_total);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(read_back(c, covered, d_total, 8));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
