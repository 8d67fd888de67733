// kd_lcp.hip -- what the indexed text holds by itself: the LCP array of its sorted rotations, and the figures that are reductions
// of that array (bce_hip_lcp / _lcp_device, bce_hip_kgrams, bce_hip_longest_repeat, `bce -gk`).
//
// Everything is about the CIRCULAR text, as the coder and bce_hip_count's cyclic mode see it.  lcp[0] = 0, and for 1 <= r < n
// lcp[r] = the bytes on which the rotations sa[r - 1] and sa[r] agree, at most max_len (lcp_step.h: rot_lcp).  There is no cap at
// n, so rows tied to max_len bytes all carry max_len among themselves, whatever order K1 left them in: the capped array is a
// function of the text alone.
//   lcp      one lane per row: two suffix-array words, then rot_lcp on the text.  Plain stores, no LDS, no atomics.
//   classes  for one k: the maximal runs of rows [s, e) with lcp[r] >= k inside are the distinct cyclic k-grams, e - s = N(w).
//            A running maximum of "r where lcp[r] < k, or r = 0" gives every row its class start; the last row of a class (the
//            text's last row, or lcp[r + 1] < k) adds the class to every figure.  Block-wise: maxima of 2048-element blocks,
//            one workgroup that passes the carry from block to block (scan_util.h's carried pass), the blocks again
//            with their carry, one workgroup that adds the blocks' figures into the record.  No atomics: every sum is a uint64_t
//            sum of the same terms, every maximum has one winner.  A class may span any number of blocks.
//   longest  block maxima of (lcp[r], ~r), then one workgroup, which also fetches sa[r - 1] and sa[r].
// Everything written is the feature's own (qb::rep_* of c->qbuf) or the caller's output.  sa[sa_res] and the text are only read.
#include "common.h"
#include "bce_cost.h"
#include "lcp_step.h"
#include "scan_util.h"

namespace bce {

namespace {

constexpr int REP_T = 256;                   // lanes per workgroup (4 waves)
constexpr int REP_ITEMS = 8;                 // reductions: elements per lane
constexpr uint32_t REP_BLOCK = REP_T * REP_ITEMS;

// what one block adds to a k's record
struct ClassPart { uint32_t distinct, once; uint64_t nlogn, top; };   // top = (size << 32) | ~start of its largest class, lowest start first

// sa == nullptr: the text of one byte, whose only row is row 0
__global__ __launch_bounds__(REP_T) void lcp_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa, uint32_t n,
                                                    uint32_t max_len, uint32_t *__restrict__ lcp) {
  const uint32_t r = blockIdx.x * REP_T + threadIdx.x;
  if (r >= n) return;
  lcp[r] = r ? rot_lcp(text, n, sa[r - 1u], sa[r], max_len) : 0u;
}

// ---- the classes of one k -----------------------------------------------------------------------------------------------------------
// Lane t of a workgroup owns the elements base + t * REP_ITEMS + i, i < REP_ITEMS.
__device__ __forceinline__ uint32_t class_index(uint32_t base, int i) { return base + threadIdx.x * REP_ITEMS + (uint32_t)i; }
// w[i] = lcp[first + i], i < REP_ITEMS, as two 16-byte loads where all eight rows exist (first is a multiple of REP_ITEMS and the
// array a device allocation of its own, c->qbuf[qb::rep_lcp]: 32-byte aligned words); rows at or beyond n read as 0xFFFFFFFF.
__device__ __forceinline__ void load_rows(const uint32_t *__restrict__ lcp, uint32_t first, uint32_t n, uint32_t (&w)[REP_ITEMS]) {
  if (n - first >= (uint32_t)REP_ITEMS && first < n) {
    const uint4 a = *reinterpret_cast<const uint4 *>(lcp + first), b = *reinterpret_cast<const uint4 *>(lcp + first + 4);
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < REP_ITEMS; ++i) w[i] = first + (uint32_t)i < n ? lcp[first + (uint32_t)i] : 0xFFFFFFFFu;
  }
}
// element r of the scanned sequence: r where a class starts at row r, else 0 (row 0 always starts one, and 0 is the identity);
// w = lcp[r], 0xFFFFFFFF beyond the text
__device__ __forceinline__ uint32_t class_elem(uint32_t w, uint32_t r, uint32_t k) { return w < k ? r : 0u; }

__global__ __launch_bounds__(REP_T) void class_max_kernel(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t k, uint32_t *__restrict__ bmax) {
  const uint32_t base = blockIdx.x * REP_BLOCK;
  uint32_t w[REP_ITEMS], m = 0;
  load_rows(lcp, class_index(base, 0), n, w);
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) { const uint32_t v = class_elem(w[i], class_index(base, i), k); m = m > v ? m : v; }
  m = block_reduce_max<REP_T>(m);
  if (threadIdx.x == 0) bmax[blockIdx.x] = m;
}

// one workgroup: bmax[0, nb) -> for every block the maximum of the blocks in front of it, in place
__global__ __launch_bounds__(REP_T) void class_top_kernel(uint32_t *__restrict__ bmax, uint32_t nb) {
  block_carried_scan_max<REP_T, false>(bmax, nb);
}

__global__ __launch_bounds__(REP_T) void class_fill_kernel(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t k,
                                                           const uint32_t *__restrict__ bmax, ClassPart *__restrict__ part) {
  __shared__ uint32_t tab[kLog2Steps + 1];
  for (uint32_t i = threadIdx.x; i <= kLog2Steps; i += REP_T) tab[i] = kLog2TableDev.t[i];
  const uint32_t base = blockIdx.x * REP_BLOCK;
  uint32_t w[REP_ITEMS], v[REP_ITEMS], m = 0;
  load_rows(lcp, class_index(base, 0), n, w);
  const uint32_t after = class_index(base, REP_ITEMS);                // the row behind the lane's last
  const uint32_t wnext = after < n ? lcp[after] : 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) { v[i] = class_elem(w[i], class_index(base, i), k); m = m > v[i] ? m : v[i]; }
  uint32_t tot;
  const uint32_t ex = block_excl_scan_max<REP_T>(m, &tot), front = bmax[blockIdx.x];   // (its barriers also publish tab)
  uint32_t start = ex > front ? ex : front, distinct = 0, once = 0;
  uint64_t nlogn = 0, top = 0;
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) {
    start = start > v[i] ? start : v[i];                              // the first row of r's class
    const uint32_t r = class_index(base, i);
    const uint32_t behind = i + 1 < REP_ITEMS ? w[(i + 1) % REP_ITEMS] : wnext;   // lcp[r + 1]
    if (r < n && (r + 1u == n || behind < k)) {                       // r is the last row of its class
      const uint32_t size = r - start + 1u;
      distinct += 1u;
      once += size == 1u;
      nlogn += (uint64_t)size * log2_q24_with(tab, size);
      const uint64_t key = ((uint64_t)size << 32) | (uint32_t)~start;
      top = top > key ? top : key;
    }
  }
  distinct = block_reduce_sum<REP_T>(distinct);
  once = block_reduce_sum<REP_T>(once);
  nlogn = block_reduce_sum64<REP_T>(nlogn);
  top = block_reduce_max64<REP_T>(top);
  if (threadIdx.x == 0) part[blockIdx.x] = ClassPart{distinct, once, nlogn, top};
}

// one workgroup: *out = the record of the parts [0, nb); the position of the largest class's first row is fetched here
__global__ __launch_bounds__(REP_T) void class_sum_kernel(const ClassPart *__restrict__ part, uint32_t nb, const uint32_t *__restrict__ sa,
                                                          bce_hip_kgram *__restrict__ out) {
  uint64_t distinct = 0, once = 0, nlogn = 0, top = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += REP_T) {
    const ClassPart p = part[b];
    distinct += p.distinct; once += p.once; nlogn += p.nlogn;
    top = top > p.top ? top : p.top;
  }
  distinct = block_reduce_sum64<REP_T>(distinct);
  once = block_reduce_sum64<REP_T>(once);
  nlogn = block_reduce_sum64<REP_T>(nlogn);
  top = block_reduce_max64<REP_T>(top);
  if (threadIdx.x == 0) {
    const uint32_t start = ~(uint32_t)top;
    bce_hip_kgram g;
    g.distinct = distinct; g.once = once; g.nlogn_q24 = nlogn;
    g.max_count = (uint32_t)(top >> 32);
    g.max_pos = sa ? sa[start] : 0u;
    *out = g;
  }
}

// ---- the longest repeat -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(REP_T) void repeat_max_kernel(const uint32_t *__restrict__ lcp, uint32_t n, uint64_t *__restrict__ bkey) {
  const uint32_t base = blockIdx.x * REP_BLOCK;
  uint32_t w[REP_ITEMS];
  load_rows(lcp, class_index(base, 0), n, w);
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) {
    const uint32_t r = class_index(base, i);
    const uint64_t key = r < n ? ((uint64_t)w[i] << 32) | (uint32_t)~r : 0u;
    m = m > key ? m : key;
  }
  m = block_reduce_max64<REP_T>(m);
  if (threadIdx.x == 0) bkey[blockIdx.x] = m;
}

// one workgroup: out[0] = the largest lcp, out[1], out[2] = sa[r - 1], sa[r] of the lowest row r that reaches it.  The largest is 0
// exactly when row 0 wins (no two rotations share a byte, or the text has one byte): then there is no pair, both are 0xFFFFFFFF.
__global__ __launch_bounds__(REP_T) void repeat_top_kernel(const uint64_t *__restrict__ bkey, uint32_t nb, const uint32_t *__restrict__ sa,
                                                           uint32_t *__restrict__ out) {
  uint64_t m = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += REP_T) m = m > bkey[b] ? m : bkey[b];
  m = block_reduce_max64<REP_T>(m);
  if (threadIdx.x == 0) {
    const uint32_t r = ~(uint32_t)m;
    out[0] = (uint32_t)(m >> 32);
    out[1] = r ? sa[r - 1u] : 0xFFFFFFFFu;
    out[2] = r ? sa[r] : 0xFFFFFFFFu;
  }
}

uint32_t rep_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + REP_BLOCK - 1) / REP_BLOCK); }

}  // namespace

// d_lcp[r], r < n: the LCP array of the context's sorted rotations, capped at max_len.  sa: K1's suffix array, null for a text of
// one byte.  Queued on the context's stream; the caller waits.
int kd_lcp(bce_hip_ctx *c, const uint32_t *sa, uint32_t max_len, uint32_t *d_lcp) {
  const uint32_t grid = (uint32_t)(((uint64_t)c->n + REP_T - 1) / REP_T);
  hipLaunchKernelGGL(lcp_kernel, dim3(grid), dim3(REP_T), 0, c->stream, c->text.as<uint8_t>(), sa, c->n, max_len, d_lcp);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// out[i] = the record of ks[i], i < nk <= 64, from an array of n words kd_lcp left with a bound >= every ks[i]; d_lcp: 32-byte aligned (rep_lcp).  One set of launches per k,
// queued on the context's stream; the records' way back is the wait.
int kd_kgrams(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, const uint32_t *ks, uint32_t nk, bce_hip_kgram *out) {
  const uint32_t nb = rep_blocks(n);
  BCE_TRY(ensure(c, c->qbuf[qb::rep_res], 64 * sizeof(bce_hip_kgram)));
  BCE_TRY(ensure(c, c->qbuf[qb::rep_bsum], (size_t)nb * (sizeof(ClassPart) + 4)));   // the blocks' parts, then their maxima
  ClassPart *part = c->qbuf[qb::rep_bsum].as<ClassPart>();
  uint32_t *bmax = reinterpret_cast<uint32_t *>(part + nb);
  bce_hip_kgram *d_out = c->qbuf[qb::rep_res].as<bce_hip_kgram>();
  for (uint32_t i = 0; i < nk; ++i) {
    hipLaunchKernelGGL(class_max_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, ks[i], bmax);
    hipLaunchKernelGGL(class_top_kernel, dim3(1), dim3(REP_T), 0, c->stream, bmax, nb);
    hipLaunchKernelGGL(class_fill_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, ks[i], bmax, part);
    hipLaunchKernelGGL(class_sum_kernel, dim3(1), dim3(REP_T), 0, c->stream, part, nb, sa, d_out + i);
    BCE_HIP_TRY(c, hipGetLastError());
  }
  BCE_TRY(read_back(c, out, d_out, (size_t)nk * sizeof(bce_hip_kgram)));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// res[0] = the largest d_lcp[r], r < n, res[1], res[2] = sa[r - 1], sa[r] of the lowest such r (0xFFFFFFFF twice where the largest is 0).
int kd_longest_repeat(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, uint32_t res[3]) {
  const uint32_t nb = rep_blocks(n);
  BCE_TRY(ensure(c, c->qbuf[qb::rep_res], 64 * sizeof(bce_hip_kgram)));
  BCE_TRY(ensure(c, c->qbuf[qb::rep_bsum], (size_t)nb * 8));
  uint64_t *bkey = c->qbuf[qb::rep_bsum].as<uint64_t>();
  uint32_t *d_out = c->qbuf[qb::rep_res].as<uint32_t>();
  hipLaunchKernelGGL(repeat_max_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, bkey);
  hipLaunchKernelGGL(repeat_top_kernel, dim3(1), dim3(REP_T), 0, c->stream, bkey, nb, sa, d_out);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(read_back(c, res, d_out, 12));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
