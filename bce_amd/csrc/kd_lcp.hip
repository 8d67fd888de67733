// kd_lcp.hip -- what the indexed text holds by itself: the LCP array of its sorted rotations, and the figures that are reductions
// of that array (bce_hip_lcp / _lcp_device, bce_hip_kgrams, bce_hip_longest_repeat, `bce -gk`), and the list of the most frequent
// k-grams (bce_hip_top_kgrams, `bce -gf`).
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
//   top      for one k: the classes' sizes binned by floor(log2), the host's threshold bin (top_step.h), the classes at or above it
//            compacted in row order, sorted stably by size, the first `limit` gathered with their bytes (kd_top_kgrams, below).
// Everything written is the feature's own (qb::rep_* and qb::top_* of c->qbuf) or the caller's output.  sa[sa_res] and the text are only read.
#include "common.h"
#include "bce_cost.h"
#include "lcp_step.h"
#include "scan_util.h"
#include "top_step.h"

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

// ---- the most frequent k-grams: from the reduction of the classes to a list of them ------------------------------------------------
// The class starts are class_max_kernel's and class_top_kernel's; the three passes below run over the blocks again with that carry.
// f(i, size, start) for every class whose last row is the lane's i-th, in row order.  All lanes of the workgroup call it (barriers).
template <class F>
__device__ __forceinline__ void for_class_ends(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t k, const uint32_t *__restrict__ bmax, F &&f) {
  const uint32_t base = blockIdx.x * REP_BLOCK;
  uint32_t w[REP_ITEMS], v[REP_ITEMS], m = 0;
  load_rows(lcp, class_index(base, 0), n, w);
  const uint32_t after = class_index(base, REP_ITEMS);                // the row behind the lane's last
  const uint32_t wnext = after < n ? lcp[after] : 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) { v[i] = class_elem(w[i], class_index(base, i), k); m = m > v[i] ? m : v[i]; }
  uint32_t tot;
  const uint32_t ex = block_excl_scan_max<REP_T>(m, &tot), front = bmax[blockIdx.x];
  uint32_t start = ex > front ? ex : front;                           // (the carry: a class may have started any number of blocks ago)
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) {
    start = start > v[i] ? start : v[i];
    const uint32_t r = class_index(base, i);
    const uint32_t behind = i + 1 < REP_ITEMS ? w[(i + 1) % REP_ITEMS] : wnext;
    if (r < n && (r + 1u == n || behind < k)) f(i, r - start + 1u, start);
  }
}

// bhist[block * 32 + b] = the classes that END in the block and have floor(log2 size) = b.  Every lane leaves the bins of its eight
// rows in LDS (0xFF: no class ends there); then lane t counts bin t % 32 in eighth t / 32 of the block, four rows per word.
__global__ __launch_bounds__(REP_T) void top_hist_kernel(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t k, const uint32_t *__restrict__ bmax,
                                                         uint32_t *__restrict__ bhist) {
  __shared__ uint32_t bins[REP_BLOCK / 4];
  __shared__ uint32_t part[REP_T];
  uint32_t mine[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  for_class_ends(lcp, n, k, bmax, [&](int i, uint32_t size, uint32_t) {
    const uint32_t sh = (uint32_t)(i & 3) * 8u;
    mine[i >> 2] = (mine[i >> 2] & ~(0xFFu << sh)) | (top_bin(size) << sh);
  });
  bins[threadIdx.x * 2] = mine[0];
  bins[threadIdx.x * 2 + 1] = mine[1];
  __syncthreads();
  const uint32_t b = threadIdx.x & 31u, seg = threadIdx.x >> 5, pat = b * 0x01010101u;
  uint32_t cnt = 0;
  for (uint32_t j = 0; j < REP_BLOCK / 32; ++j) {                      // the bytes of y that are 0, exactly: no carry leaves a byte
    const uint32_t y = bins[seg * (REP_BLOCK / 32) + j] ^ pat;
    cnt += (uint32_t)__popc(~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu));
  }
  part[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x < 32) {
    uint32_t s = 0;
#pragma unroll
    for (int g = 0; g < REP_T / 32; ++g) s += part[g * 32 + threadIdx.x];
    bhist[(size_t)blockIdx.x * kTopBins + threadIdx.x] = s;
  }
}

// one workgroup: hist[b] = the sum of the blocks' counters of bin b
__global__ __launch_bounds__(REP_T) void top_hist_sum_kernel(const uint32_t *__restrict__ bhist, uint32_t nb, uint64_t *__restrict__ hist) {
  __shared__ uint64_t part[REP_T];
  uint64_t s = 0;
  for (uint32_t blk = threadIdx.x >> 5; blk < nb; blk += REP_T / 32) s += bhist[(size_t)blk * kTopBins + (threadIdx.x & 31u)];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < 32) {
    uint64_t t = 0;
#pragma unroll
    for (int g = 0; g < REP_T / 32; ++g) t += part[g * 32 + threadIdx.x];
    hist[threadIdx.x] = t;
  }
}

// bcnt[block] = the candidates (classes of size >= 2^t) that end in the block
__global__ __launch_bounds__(REP_T) void top_count_kernel(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t k, const uint32_t *__restrict__ bmax,
                                                          uint32_t t, uint64_t *__restrict__ bcnt) {
  uint32_t mine = 0;
  for_class_ends(lcp, n, k, bmax, [&](int, uint32_t size, uint32_t) { mine += (size >> t) != 0u; });
  mine = block_reduce_sum<REP_T>(mine);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = mine;
}

// one workgroup: bcnt[0, nb) -> the candidates of the blocks in front, in place
__global__ __launch_bounds__(REP_T) void top_offsets_kernel(uint64_t *__restrict__ bcnt, uint32_t nb) {
  (void)block_carried_scan_sum64<REP_T>(bcnt, nb);
}

// the candidates in ROW order: key = key_max - size (ascending keys are descending sizes), value = the class's first row.  m: the
// candidate count the host worked out from the histogram -- what the arrays hold; nothing is stored at or beyond it.
__global__ __launch_bounds__(REP_T) void top_emit_kernel(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t k, const uint32_t *__restrict__ bmax,
                                                         uint32_t t, uint32_t key_max, const uint64_t *__restrict__ boff, uint32_t m,
                                                         uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  uint32_t size[REP_ITEMS], first[REP_ITEMS], mine = 0;
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i) size[i] = 0;
  for_class_ends(lcp, n, k, bmax, [&](int i, uint32_t sz, uint32_t start) {
    if ((sz >> t) != 0u) { size[i] = sz; first[i] = start; mine += 1u; }
  });
  uint32_t tot;
  uint64_t at = boff[blockIdx.x] + block_excl_scan_sum<REP_T>(mine, &tot);
#pragma unroll
  for (int i = 0; i < REP_ITEMS; ++i)
    if (size[i]) {
      if (at < m) { key[at] = key_max - size[i]; val[at] = first[i]; }
      ++at;
    }
}

// entry e < found of the sorted pairs: its count, first row and sa[row] (sa == nullptr: the text of one byte, position 0)
__global__ __launch_bounds__(REP_T) void top_gather_kernel(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t found,
                                                           uint32_t key_max, const uint32_t *__restrict__ sa, bce_hip_top_kgram *__restrict__ out) {
  const uint32_t e = blockIdx.x * REP_T + threadIdx.x;
  if (e >= found) return;
  const uint32_t row = val[e];
  bce_hip_top_kgram g;
  g.count = key_max - key[e]; g.row = row; g.pos = sa ? sa[row] : 0u;
  out[e] = g;
}

// one lane per output byte: bytes[e * k + j] = T[(pos_e + j) mod n], e < found, j < k
__global__ __launch_bounds__(REP_T) void top_bytes_kernel(const uint8_t *__restrict__ text, uint32_t n, const bce_hip_top_kgram *__restrict__ out,
                                                          uint32_t k, uint64_t total, uint8_t *__restrict__ bytes) {
  for (uint64_t i = (uint64_t)blockIdx.x * REP_T + threadIdx.x; i < total; i += (uint64_t)gridDim.x * REP_T) {
    const uint32_t e = (uint32_t)(i / k), j = (uint32_t)(i - (uint64_t)e * k);
    bytes[i] = text[(out[e].pos + j % n) % n];                        // (both terms below n: no wrap of the sum below 2^32)
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

// The first min(limit, distinct) classes of k, by size descending and first row ascending, from an array of n words kd_lcp left
// with a bound >= max(k, 1); d_lcp: 32-byte aligned (rep_lcp).  d_out: room for `limit` entries in device memory; d_bytes: null, or
// room for limit * k bytes there (then `text` is read: the n bytes the rows are rotations of).  *found entries are written.
//   class starts (the reduction's two launches) -> histogram of floor(log2 size), 256 bytes back: the wait -> the threshold bin on
//   the host (top_step.h) -> candidates counted per block, one workgroup for the blocks' offsets, the candidates written in row
//   order -> the stable sort on the key's significant bits (none: nothing launched) -> entries and bytes gathered.
// The candidate arrays are sized by the histogram's exact count, never by n.  The sort's histograms are c->rs_hist on the context's
// stream, as in kd_locate.hip; a model flush that still runs on a stream of its own is waited for first.  Complete on return.
int kd_top_kgrams(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, const uint8_t *text, uint32_t k, uint32_t limit,
                  bce_hip_top_kgram *d_out, uint8_t *d_bytes, uint32_t *found, uint64_t *distinct, uint64_t size_hist[32]) {
  const uint32_t nb = rep_blocks(n);
  BCE_TRY(ensure(c, c->qbuf[qb::top_res], kTopBins * sizeof(uint64_t)));
  BCE_TRY(ensure(c, c->qbuf[qb::top_bsum], (size_t)nb * (8 + 4 + kTopBins * 4)));   // the blocks' candidate counts, class-start maxima, counters
  uint64_t *d_hist = c->qbuf[qb::top_res].as<uint64_t>();
  uint64_t *bcnt = c->qbuf[qb::top_bsum].as<uint64_t>();
  uint32_t *bmax = reinterpret_cast<uint32_t *>(bcnt + nb), *bhist = bmax + nb;
  hipLaunchKernelGGL(class_max_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, k, bmax);
  hipLaunchKernelGGL(class_top_kernel, dim3(1), dim3(REP_T), 0, c->stream, bmax, nb);
  hipLaunchKernelGGL(top_hist_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, k, bmax, bhist);
  hipLaunchKernelGGL(top_hist_sum_kernel, dim3(1), dim3(REP_T), 0, c->stream, bhist, nb, d_hist);
  BCE_HIP_TRY(c, hipGetLastError());
  uint64_t H[kTopBins];
  BCE_TRY(read_back(c, H, d_hist, sizeof H));
  const uint64_t classes = top_classes(H), want = classes < limit ? classes : limit;
  if (classes == 0 || classes > n) { snprintf(c->err, sizeof c->err, "top k-grams: %llu classes in %u rows", (unsigned long long)classes, n); return BCE_HIP_E_INTERNAL; }
  uint64_t cand = 0;
  int top = 0;
  const int t = top_threshold(H, want, &cand, &top);
  const uint32_t m = (uint32_t)cand, key_max = top_key_max(top), bits = top_key_bits(t, top);
  for (qb::Id id : {qb::top_key0, qb::top_key1, qb::top_val0, qb::top_val1}) BCE_TRY(ensure(c, c->qbuf[id], (size_t)m * 4));
  uint32_t *key[2] = {c->qbuf[qb::top_key0].as<uint32_t>(), c->qbuf[qb::top_key1].as<uint32_t>()};
  uint32_t *val[2] = {c->qbuf[qb::top_val0].as<uint32_t>(), c->qbuf[qb::top_val1].as<uint32_t>()};
  hipLaunchKernelGGL(top_count_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, k, bmax, (uint32_t)t, bcnt);
  hipLaunchKernelGGL(top_offsets_kernel, dim3(1), dim3(REP_T), 0, c->stream, bcnt, nb);
  hipLaunchKernelGGL(top_emit_kernel, dim3(nb), dim3(REP_T), 0, c->stream, d_lcp, n, k, bmax, (uint32_t)t, key_max, bcnt, m, key[0], val[0]);
  BCE_HIP_TRY(c, hipGetLastError());
  if (k4_in_flight(c)) BCE_HIP_TRY(c, hipStreamSynchronize(c->k4_stream));
  int res = 0;
  BCE_TRY(radix_sort_pairs(c, key, val, m, 0, bits, &res, 8));
  const uint32_t nfound = (uint32_t)(want < m ? want : m);
  hipLaunchKernelGGL(top_gather_kernel, dim3((nfound + REP_T - 1) / REP_T), dim3(REP_T), 0, c->stream, key[res], val[res], nfound, key_max, sa, d_out);
  const uint64_t total = (uint64_t)nfound * k;
  if (d_bytes && total) {
    const uint64_t gb = (total + REP_T - 1) / REP_T;
    hipLaunchKernelGGL(top_bytes_kernel, dim3((uint32_t)(gb < 65536 ? gb : 65536)), dim3(REP_T), 0, c->stream, text, n, d_out, k, total, d_bytes);
  }
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  *found = nfound;
  if (distinct) *distinct = classes;
  if (size_hist) memcpy(size_hist, H, sizeof H);
  return BCE_HIP_OK;
}

}  // namespace bce
