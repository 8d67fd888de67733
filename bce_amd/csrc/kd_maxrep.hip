// kd_maxrep.hip -- which strings the indexed text repeats: the list of its maximal repeats, heaviest first (bce_hip_maximal_repeats /
// _maximal_repeats_device, the hook bce_hip_maxrep_of_arrays_device, `bce -gp`, `bce -gpd`), and the number of runs of its BWT.
//
// The rule is maxrep_step.h's: every LCP interval [p, q) of the capped LCP array is named by ONE of its rows, the lowest that carries
// the interval's value l; the row finds p and q in the two-storey min-trees of kd_self.hip (lpf_step.h's searches, unchanged), tests
// left-maximality on a prefix count of the BWT's changes and works out the weight the list is ordered by.
//   change   one workgroup per block of 2048 rows: bw[r] != bw[r - 1] from sa and the text (or from bytes of the caller's), the
//            count up to every row inside the block and the block's count; one workgroup carries the blocks' counts (scan_util.h's
//            carried pass; the grand total is bwt_runs - 1); the blocks again add their carry: D[r], one word per row.
//   trees    nsv_trees over the LCP array, as it is.
//   solve    one workgroup per block, its tree in LDS, one lane per row: mxr_row.  wt[r] = the weight of the repeat row r represents,
//            or 0; first[r] = that interval's first row.  At most 2 log2(NB) + 11 dependent global loads per search.
//   hist     floor(log2 wt) binned per block, 64 bins, and the repeats at the bound; one workgroup sums the blocks.  528 bytes back:
//            the one wait before the emit.
//   select   the host's threshold bin (maxrep_step.h), candidates counted per block, one workgroup for their offsets, the candidates
//            written in ROW order at exact offsets as (complement of the weight, row); radix_sort_wide on the significant bits --
//            stable, so equal weights keep row order; the first `found` gathered, then one lane per output byte.
// Per row: 4 bytes of D, 8 of wt, 4 of first (16), beside the LCP array (4) and the blocks' trees (4).  The candidate arrays are
// sized by the histogram's exact count.  No atomics: every value is written by the one lane that owns it.  Everything written is
// the feature's own (qb::mxr_*), rep_lcp's reader's trees (slf_tree, slf_top) or the caller's output; sa and the text are only read.
#include "common.h"
#include "maxrep_step.h"
#include "scan_util.h"

namespace bce {

namespace {

constexpr int MXR_T = 256;                   // lanes per workgroup (4 waves)
constexpr int MXR_ITEMS = 8;                 // rows per lane
constexpr uint32_t MXR_BLOCK = MXR_T * MXR_ITEMS;
static_assert(MXR_BLOCK == NSV_TREE_BLOCK, "the solve runs on nsv_trees' blocks");
constexpr uint32_t MXR_CNT = kMxrBins + 1;   // counters per block: the bins, then the repeats at the bound

inline uint32_t mxr_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + MXR_BLOCK - 1) / MXR_BLOCK); }

// the byte in front of row r's rotation
__device__ __forceinline__ uint8_t mxr_bw(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa, const uint8_t *__restrict__ bw,
                                          uint32_t n, uint32_t r) {
  if (bw) return bw[r];
  const uint32_t i = sa[r];
  return text[i ? i - 1u : n - 1u];
}

// Lane t owns the rows base + t * MXR_ITEMS + i.  D[r] = the changes among the block's rows up to r; bsum[block] = the block's changes.
__global__ __launch_bounds__(MXR_T) void mxr_change_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa,
                                                           const uint8_t *__restrict__ bw, uint32_t n, uint32_t *__restrict__ D,
                                                           uint64_t *__restrict__ bsum) {
  const uint32_t first = blockIdx.x * MXR_BLOCK + threadIdx.x * MXR_ITEMS;
  uint32_t loc[MXR_ITEMS], cnt = 0;
  uint8_t prev = first > 0u && first <= n ? mxr_bw(text, sa, bw, n, first - 1u) : (uint8_t)0;
#pragma unroll
  for (int i = 0; i < MXR_ITEMS; ++i) {
    const uint32_t r = first + (uint32_t)i;
    if (r < n) {
      const uint8_t cur = mxr_bw(text, sa, bw, n, r);
      cnt += r > 0u && cur != prev;
      prev = cur;
    }
    loc[i] = cnt;
  }
  uint32_t tot;
  const uint32_t ex = block_excl_scan_sum<MXR_T>(cnt, &tot);
#pragma unroll
  for (int i = 0; i < MXR_ITEMS; ++i) {
    const uint32_t r = first + (uint32_t)i;
    if (r < n) D[r] = ex + loc[i];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one workgroup: a[0, nb) -> the sum of the words in front, in place; *total = the sum of all
__global__ __launch_bounds__(MXR_T) void mxr_offsets_kernel(uint64_t *__restrict__ a, uint32_t nb, uint64_t *__restrict__ total) {
  const uint64_t sum = block_carried_scan_sum64<MXR_T>(a, nb);
  if (total && threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(MXR_T) void mxr_carry_kernel(uint32_t *__restrict__ D, uint32_t n, const uint64_t *__restrict__ boff) {
  const uint32_t base = blockIdx.x * MXR_BLOCK, add = (uint32_t)boff[blockIdx.x];
#pragma unroll
  for (int k = 0; k < MXR_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * MXR_T + threadIdx.x;
    if (i < n - base) D[base + i] += add;
  }
}

// the block's tree into LDS, as nsv_solve_kernel; one lane per row
__global__ __launch_bounds__(MXR_T) void mxr_solve_kernel(const uint32_t *__restrict__ vals, uint32_t n, const uint32_t *__restrict__ inner,
                                                          const uint32_t *__restrict__ top, uint32_t NB, const uint32_t *__restrict__ D,
                                                          uint32_t min_len, uint32_t order, uint64_t *__restrict__ wt,
                                                          uint32_t *__restrict__ first) {
  __shared__ uint32_t t[2 * MXR_BLOCK];
  const uint32_t base = blockIdx.x * MXR_BLOCK;
#pragma unroll
  for (int k = 0; k < MXR_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * MXR_T + threadIdx.x;
    t[i] = inner[base + i];
    t[MXR_BLOCK + i] = i < n - base ? vals[base + i] : NSV_PAD;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < MXR_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * MXR_T + threadIdx.x;
    if (i >= n - base) break;                                         // (the rows of a lane ascend)
    uint32_t p = 0;
    const uint64_t w = mxr_row(t, MXR_BLOCK, i, blockIdx.x, top, NB, inner, vals, n, D, min_len, order, &p);
    wt[base + i] = w;
    if (w) first[base + i] = p;
  }
}

// bhist[block * MXR_CNT + b] = the block's repeats with floor(log2 weight) = b; [.. + 64] = those of them at the bound.  Every row
// leaves its bin as a byte in LDS (0xFF: no repeat); then lane t counts bin t % 64 in quarter t / 64 of the block, four rows per word.
__global__ __launch_bounds__(MXR_T) void mxr_hist_kernel(const uint64_t *__restrict__ wt, const uint32_t *__restrict__ vals, uint32_t n,
                                                         uint32_t max_len, uint32_t *__restrict__ bhist) {
  __shared__ uint32_t bins[MXR_BLOCK / 4];
  __shared__ uint32_t part[MXR_T];
  uint8_t *bin8 = reinterpret_cast<uint8_t *>(bins);
  const uint32_t base = blockIdx.x * MXR_BLOCK;
  uint32_t capped = 0;
#pragma unroll
  for (int k = 0; k < MXR_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * MXR_T + threadIdx.x;
    const uint64_t w = i < n - base ? wt[base + i] : 0ull;
    bin8[i] = w ? (uint8_t)mxr_bin(w) : (uint8_t)0xFF;
    if (w) capped += vals[base + i] == max_len;
  }
  capped = block_reduce_sum<MXR_T>(capped);                            // (its barriers also publish the bins)
  const uint32_t b = threadIdx.x & 63u, seg = threadIdx.x >> 6, pat = b * 0x01010101u;
  uint32_t cnt = 0;
  for (uint32_t j = 0; j < MXR_BLOCK / 16; ++j) {                      // the bytes of y that are 0, exactly: no carry leaves a byte
    const uint32_t y = bins[seg * (MXR_BLOCK / 16) + j] ^ pat;
    cnt += (uint32_t)__popc(~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu));
  }
  part[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x < 64) {
    uint32_t s = 0;
#pragma unroll
    for (int g = 0; g < MXR_T / 64; ++g) s += part[g * 64 + threadIdx.x];
    bhist[(size_t)blockIdx.x * MXR_CNT + threadIdx.x] = s;
  }
  if (threadIdx.x == 0) bhist[(size_t)blockIdx.x * MXR_CNT + kMxrBins] = capped;
}

// one workgroup: res[b] = the sum of the blocks' counters b, b <= 64
__global__ __launch_bounds__(MXR_T) void mxr_hist_sum_kernel(const uint32_t *__restrict__ bhist, uint32_t nb, uint64_t *__restrict__ res) {
  __shared__ uint64_t part[MXR_T];
  uint64_t s = 0, capped = 0;
  for (uint32_t blk = threadIdx.x >> 6; blk < nb; blk += MXR_T / 64) s += bhist[(size_t)blk * MXR_CNT + (threadIdx.x & 63u)];
  for (uint32_t blk = threadIdx.x; blk < nb; blk += MXR_T) capped += bhist[(size_t)blk * MXR_CNT + kMxrBins];
  part[threadIdx.x] = s;
  capped = block_reduce_sum64<MXR_T>(capped);                          // (its barriers also publish the parts)
  if (threadIdx.x < 64) {
    uint64_t t = 0;
#pragma unroll
    for (int g = 0; g < MXR_T / 64; ++g) t += part[g * 64 + threadIdx.x];
    res[threadIdx.x] = t;
  }
  if (threadIdx.x == 0) res[kMxrBins] = capped;
}

// Lane t owns the rows base + t * MXR_ITEMS + i, so that a block's candidates come out in row order.
__device__ __forceinline__ void mxr_load_weights(const uint64_t *__restrict__ wt, uint32_t n, uint32_t first, uint64_t (&w)[MXR_ITEMS]) {
#pragma unroll
  for (int i = 0; i < MXR_ITEMS; ++i) w[i] = first + (uint32_t)i < n ? wt[first + (uint32_t)i] : 0ull;
}

// bcnt[block] = the block's candidates (weights of 2^t or more)
__global__ __launch_bounds__(MXR_T) void mxr_count_kernel(const uint64_t *__restrict__ wt, uint32_t n, uint32_t t, uint64_t *__restrict__ bcnt) {
  uint64_t w[MXR_ITEMS];
  mxr_load_weights(wt, n, blockIdx.x * MXR_BLOCK + threadIdx.x * MXR_ITEMS, w);
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < MXR_ITEMS; ++i) mine += (w[i] >> t) != 0ull;
  mine = block_reduce_sum<MXR_T>(mine);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = mine;
}

// the candidates in ROW order: key = key_max - weight in two words, value = the row.  m: the candidate count the host worked out from
// the histogram -- what the arrays hold; nothing is stored at or beyond it.
__global__ __launch_bounds__(MXR_T) void mxr_emit_kernel(const uint64_t *__restrict__ wt, uint32_t n, uint32_t t, uint64_t key_max,
                                                         const uint64_t *__restrict__ boff, uint32_t m, uint32_t *__restrict__ lo,
                                                         uint32_t *__restrict__ hi, uint32_t *__restrict__ val) {
  const uint32_t first = blockIdx.x * MXR_BLOCK + threadIdx.x * MXR_ITEMS;
  uint64_t w[MXR_ITEMS];
  mxr_load_weights(wt, n, first, w);
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < MXR_ITEMS; ++i) mine += (w[i] >> t) != 0ull;
  uint32_t tot;
  uint64_t at = boff[blockIdx.x] + block_excl_scan_sum<MXR_T>(mine, &tot);
#pragma unroll
  for (int i = 0; i < MXR_ITEMS; ++i)
    if ((w[i] >> t) != 0ull) {
      if (at < m) {
        const uint64_t key = key_max - w[i];
        lo[at] = (uint32_t)key; hi[at] = (uint32_t)(key >> 32); val[at] = first + (uint32_t)i;
      }
      ++at;
    }
}

// entry e < found of the sorted candidates
__global__ __launch_bounds__(MXR_T) void mxr_gather_kernel(const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                           const uint32_t *__restrict__ val, uint32_t found, uint64_t key_max, uint32_t order,
                                                           const uint32_t *__restrict__ vals, const uint32_t *__restrict__ first,
                                                           const uint32_t *__restrict__ sa, bce_hip_maxrep *__restrict__ out) {
  const uint32_t e = blockIdx.x * MXR_T + threadIdx.x;
  if (e >= found) return;
  const uint32_t r = val[e], len = vals[r], p = first[r];
  const uint64_t w = key_max - (((uint64_t)hi[e] << 32) | lo[e]);
  bce_hip_maxrep g;
  g.len = len; g.count = mxr_count_of(order, w, len); g.row = p; g.pos = sa[p];
  out[e] = g;
}

// one lane per output byte: bytes[e * per + j] = T[(pos_e + j) mod n] for j < min(len_e, per), else 0
__global__ __launch_bounds__(MXR_T) void mxr_bytes_kernel(const uint8_t *__restrict__ text, uint32_t n, const bce_hip_maxrep *__restrict__ out,
                                                          uint32_t per, uint64_t total, uint8_t *__restrict__ bytes) {
  for (uint64_t i = (uint64_t)blockIdx.x * MXR_T + threadIdx.x; i < total; i += (uint64_t)gridDim.x * MXR_T) {
    const uint32_t e = (uint32_t)(i / per), j = (uint32_t)(i - (uint64_t)e * per);
    const bce_hip_maxrep g = out[e];
    bytes[i] = j < g.len ? text[(g.pos + j % n) % n] : (uint8_t)0;      // (both terms below n: no wrap of the sum below 2^32)
  }
}

}  // namespace

int kd_maxrep(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_lcp, uint32_t n, const uint8_t *text, const uint8_t *bw, uint32_t min_len,
              uint32_t max_len, uint32_t order, uint32_t limit, bce_hip_maxrep *d_out, uint8_t *d_bytes, uint32_t bytes_per, bce_hip_maxrep_info *info) {
  bce_hip_maxrep_info got = {0, 0, 1, 0, 0};
  if (n < 2) { *info = got; return BCE_HIP_OK; }                       // one rotation: no interval, one run
  const uint32_t nb = mxr_blocks(n);
  BCE_TRY(ensure(c, c->qbuf[qb::mxr_res], (MXR_CNT + 1) * sizeof(uint64_t)));
  BCE_TRY(ensure(c, c->qbuf[qb::mxr_bsum], (size_t)nb * (8 + MXR_CNT * 4)));
  BCE_TRY(ensure(c, c->qbuf[qb::mxr_chg], (size_t)n * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::mxr_wt], (size_t)n * 8));
  BCE_TRY(ensure(c, c->qbuf[qb::mxr_first], (size_t)n * 4));
  uint64_t *d_res = c->qbuf[qb::mxr_res].as<uint64_t>(), *bsum = c->qbuf[qb::mxr_bsum].as<uint64_t>(), *wt = c->qbuf[qb::mxr_wt].as<uint64_t>();
  uint32_t *bhist = reinterpret_cast<uint32_t *>(bsum + nb), *D = c->qbuf[qb::mxr_chg].as<uint32_t>(), *first = c->qbuf[qb::mxr_first].as<uint32_t>();
  const dim3 grid(nb), wg(MXR_T);
  hipLaunchKernelGGL(mxr_change_kernel, grid, wg, 0, c->stream, text, sa, bw, n, D, bsum);
  hipLaunchKernelGGL(mxr_offsets_kernel, dim3(1), wg, 0, c->stream, bsum, nb, d_res + MXR_CNT);
  hipLaunchKernelGGL(mxr_carry_kernel, grid, wg, 0, c->stream, D, n, bsum);
  BCE_HIP_TRY(c, hipGetLastError());
  uint32_t NB = 0;
  BCE_TRY(nsv_trees(c, d_lcp, n, &NB));
  hipLaunchKernelGGL(mxr_solve_kernel, grid, wg, 0, c->stream, d_lcp, n, c->qbuf[qb::slf_tree].as<uint32_t>(), c->qbuf[qb::slf_top].as<uint32_t>(), NB,
                     D, min_len, order, wt, first);
  hipLaunchKernelGGL(mxr_hist_kernel, grid, wg, 0, c->stream, wt, d_lcp, n, max_len, bhist);
  hipLaunchKernelGGL(mxr_hist_sum_kernel, dim3(1), wg, 0, c->stream, bhist, nb, d_res);
  BCE_HIP_TRY(c, hipGetLastError());
  uint64_t R[MXR_CNT + 1];
  BCE_TRY(read_back(c, R, d_res, sizeof R));
  got.total = mxr_total(R);
  got.capped = R[kMxrBins];
  got.bwt_runs = R[MXR_CNT] + 1u;
  if (got.total > n || got.capped > got.total || R[MXR_CNT] >= n) {
    snprintf(c->err, sizeof c->err, "maximal repeats: %llu repeats, %llu BWT changes in %u rows", (unsigned long long)got.total, (unsigned long long)R[MXR_CNT], n);
    return BCE_HIP_E_INTERNAL;
  }
  if (got.total == 0) { *info = got; return BCE_HIP_OK; }
  const uint64_t want = got.total < limit ? got.total : limit;
  uint64_t cand = 0;
  int top = 0;
  const int t = mxr_threshold(R, want, &cand, &top);
  const uint32_t m = (uint32_t)cand, bits = mxr_key_bits(t, top);
  const uint64_t key_max = mxr_key_max(top);
  if (getenv("BCE_MAXREP_TRACE"))                                      // (tools/maxrep_rate.py reads it: what the threshold lets through)
    fprintf(stderr, "maxrep: total %llu want %llu threshold_bin %d top_bin %d candidates %u key_bits %u\n", (unsigned long long)got.total,
            (unsigned long long)want, t, top, m, bits);
  for (qb::Id id : {qb::mxr_lo0, qb::mxr_lo1, qb::mxr_hi0, qb::mxr_hi1, qb::mxr_val0, qb::mxr_val1}) BCE_TRY(ensure(c, c->qbuf[id], (size_t)m * 4));
  uint32_t *lo[2] = {c->qbuf[qb::mxr_lo0].as<uint32_t>(), c->qbuf[qb::mxr_lo1].as<uint32_t>()};
  uint32_t *hi[2] = {c->qbuf[qb::mxr_hi0].as<uint32_t>(), c->qbuf[qb::mxr_hi1].as<uint32_t>()};
  uint32_t *val[2] = {c->qbuf[qb::mxr_val0].as<uint32_t>(), c->qbuf[qb::mxr_val1].as<uint32_t>()};
  hipLaunchKernelGGL(mxr_count_kernel, grid, wg, 0, c->stream, wt, n, (uint32_t)t, bsum);
  hipLaunchKernelGGL(mxr_offsets_kernel, dim3(1), wg, 0, c->stream, bsum, nb, (uint64_t *)nullptr);
  hipLaunchKernelGGL(mxr_emit_kernel, grid, wg, 0, c->stream, wt, n, (uint32_t)t, key_max, bsum, m, lo[0], hi[0], val[0]);
  BCE_HIP_TRY(c, hipGetLastError());
  if (k4_in_flight(c)) BCE_HIP_TRY(c, hipStreamSynchronize(c->k4_stream));
  int res = 0;
  BCE_TRY(radix_sort_wide(c, lo, hi, val, m, 0, bits, &res, 8));
  const uint32_t nfound = (uint32_t)(want < m ? want : m);
  hipLaunchKernelGGL(mxr_gather_kernel, dim3((nfound + MXR_T - 1) / MXR_T), wg, 0, c->stream, lo[res], hi[res], val[res], nfound, key_max, order, d_lcp,
                     first, sa, d_out);
  const uint64_t total = (uint64_t)nfound * bytes_per;
  if (d_bytes && total) {
    const uint64_t gb = (total + MXR_T - 1) / MXR_T;
    hipLaunchKernelGGL(mxr_bytes_kernel, dim3((uint32_t)(gb < 65536 ? gb : 65536)), wg, 0, c->stream, text, n, d_out, bytes_per, total, d_bytes);
  }
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  got.found = nfound;
  *info = got;
  return BCE_HIP_OK;
}

}  // namespace bce
