// kd_sufsort.hip -- the suffix array as a PRODUCT, and a checker for one (bce_hip_suffix_array / _device, bce_hip_sufcheck / _device,
// the libdivsufsort seam's divsufsort and sufcheck, `bce -gs`, `bce -gsd`, `bce -gsc`).
//
// The gather.  K1's sort of the m = n + 1 rotations of T$ (unique sentinel: k1_bwt.hip, k1_suffix_array) leaves the rotation that
// starts with $ in row 0 and the suffixes of T in rows 1 .. n, and rank[i] = the row of rotation i: ranks are "slot of the group's
// head", every group is a singleton when the sentinel is unique, so rank is the inverse of the order (what k1_divbwt reads its
// primary index from, and what the depth-first tail of K3 takes for the inverse).  One kernel: sa_out[r - 1] = sa[r], and where
// the inverse is wanted isa_out[i] = rank[i] - 1: all four streams are coalesced, 8 n bytes a side.
//
// The checker.  T: n bytes, SA: n words read as unsigned, 1 <= n < 2^31.  Three stages over blocks of SFC_BLOCK = 2048 rows, each
// reducing "the smallest index that fails" per block (scan_util.h: the maximum of ~index, 0 = none), then ONE workgroup per stage
// that walks the blocks' results 256 at a time:
//   range    row i with SA[i] >= n;
//   missing  inv[] filled with 0xFFFFFFFF, inv[SA[i]] = i scattered (entries out of range skipped; duplicates race, and whichever
//            writer wins, a position is left unnamed elsewhere): text position p with inv[p] still 0xFFFFFFFF;
//   order    row i >= 1 with a = SA[i - 1], b = SA[i] that does NOT satisfy
//              T[a] < T[b],  or  T[a] == T[b] and ( a + 1 == n  or  ( b + 1 < n and inv[a + 1] < inv[b + 1] ) ).
// For a permutation the rule holds on every row exactly when the array is sorted (Burkhardt, Karkkainen: by induction on the
// length of the common prefix, rows i - 1 and i compare as their first bytes and then as the suffixes one byte on, whose order inv
// already states; the empty suffix behind n - 1 is the smallest).  All three stages are queued at once -- the later ones guard
// every index, so an array that fails an earlier stage makes them compute something that nobody reads -- and three words come
// back; the first stage that found something decides.  No atomics: a block's result is written by its lane 0.
// Everything written is the feature's own (qb::sfc_* of c->qbuf); nothing a stage keeps is read.
#include "common.h"
#include "scan_util.h"

namespace bce {

namespace {

constexpr int SFC_T = 256;                   // lanes per workgroup (4 waves)
constexpr int SFC_ITEMS = 8;                 // rows per lane
constexpr uint32_t SFC_BLOCK = SFC_T * SFC_ITEMS;   // 2048

inline uint32_t sfc_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + SFC_BLOCK - 1) / SFC_BLOCK); }

__global__ __launch_bounds__(SFC_T) void sa_gather_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ rank, uint32_t n,
                                                          uint32_t *__restrict__ sa_out, uint32_t *__restrict__ isa_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * SFC_T + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SFC_T) {
    sa_out[i] = sa[i + 1u];                      // (row 0 is the rotation that starts with $)
    if (isa_out) isa_out[i] = rank[i] - 1u;
  }
}

// the block's smallest failing index as ~index (0: none), out of lane 0
__device__ __forceinline__ void sfc_block_result(uint32_t key, uint32_t *__restrict__ bres) {
  key = block_reduce_max<SFC_T>(key);
  if (threadIdx.x == 0) bres[blockIdx.x] = key;
}

__global__ __launch_bounds__(SFC_T) void sfc_range_kernel(const uint32_t *__restrict__ sa, uint32_t n, uint32_t *__restrict__ inv,
                                                          uint32_t *__restrict__ bres) {
  const uint32_t base = blockIdx.x * SFC_BLOCK;
  uint32_t key = 0;
#pragma unroll
  for (int k = SFC_ITEMS - 1; k >= 0; --k) {                           // (descending: the last assignment is the lane's lowest row)
    const uint32_t i = base + (uint32_t)k * SFC_T + threadIdx.x;
    if (i >= n) continue;
    const uint32_t p = sa[i];
    if (p >= n) key = ~i;
    else inv[p] = i;
  }
  sfc_block_result(key, bres);
}

__global__ __launch_bounds__(SFC_T) void sfc_missing_kernel(const uint32_t *__restrict__ inv, uint32_t n, uint32_t *__restrict__ bres) {
  const uint32_t base = blockIdx.x * SFC_BLOCK;
  uint32_t key = 0;
#pragma unroll
  for (int k = SFC_ITEMS - 1; k >= 0; --k) {
    const uint32_t p = base + (uint32_t)k * SFC_T + threadIdx.x;
    if (p < n && inv[p] == 0xFFFFFFFFu) key = ~p;
  }
  sfc_block_result(key, bres);
}

__global__ __launch_bounds__(SFC_T) void sfc_order_kernel(const uint8_t *__restrict__ T, const uint32_t *__restrict__ sa,
                                                          const uint32_t *__restrict__ inv, uint32_t n, uint32_t *__restrict__ bres) {
  const uint32_t base = blockIdx.x * SFC_BLOCK;
  uint32_t key = 0;
#pragma unroll
  for (int k = SFC_ITEMS - 1; k >= 0; --k) {
    const uint32_t i = base + (uint32_t)k * SFC_T + threadIdx.x;
    if (i == 0 || i >= n) continue;
    const uint32_t a = sa[i - 1u], b = sa[i];
    if (a >= n || b >= n) continue;                                    // (the range stage has decided: nothing here is read)
    const uint8_t ta = T[a], tb = T[b];
    bool ok = ta < tb;
    if (ta == tb) ok = a + 1u == n || (b + 1u < n && inv[a + 1u] < inv[b + 1u]);
    if (!ok) key = ~i;
  }
  sfc_block_result(key, bres);
}

// one workgroup per stage: res[stage] = the largest of the stage's nb block results
__global__ __launch_bounds__(SFC_T) void sfc_top_kernel(const uint32_t *__restrict__ bres, uint32_t nb, uint32_t *__restrict__ res) {
  const uint32_t *mine = bres + (size_t)blockIdx.x * nb;
  uint32_t m = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += SFC_T) m = m > mine[b] ? m : mine[b];
  m = block_reduce_max<SFC_T>(m);
  if (threadIdx.x == 0) res[blockIdx.x] = m;
}

}  // namespace

// d_sa[r] = sa[r + 1] and, unless d_isa is null, d_isa[i] = rank[i] - 1, for the n suffixes behind K1's sort of n + 1 rotations
// with a unique sentinel.  Queued; the caller waits.
int kd_sa_gather(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *rank, uint32_t n, uint32_t *d_sa, uint32_t *d_isa) {
  const uint64_t want = ((uint64_t)n + SFC_T - 1) / SFC_T;
  hipLaunchKernelGGL(sa_gather_kernel, dim3((uint32_t)(want < 65536u ? want : 65536u)), dim3(SFC_T), 0, c->stream, sa, rank, n, d_sa, d_isa);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// The verdict on d_sa (n words) as a suffix array of d_text (n bytes), 1 <= n < 2^31: *reason = BCE_HIP_SUFCHECK_*, *bad = the row
// or text position, UINT64_MAX for a sound array.  Complete on return.
int kd_sufcheck(bce_hip_ctx *c, const uint8_t *d_text, const uint32_t *d_sa, uint32_t n, uint64_t *bad, uint32_t *reason) {
  const uint32_t nb = sfc_blocks(n);
  DevBuf &inv = c->qbuf[qb::sfc_inv], &bsum = c->qbuf[qb::sfc_bsum], &res = c->qbuf[qb::sfc_res];
  BCE_TRY(ensure(c, inv, (size_t)n * 4));
  BCE_TRY(ensure(c, bsum, (size_t)nb * 3 * 4));
  BCE_TRY(ensure(c, res, 16));
  uint32_t *b = bsum.as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(inv.p, 0xFF, (size_t)n * 4, c->stream));
  hipLaunchKernelGGL(sfc_range_kernel, dim3(nb), dim3(SFC_T), 0, c->stream, d_sa, n, inv.as<uint32_t>(), b);
  hipLaunchKernelGGL(sfc_missing_kernel, dim3(nb), dim3(SFC_T), 0, c->stream, (const uint32_t *)inv.as<uint32_t>(), n, b + nb);
  hipLaunchKernelGGL(sfc_order_kernel, dim3(nb), dim3(SFC_T), 0, c->stream, d_text, d_sa, (const uint32_t *)inv.as<uint32_t>(), n, b + 2 * (size_t)nb);
  hipLaunchKernelGGL(sfc_top_kernel, dim3(3), dim3(SFC_T), 0, c->stream, (const uint32_t *)b, nb, res.as<uint32_t>());
  BCE_HIP_TRY(c, hipGetLastError());
  uint32_t found[3];
  BCE_TRY(read_back(c, found, res.p, sizeof found));
  BCE_HIP_TRY(c, hipGetLastError());
  *reason = BCE_HIP_SUFCHECK_OK;
  *bad = UINT64_MAX;
  for (uint32_t s = 0; s < 3; ++s)
    if (found[s]) { *reason = s + 1u; *bad = ~found[s]; break; }
  return BCE_HIP_OK;
}

}  // namespace bce
