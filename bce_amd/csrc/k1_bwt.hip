// k1_bwt.hip -- K1: rotation sort + BWT on the GPU.  Replaces File::rotate + File::bwt
// (bce.cpp:858-910), i.e. the host libdivsufsort call divbwt(T,T,0,n-1) (bce.cpp:901) and the two
// std::rotate fix-ups around it.
//
// What the reference produces (verified against the oracle): the BWT of ALL CYCLIC
// ROTATIONS of the input (rotations in sorted order, each contributing the byte that precedes it) and
// offset_ = the first index at which a minimal rotation starts.  Equal rotations (periodic inputs)
// have equal preceding bytes, so their relative order does not matter.
//
// Algorithm (MI355X-first, no sentinel, no recursion): prefix doubling on cyclic ranks; ranks are "index of the group head",
// so they only ever refine; stop when every group is a singleton or h >= n.  The sorter is k1_sort_rotations:
//   * first sort on a 64-BIT key of as many symbols as fit (alphabet compacted to ceil(log2 sigma) bits: 12 symbols
//     of text, 8 of arbitrary bytes) built in text order -- no gather at all; ranks by one scatter.
//   * every later round works on the ACTIVE list only (elements of non-singleton groups, ascending SA slots, head
//     flags in bit 31) and sorts each group where it lies: a workgroup loads the groups that START in its 2048-element
//     chunk into LDS, gathers rank[p + h] once, rank-sorts each group (all-pairs counting, groups <= 2048), writes the
//     suffixes back to their slots and the new ranks to a staging array -- two random accesses per element and no radix
//     pass.  Groups larger than 2048 are DEFERRED to one wide radix sort on (group number, rank[p + h]).  New ranks are
//     applied by a second kernel: a gather of another workgroup must never see a rank of this round (mixing old and new
//     ranks inside one comparison can order two suffixes wrongly).
// The sort comes in two halves (k1_first_sort: the first sort alone; k1_finish: ranks and every later round) so that the one-shot
// compression can make a provisional BWT between them and start the enumeration on it (api.hip compress_early): it
// asks the first sort for the depth that suits the step and, where the key has 8 bits to spare, lets each rotation's preceding
// byte ride in the key's low bits, so that the provisional BWT is read off the sorted keys.  k1_bwt runs both halves at the full
// depth, without the byte, and the final gather.
// The second half reads top to bottom as the steps of K1View (first_ranks, then per round segmented_round, sort_deferred,
// apply_ranks, relist); K1Buffers and K1View are the one place that says which of the context's buffers plays which part when.
#include <stdlib.h>

#include <utility>

#include "common.h"
#include "scan_util.h"

namespace bce {

constexpr int K1_T = 256;

// Blocks of the per-block passes (heads / apply / active list): at most K1_MAXB, each a whole number of 2048-element chunks.
// (nb is NOT monotonic in n -- 10^8 elements give 1018 blocks, 4*10^7 give 1022 -- so everything laid out behind the
//  per-block array sits at K1_MAXB, not at the first plan's nb: with the scalars at nb(n) the active rounds' block 1020
//  shared its count with the list length that block 0 writes at the end of the same kernel, which showed as soon as
//  other contexts delayed the last blocks of a launch.)
constexpr uint32_t K1_MAXB = 1024;
struct K1Plan { uint32_t nb, per_block; };
static K1Plan k1_plan(uint32_t n) {
  const uint32_t chunk = 2048;
  uint32_t chunks = (uint32_t)(((uint64_t)n + chunk - 1) / chunk);
  if (!chunks) chunks = 1;
  uint32_t nb = chunks < K1_MAXB ? chunks : K1_MAXB;
  uint32_t cpb = (chunks + nb - 1) / nb;
  nb = (chunks + cpb - 1) / cpb;
  return {nb, cpb * chunk};
}

// The words of c->blk behind the per-block array (blockmax / blockcnt, K1_MAXB words): results the host reads back, and
// three small tables.  k1_word() is the one place that knows where they lie.
enum K1Word : uint32_t {
  K1W_GROUPS = 0,                  // (unused; zeroed with the next three)
  K1W_OFFSET = 1,                  // offset_: k1_final_bwt
  K1W_ACTIVE = 2,                  // length of the next round's active list
  K1W_DEFERRED = 3,                // elements of groups too large for LDS in this round
  K1W_DL_COUNT = 4,                // the deferred list as built: its elements ...
  K1W_DL_GROUPS = 5,               // ... and its groups (written as a pair, behind K1W_DL_COUNT)
  K1W_HIST = 16,                   // byte histogram, 256 words
  K1W_CODE = 16 + 256,             // symbol code table, 256 x u16 (with the sentinel 257 symbols can occur)
  K1W_BLOCKCNT2 = 16 + 256 + 128,  // a second per-block array, K1_MAXB words (the deferred list's heads per block)
  K1W_END = 16 + 256 + 128 + K1_MAXB
};
static uint32_t *k1_word(bce_hip_ctx *c, K1Word w) { return c->blk.as<uint32_t>() + K1_MAXB + w; }

constexpr uint32_t K1_SLOT = 0x7FFFFFFFu, K1_HEAD = 0x80000000u;   // an active-list element: SA slot | starts a group
constexpr uint8_t KF_HEAD = 1, KF_KEEP = 2, KF_DEFER = 4;          // a round's verdict on a list element (flag[])

// What the blocks before this one hand on to it, from a per-block array that an earlier kernel filled:
// the max of blockmax[0 .. blockIdx.x) ...
__device__ __forceinline__ uint32_t k1_blocks_before_max(const uint32_t *__restrict__ blockmax) {
  uint32_t c = 0;
  for (uint32_t b = threadIdx.x; b < blockIdx.x; b += K1_T) { const uint32_t v = blockmax[b]; c = c > v ? c : v; }
  return block_reduce_max<K1_T>(c);
}
// ... and the sum of blockcnt[0 .. blockIdx.x), with the sum of all nb of them in *all
__device__ __forceinline__ uint32_t k1_blocks_before_sum(const uint32_t *__restrict__ blockcnt, uint32_t nb, uint32_t *all) {
  uint32_t b = 0, a = 0;
  for (uint32_t k = threadIdx.x; k < nb; k += K1_T) { const uint32_t v = blockcnt[k]; a += v; if (k < blockIdx.x) b += v; }
  const uint32_t before = block_reduce_sum<K1_T>(b);
  *all = block_reduce_sum<K1_T>(a);
  return before;
}

// nrk[j] = j where a new group starts, else 0; per-block max.  (k1, k2): the sorted key's high and low word; k2_mask: the bits
// of k2 that are key (a carried byte below them is not)
__global__ __launch_bounds__(K1_T) void k1_heads_kernel(const uint32_t *__restrict__ k1,
                                                        const uint32_t *__restrict__ k2, uint32_t k2_mask, uint32_t n,
                                                        uint32_t per_block, uint32_t *__restrict__ nrk,
                                                        uint32_t *__restrict__ blockmax) {
  const uint64_t beg = (uint64_t)blockIdx.x * per_block;
  uint64_t end = beg + per_block;
  if (end > n) end = n;
  uint32_t mx = 0;
  for (uint64_t j = beg + threadIdx.x; j < end; j += K1_T) {
    bool head = (j == 0);
    if (!head) {
      head = k1[j] != k1[j - 1];
      if (!head) head = ((k2[j] ^ k2[j - 1]) & k2_mask) != 0u;
    }
    nrk[j] = head ? (uint32_t)j : 0u;
    if (head) mx = (uint32_t)j;
  }
  mx = block_reduce_max<K1_T>(mx);
  if (threadIdx.x == 0) blockmax[blockIdx.x] = mx;
}

// The running max of nrk over this block's range of [0, n), seeded by the blocks before it: with nrk[j] = "a number that
// grows with j where a group starts, else 0" that is the number of j's group head.  VIA_IDX: dst[idx[j]] = it, else dst[j] = it.
template <bool VIA_IDX>
__device__ __forceinline__ void k1_running_max(const uint32_t *__restrict__ nrk, const uint32_t *__restrict__ blockmax, uint32_t n,
                                               uint32_t per_block, const uint32_t *__restrict__ idx, uint32_t *__restrict__ dst) {
  uint32_t carry = k1_blocks_before_max(blockmax);
  const uint64_t beg = (uint64_t)blockIdx.x * per_block;
  uint64_t end = beg + per_block;
  if (end > n) end = n;
  for (uint64_t base = beg; base < end; base += K1_T) {
    const uint64_t j = base + threadIdx.x;
    const bool valid = j < end;
    const uint32_t v = valid ? nrk[j] : 0u;
    uint32_t tot;
    uint32_t inc = block_incl_scan_max<K1_T>(v, &tot);
    inc = inc > carry ? inc : carry;
    if (valid) dst[VIA_IDX ? idx[j] : j] = inc;
    carry = carry > tot ? carry : tot;
  }
}

// rank[sa[j]] = max(nrk[0..j]): the rank of a suffix is the number of its group's head.  After the first sort sa is the whole
// order and the number an index; for the deferred groups sa is their sorted suffixes and the number a slot.
__global__ __launch_bounds__(K1_T) void k1_apply_kernel(const uint32_t *__restrict__ nrk,
                                                        const uint32_t *__restrict__ blockmax, uint32_t n,
                                                        uint32_t per_block, const uint32_t *__restrict__ sa,
                                                        uint32_t *__restrict__ rank) {
  k1_running_max<true>(nrk, blockmax, n, per_block, sa, rank);
}

// ---- rank scatters as sorts (inputs far beyond the caches: 10^9 B) ----
// rank[SA[j]] = v and rank[vs[i]] = nr[i] are one random 4-byte store per element into an array of 4 n bytes: at n = 10^9
// every one misses every cache and moves a line for its four bytes (k1_apply_kernel: 45 ms for one scatter of 4 GB, 23 G
// stores / s; 2.3 ms at 10^8).  Measured first, and rejected: ONE radix pass on the top bits of the destination, then stores
// into 16 MB windows -- the stores ran at the same 26 G / s (the eight XCDs' L2s each hold a part of every line of the
// window and write it back partly filled), and the BWT as a byte scatter bwt[rank[p]] = T[p - 1] into 4 MB windows took 28 ms
// against 19 for the gather.  What does pay is to SORT the pairs by destination (three 9/10-bit passes of the pair sort,
// ~4.5 ms each per 10^9 pairs): the scatter of a permutation becomes the sorted value array itself, that of a subset a
// store stream in ascending order.
#ifndef K1_PART_MIN
#define K1_PART_MIN (1u << 27)                   // elements from which the sorted form is used
#endif

// hv[j] = max(nrk[0..j]) = index of j's group head (what k1_apply_kernel scatters), written in place of order j
__global__ __launch_bounds__(K1_T) void k1_headidx_kernel(const uint32_t *__restrict__ nrk, const uint32_t *__restrict__ blockmax, uint32_t n,
                                                          uint32_t per_block, uint32_t *__restrict__ hv) {
  k1_running_max<false>(nrk, blockmax, n, per_block, nullptr, hv);
}
// dst[key[i]] = val[i] for the keys below `limit` (pairs grouped by destination range)
__global__ __launch_bounds__(K1_T) void k1_scatter32_kernel(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t m,
                                                            uint32_t limit, uint32_t *__restrict__ dst) {
  for (uint64_t i = (uint64_t)blockIdx.x * K1_T + threadIdx.x; i < m; i += (uint64_t)gridDim.x * K1_T) {
    const uint32_t k = key[i];
    if (k < limit) dst[k] = val[i];
  }
}
// the segmented round's results as pairs: key = the suffix (0xFFFFFFFF for deferred elements: they are applied elsewhere)
__global__ __launch_bounds__(K1_T) void k1_seg_pairs_kernel(const uint32_t *__restrict__ vs, const uint8_t *__restrict__ flag, uint8_t defer, uint32_t m,
                                                            uint32_t *__restrict__ key) {
  for (uint64_t i = (uint64_t)blockIdx.x * K1_T + threadIdx.x; i < m; i += (uint64_t)gridDim.x * K1_T)
    key[i] = (flag[i] & defer) ? 0xFFFFFFFFu : vs[i];
}
__global__ __launch_bounds__(K1_T) void k1_bwt_kernel(const uint8_t *__restrict__ T, const uint32_t *__restrict__ sa,
                                                      uint32_t n, uint8_t *__restrict__ bwt) {
  for (uint64_t j = (uint64_t)blockIdx.x * K1_T + threadIdx.x; j < n; j += (uint64_t)gridDim.x * K1_T) {
    const uint32_t q = sa[j];
    bwt[j] = T[q ? q - 1 : n - 1];
  }
}

// The same from sorted keys that carry the preceding byte in their low 8 bits: four keys in, four bytes out.
__global__ __launch_bounds__(K1_T) void k1_bwt_carried_kernel(const uint32_t *__restrict__ lo, uint32_t n, uint8_t *__restrict__ bwt) {
  const uint32_t quads = n >> 2;
  const uint4 *lo4 = reinterpret_cast<const uint4 *>(lo);
  uint32_t *bwt4 = reinterpret_cast<uint32_t *>(bwt);
  for (uint64_t i = (uint64_t)blockIdx.x * K1_T + threadIdx.x; i < quads; i += (uint64_t)gridDim.x * K1_T) {
    const uint4 k = lo4[i];
    bwt4[i] = (k.x & 0xFFu) | (k.y & 0xFFu) << 8 | (k.z & 0xFFu) << 16 | (k.w & 0xFFu) << 24;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
    const uint32_t j = (quads << 2) + threadIdx.x;
    bwt[j] = (uint8_t)lo[j];
  }
}

// offset_ = smallest position whose rotation is minimal (rank 0): rotate() keeps the FIRST minimal
// index (bce.cpp:873-874)
__global__ __launch_bounds__(K1_T) void k1_offset_kernel(const uint32_t *__restrict__ rank, uint32_t n,
                                                         uint32_t *__restrict__ out) {
  uint32_t best = 0xFFFFFFFFu;
  for (uint64_t p = (uint64_t)blockIdx.x * K1_T + threadIdx.x; p < n; p += (uint64_t)gridDim.x * K1_T)
    if (rank[p] == 0 && (uint32_t)p < best) best = (uint32_t)p;
  // wave min, then one atomic per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(best, o); best = best < t ? best : t; }
  if ((threadIdx.x & 63u) == 0 && best != 0xFFFFFFFFu) atomicMin(out, best);
}

// The first active list, from the first sort's heads: count (pass 0) / write (pass 1) the elements of non-singleton groups.
// head(i) = i == 0 || nrk[i] != 0; an element is a singleton iff it is a head and its successor is a head (or it is the last
// one).  out = the element's slot i | K1_HEAD where it starts a group (the rounds find the groups of the list from these
// bits), vout = the suffix at the slot: it travels with the list.
template <int PASS>
__global__ __launch_bounds__(K1_T) void k1_active_kernel(const uint32_t *__restrict__ nrk, uint32_t m,
                                                         uint32_t per_block, uint32_t nb, uint32_t *__restrict__ blockcnt,
                                                         uint32_t *__restrict__ out, uint32_t *__restrict__ total,
                                                         const uint32_t *__restrict__ sa_in, uint32_t *__restrict__ vout) {
  const uint64_t beg = (uint64_t)blockIdx.x * per_block;
  uint64_t end = beg + per_block;
  if (end > m) end = m;
  auto keep = [&](uint64_t i) -> bool {
    const bool h0 = i == 0 || nrk[i] != 0;
    const bool h1 = i + 1 >= m || nrk[i + 1] != 0;
    return !(h0 && h1);
  };
  if (PASS == 0) {
    uint32_t c = 0;
    for (uint64_t i = beg + threadIdx.x; i < end; i += K1_T) c += keep(i) ? 1u : 0u;
    c = block_reduce_sum<K1_T>(c);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = c;
  } else {
    uint32_t all;
    uint32_t base = k1_blocks_before_sum(blockcnt, nb, &all);
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = all;
    for (uint64_t c0 = beg; c0 < end; c0 += K1_T) {
      const uint64_t i = c0 + threadIdx.x;
      const bool k = i < end && keep(i);
      uint32_t tot;
      const uint32_t ex = block_excl_scan_sum<K1_T>(k ? 1u : 0u, &tot);
      if (k) {
        out[base + ex] = (uint32_t)i | ((i == 0 || nrk[i] != 0) ? K1_HEAD : 0u);
        vout[base + ex] = sa_in[i];
      }
      base += tot;
    }
  }
}

static uint32_t grid_for(uint32_t n) {
  uint64_t b = ((uint64_t)n + K1_T - 1) / K1_T;
  return (uint32_t)(b < 4096 ? (b ? b : 1) : 4096);
}

// ---- first sort: a 64-bit key of as many symbols as fit ---------------------------------------------------------------------
__global__ __launch_bounds__(K1_T) void k1_bytehist_kernel(const uint8_t *__restrict__ T, uint32_t n, uint32_t *__restrict__ hist) {
  __shared__ uint32_t lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * K1_T + threadIdx.x; i < n; i += (uint64_t)gridDim.x * K1_T) atomicAdd(&lh[T[i]], 1u);
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

// key[p] = the first nsym symbols of rotation p, `bits` bits each, first symbol most significant; val[p] = p.
// m = number of rotations (n bytes of T, plus the sentinel when m = n + 1: symbol 0, every byte's code is then >= 1).
// carry (never with the sentinel, nsym * bits <= 56): the key moves up by 8 bits and T[p - 1], the rotation's BWT byte, rides below.
constexpr int K1I_E = 8;
__global__ __launch_bounds__(K1_T) void k1_init64_kernel(const uint8_t *__restrict__ T, uint32_t m, uint32_t nbytes,
                                                         const uint16_t *__restrict__ code, uint32_t bits, uint32_t nsym, uint32_t carry,
                                                         uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, uint32_t *__restrict__ val) {
  __shared__ uint16_t sym[K1_T * K1I_E + 16];
  __shared__ uint16_t lut[256];
  lut[threadIdx.x] = code[threadIdx.x];
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * (K1_T * K1I_E);
  for (uint32_t i = threadIdx.x; i < K1_T * K1I_E + 16; i += K1_T) {
    uint64_t q = base + i;
    if (q >= m) q %= m;
    sym[i] = q < nbytes ? lut[T[q]] : (uint16_t)0;           // (q == nbytes only with the sentinel)
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < K1I_E; ++e) {
    const uint32_t o = (uint32_t)e * K1_T + threadIdx.x;
    const uint64_t p = base + o;
    if (p < m) {
      uint64_t k = 0;
      for (uint32_t b = 0; b < nsym; ++b) k = (k << bits) | sym[o + b];
      if (carry) k = (k << 8) | T[p ? p - 1 : (uint64_t)nbytes - 1];
      lo[p] = (uint32_t)k;
      hi[p] = (uint32_t)(k >> 32);
      val[p] = (uint32_t)p;
    }
  }
}

// ---- segmented rounds ----
constexpr int SEG_T = 1024;                    // threads of a workgroup
constexpr int SEG_CH = 2048;                   // list elements whose groups a workgroup owns (groups that START in its chunk)
constexpr int SEG_CAP = 2048;                  // largest group sorted in LDS; larger ones are deferred
constexpr int SEG_W = SEG_CH + SEG_CAP;        // sortable window: list positions [base, base + W)
constexpr int SEG_HW = SEG_W + SEG_CAP;        // head-flag window: list positions [base - CAP, base + W)

// highest set bit at or below pos (and at or above lo_limit), or -1
__device__ __forceinline__ int seg_prev_bit(const uint64_t *b, int pos, int lo_limit) {
  int wi = pos >> 6;
  uint64_t word = b[wi] & (~0ull >> (63 - (pos & 63)));
  const int wl = lo_limit >> 6;
  while (word == 0 && wi > wl) { --wi; word = b[wi]; }
  if (!word) return -1;
  const int r = wi * 64 + 63 - __clzll((long long)word);
  return r >= lo_limit ? r : -1;
}
// lowest set bit above pos (and at or below hi_limit), or -1
__device__ __forceinline__ int seg_next_bit(const uint64_t *b, int pos, int hi_limit) {
  int wi = pos >> 6;
  uint64_t word = (pos & 63) == 63 ? 0ull : (b[wi] & (~0ull << ((pos & 63) + 1)));
  const int wh = hi_limit >> 6;
  while (word == 0 && wi < wh) { ++wi; word = b[wi]; }
  if (!word) return -1;
  const int r = wi * 64 + __ffsll((long long)word) - 1;
  return r <= hi_limit ? r : -1;
}

// One doubling round on the groups that lie whole in LDS.  A[i] = SA slot of active element i (ascending) | head bit.
// Writes: sa[slot] (the group's suffixes in their new order), nr[i] / vs[i] (new rank = slot of the new group's head, and
// the suffix now at position i: applied by k1_seg_apply_kernel), flag[i] (new head, keep = not a singleton); elements of
// groups larger than SEG_CAP get KF_DEFER and are counted in *ndefer.
__global__ __launch_bounds__(SEG_T) void k1_seg_sort_kernel(const uint32_t *__restrict__ A, const uint32_t *__restrict__ V, uint32_t m, uint32_t *__restrict__ sa,
                                                            const uint32_t *__restrict__ rank, uint32_t n, uint32_t h,
                                                            uint32_t *__restrict__ nr, uint32_t *__restrict__ vs,
                                                            uint8_t *__restrict__ flag, uint32_t *__restrict__ ndefer) {
  __shared__ uint64_t hb[SEG_HW / 64 + 1];
  __shared__ uint64_t nbits[SEG_W / 64 + 1];
  __shared__ __attribute__((aligned(16))) uint32_t K[SEG_W];
  __shared__ uint32_t S[SEG_W], SL[SEG_W];
  __shared__ uint32_t s_defer;
  __shared__ int s_cntw;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const int64_t base = (int64_t)blockIdx.x * SEG_CH;
  if (tid == 0) { s_defer = 0; hb[SEG_HW / 64] = 0; nbits[SEG_W / 64] = 0; }
  // 1. head bits of the window (position m is a head: the end of the list) and the slots of the sortable part
#pragma unroll
  for (int it = 0; it < SEG_HW / SEG_T; ++it) {
    const int u = it * SEG_T + (int)tid;
    const int64_t i = base - SEG_CAP + u;
    uint32_t a = 0;
    bool hd = false;
    if (i >= 0) {
      if (i < (int64_t)m) { a = A[i]; hd = (a & K1_HEAD) != 0u; }
      else hd = true;
    }
    const uint64_t bal = __ballot(hd);
    if (lane == 0) hb[u >> 6] = bal;
    if (u >= SEG_CAP) SL[u - SEG_CAP] = a & K1_SLOT;
  }
  __syncthreads();
  // the groups that start in this chunk end at the first head at or after the next chunk's start: nothing beyond it is
  // this block's business (positions of the chunk itself are always looked at: their big groups are flagged here)
  if (tid == 0) {
    const int e = seg_next_bit(hb, SEG_CAP + SEG_CH - 1, SEG_HW - 1);
    const int cw = (e < 0 ? SEG_HW : e) - SEG_CAP;
    s_cntw = cw > SEG_CH ? cw : SEG_CH;
  }
  __syncthreads();
  const int cntw = s_cntw;
  // 2. every position up to there finds its group; the ones of small groups that start in this chunk gather their key
  constexpr int EPT = SEG_W / SEG_T;
  uint32_t k2[EPT], sfx[EPT];
  int gs[EPT], ge[EPT];
  bool mine[EPT];
  uint32_t ndef = 0;
#pragma unroll
  for (int it = 0; it < EPT; ++it) {
    const int w = it * SEG_T + (int)tid, u = w + SEG_CAP;
    const int64_t i = base + w;
    mine[it] = false; gs[it] = 0; ge[it] = 0; k2[it] = 0; sfx[it] = 0;
    if (w < cntw && i < (int64_t)m) {
      const int g0 = seg_prev_bit(hb, u, u - SEG_CAP + 1);            // a head within the last CAP positions, or the group is big
      bool big = g0 < 0;
      int g1 = -1;
      if (!big) {
        const int lim = g0 + SEG_CAP < SEG_HW - 1 ? g0 + SEG_CAP : SEG_HW - 1;
        g1 = seg_next_bit(hb, u, lim);                              // the next head within CAP of the group's start
        big = g1 < 0;
      }
      if (big) {
        if (w < SEG_CH) { flag[i] = KF_DEFER; ++ndef; }               // (each element is flagged by the block of its own chunk)
      } else if (g0 >= SEG_CAP && g0 < SEG_CAP + SEG_CH) {
        mine[it] = true; gs[it] = g0 - SEG_CAP; ge[it] = g1 - SEG_CAP;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < EPT; ++it) if (mine[it]) sfx[it] = V[base + it * SEG_T + (int)tid];
#pragma unroll
  for (int it = 0; it < EPT; ++it)
    if (mine[it]) {
      uint64_t q = (uint64_t)sfx[it] + h;
      if (q >= n) q -= n;
      k2[it] = rank[q];
    }
#pragma unroll
  for (int it = 0; it < EPT; ++it) if (mine[it]) K[it * SEG_T + (int)tid] = k2[it];
  if (ndef) atomicAdd(&s_defer, ndef);
  __syncthreads();
  // 3. rank sort inside each group: position = number of smaller (key, old position) pairs = the members before w with
  //    key <= mine plus the members after w with key < mine.  Two compare-and-add-carry instructions per member, four
  //    members per LDS read (most of a mid-sized group's time is this loop: 65-2048 members, all pairs).
  int pos[EPT];
#pragma unroll
  for (int it = 0; it < EPT; ++it) {
    pos[it] = 0;
    if (mine[it]) {
      const int w = it * SEG_T + (int)tid;
      const uint32_t kw = k2[it];
      uint32_t r = 0;
      {
        int t = gs[it];
        const int e = w;                                              // [gs, w): <=
        for (; t < e && (t & 3); ++t) r += K[t] <= kw ? 1u : 0u;
        for (; t + 4 <= e; t += 4) {
          const uint4 v = *reinterpret_cast<const uint4 *>(&K[t]);
          r += (v.x <= kw ? 1u : 0u) + (v.y <= kw ? 1u : 0u) + (v.z <= kw ? 1u : 0u) + (v.w <= kw ? 1u : 0u);
        }
        for (; t < e; ++t) r += K[t] <= kw ? 1u : 0u;
      }
      {
        int t = w + 1;
        const int e = ge[it];                                         // (w, ge): <
        for (; t < e && (t & 3); ++t) r += K[t] < kw ? 1u : 0u;
        for (; t + 4 <= e; t += 4) {
          const uint4 v = *reinterpret_cast<const uint4 *>(&K[t]);
          r += (v.x < kw ? 1u : 0u) + (v.y < kw ? 1u : 0u) + (v.z < kw ? 1u : 0u) + (v.w < kw ? 1u : 0u);
        }
        for (; t < e; ++t) r += K[t] < kw ? 1u : 0u;
      }
      pos[it] = gs[it] + (int)r;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < EPT; ++it) if (mine[it]) { K[pos[it]] = k2[it]; S[pos[it]] = sfx[it]; }
  __syncthreads();
  // 4. new heads: position w of its group's new order
#pragma unroll
  for (int it = 0; it < EPT; ++it) {
    const int w = it * SEG_T + (int)tid;
    if ((w & ~63) < cntw) {                                          // (wave-uniform)
      const bool nh = mine[it] && (w == gs[it] || K[w] != K[w - 1]);
      const uint64_t bal = __ballot(nh);
      if (lane == 0) nbits[w >> 6] = bal;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < EPT; ++it)
    if (mine[it]) {
      const int w = it * SEG_T + (int)tid;
      const int hp = seg_prev_bit(nbits, w, gs[it]);                 // >= gs: the group's first position is a head
      const bool nh = hp == w;
      const bool next_head = (w + 1 == ge[it]) || ((nbits[(w + 1) >> 6] >> ((w + 1) & 63)) & 1ull);
      const int64_t i = base + w;
      const uint32_t s = S[w];
      sa[SL[w]] = s;
      nr[i] = SL[hp];
      vs[i] = s;
      flag[i] = (uint8_t)((nh ? KF_HEAD : 0) | ((nh && next_head) ? 0 : KF_KEEP));
    }
  if (tid == 0 && s_defer) atomicAdd(ndefer, s_defer);
}

// rank[vs[i]] = nr[i] for the elements the segmented kernel sorted (the deferred ones are applied by the global path)
__global__ __launch_bounds__(K1_T) void k1_seg_apply_kernel(const uint32_t *__restrict__ nr, const uint32_t *__restrict__ vs,
                                                            const uint8_t *__restrict__ flag, uint32_t m, uint32_t *__restrict__ rank) {
  for (uint64_t i = (uint64_t)blockIdx.x * K1_T + threadIdx.x; i < m; i += (uint64_t)gridDim.x * K1_T)
    if (!(flag[i] & KF_DEFER)) rank[vs[i]] = nr[i];
}

// compaction of the list by a flag: PASS 0 counts per block, PASS 1 writes.  MODE 0: deferred elements -> their list index (idx)
// and slot (slots); MODE 1: kept elements -> slot | new head bit and the suffix now at that slot (the next round's lists).
template <int PASS, int MODE>
__global__ __launch_bounds__(K1_T) void k1_relist_kernel(const uint32_t *__restrict__ A, const uint32_t *__restrict__ vs,
                                                         const uint8_t *__restrict__ flag, uint32_t m,
                                                         uint32_t per_block, uint32_t nb, uint32_t *__restrict__ blockcnt,
                                                         uint32_t *__restrict__ out, uint32_t *__restrict__ out2, uint32_t *__restrict__ total,
                                                         uint32_t *__restrict__ blockcnt2, uint32_t *__restrict__ out3) {
  const uint64_t beg = (uint64_t)blockIdx.x * per_block;
  uint64_t end = beg + per_block;
  if (end > m) end = m;
  auto take = [&](uint64_t i) -> bool { return MODE == 0 ? (flag[i] & KF_DEFER) != 0 : (flag[i] & KF_KEEP) != 0; };
  if (PASS == 0) {
    uint32_t cnt = 0, hc = 0;
    for (uint64_t i = beg + threadIdx.x; i < end; i += K1_T) {
      const bool k = take(i);
      cnt += k ? 1u : 0u;
      if (MODE == 0) hc += (k && (A[i] & K1_HEAD)) ? 1u : 0u;
    }
    cnt = block_reduce_sum<K1_T>(cnt);
    if (MODE == 0) hc = block_reduce_sum<K1_T>(hc);
    if (threadIdx.x == 0) { blockcnt[blockIdx.x] = cnt; if (MODE == 0) blockcnt2[blockIdx.x] = hc; }
  } else {
    uint32_t all, hbase = 0;
    uint32_t base = k1_blocks_before_sum(blockcnt, nb, &all);
    if (MODE == 0) {
      uint32_t all2;
      hbase = k1_blocks_before_sum(blockcnt2, nb, &all2);
      if (blockIdx.x == 0 && threadIdx.x == 0) total[1] = all2;     // deferred groups
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) total[0] = all;
    for (uint64_t c0 = beg; c0 < end; c0 += K1_T) {
      const uint64_t i = c0 + threadIdx.x;
      const bool k = i < end && take(i);
      const uint32_t a_i = (MODE == 0 && k) ? A[i] : 0u;
      uint32_t tot;
      const uint32_t ex = block_excl_scan_sum<K1_T>(k ? 1u : 0u, &tot);
      uint32_t htot = 0, hex = 0;
      const uint32_t hd = (MODE == 0 && (a_i & K1_HEAD)) ? 1u : 0u;
      if (MODE == 0) hex = block_excl_scan_sum<K1_T>(hd, &htot);
      if (k) {
        if (MODE == 0) { out[base + ex] = (uint32_t)i; out2[base + ex] = a_i & K1_SLOT; out3[base + ex] = hbase + hex + hd - 1u; }
        else { out[base + ex] = (A[i] & K1_SLOT) | ((flag[i] & KF_HEAD) ? K1_HEAD : 0u); out2[base + ex] = vs[i]; }
      }
      base += tot;
      hbase += htot;
    }
  }
}

// ---- the global path (round 3): the elements of groups too large for LDS, all such groups in ONE sort ----------------
// key = (number of the group among the deferred groups) << rbits | rank[p + h], value = p: one stable sort on the bits in
// use orders every deferred group by its second key where it lies (the list is ascending and holds whole groups, so the
// sorted sequence lines up with the slots).  One random gather and one random scatter per element, five wide passes.
__global__ __launch_bounds__(K1_T) void k1_big_gather_kernel(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ gid,
                                                             const uint32_t *__restrict__ V, const uint32_t *__restrict__ rank,
                                                             uint32_t n, uint32_t nd, uint32_t h, uint32_t rbits,
                                                             uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, uint32_t *__restrict__ val) {
  for (uint64_t j = (uint64_t)blockIdx.x * K1_T + threadIdx.x; j < nd; j += (uint64_t)gridDim.x * K1_T) {
    const uint32_t p = V[idx[j]];
    uint64_t q = (uint64_t)p + h;
    if (q >= n) q -= n;
    const uint64_t key = ((uint64_t)gid[j] << rbits) | rank[q];
    lo[j] = (uint32_t)key;
    hi[j] = (uint32_t)(key >> 32);
    val[j] = p;
  }
}
// the sorted suffixes go back to their slots; nrk[j] = slot where a new group starts (else 0), per-block maxima for k1_apply_kernel
__global__ __launch_bounds__(K1_T) void k1_big_heads_kernel(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ lo,
                                                            const uint32_t *__restrict__ hi, const uint32_t *__restrict__ val,
                                                            uint32_t nd, uint32_t per_block, uint32_t *__restrict__ sa,
                                                            uint32_t *__restrict__ nrk, uint32_t *__restrict__ blockmax) {
  const uint64_t beg = (uint64_t)blockIdx.x * per_block;
  uint64_t end = beg + per_block;
  if (end > nd) end = nd;
  uint32_t mx = 0;
  for (uint64_t j = beg + threadIdx.x; j < end; j += K1_T) {
    const uint32_t slot = slots[j];
    sa[slot] = val[j];
    const bool head = j == 0 || lo[j] != lo[j - 1] || hi[j] != hi[j - 1];
    nrk[j] = head ? slot : 0u;
    if (head) mx = slot;
  }
  mx = block_reduce_max<K1_T>(mx);
  if (threadIdx.x == 0) blockmax[blockIdx.x] = mx;
}

// the global path's result (nrk over the deferred list: slot where a new group starts, else 0) as flags of the list elements
__global__ __launch_bounds__(K1_T) void k1_defer_flags_kernel(const uint32_t *__restrict__ nrk, const uint32_t *__restrict__ idx,
                                                              const uint32_t *__restrict__ sorted, uint32_t nd,
                                                              uint8_t *__restrict__ flag, uint32_t *__restrict__ vs) {
  for (uint64_t j = (uint64_t)blockIdx.x * K1_T + threadIdx.x; j < nd; j += (uint64_t)gridDim.x * K1_T) {
    const bool hd = j == 0 || nrk[j] != 0u;
    const bool nx = j + 1 >= nd || nrk[j + 1] != 0u;
    const uint32_t i = idx[j];
    flag[i] = (uint8_t)(KF_DEFER | (hd ? KF_HEAD : 0) | ((hd && nx) ? 0 : KF_KEEP));
    vs[i] = sorted[j];
  }
}

// Elements from which the two rank scatters are done as sorts (K1_PART_MIN; BCE_K1_PART_MIN overrides it, read once).
static uint32_t k1_part_min() {
  static const uint32_t part_min = getenv("BCE_K1_PART_MIN") ? (uint32_t)strtoul(getenv("BCE_K1_PART_MIN"), nullptr, 10) : K1_PART_MIN;
  return part_min;
}

// The context's buffers as the sort names them (k1_first_sort_wide sizes them all) and the trace: what both halves see.
// Everything is queued on c->stream, so "free" below means "every kernel that reads it is queued ahead".  DESIGN, K1, has the
// roles as a table.
struct K1Buffers {
  bce_hip_ctx *c;
  uint32_t n, g;
  uint32_t *blockmax;            // c->blk's first K1_MAXB words: what the first kernel of a pair leaves per block for the second
  uint32_t *rank;                // c->rank: rank of every rotation = index of its group's head
  uint32_t *lo[2], *hi[2], *val[2];   // c->key[] / c->khi[] / c->sa[]: the first sort's ping-pong of (low word, high word, rotation), from side 0
  uint32_t *nrk;                 // c->nrk: "index where a group starts, else 0" over the first sort's order; free once the first list is queued
  uint32_t *k2;                  // c->k2: the first sorted apply's head indices; free when that sort is queued
  uint8_t *flag;                 // c->kflag: KF_* of every list element, rewritten by each round
  uint32_t *act[2], *actv[2];    // c->act[] / c->actv[]: the active list (slot | head bit), the suffix at each slot; [0] this round's, [1] the next one's
  bool trace;
  double t_prev;

  K1Buffers(bce_hip_ctx *ctx, uint32_t n_) : c(ctx), n(n_), g(grid_for(n_)) {
    blockmax = c->blk.as<uint32_t>();
    rank = c->rank.as<uint32_t>(); k2 = c->k2.as<uint32_t>(); nrk = c->nrk.as<uint32_t>();
    flag = c->kflag.as<uint8_t>();
    for (int i = 0; i < 2; ++i) {
      lo[i] = c->key[i].as<uint32_t>(); hi[i] = c->khi[i].as<uint32_t>(); val[i] = c->sa[i].as<uint32_t>();
      act[i] = c->act[i].as<uint32_t>(); actv[i] = c->actv[i].as<uint32_t>();
    }
    trace = getenv("BCE_K1_TRACE") != nullptr;
    t_prev = now_s();
  }
  uint32_t *word(K1Word w) const { return k1_word(c, w); }
  void lap(const char *what, uint64_t h_, uint32_t m_, uint32_t nd_) {
    if (!trace) return;
    (void)hipStreamSynchronize(c->stream);
    const double t = now_s();
    fprintf(stderr, "k1 %p: %-10s h %llu active %u deferred %u (+%.2f ms)\n", (void *)c, what, (unsigned long long)h_, m_, nd_, (t - t_prev) * 1e3);
    t_prev = t;
  }
};

// The second half's state, built from what the first half left in the context (k1_res, k1_h, k1_carry), and its steps.
struct K1View : K1Buffers {
  K1Plan pl;                     // the per-block passes over all n elements
  uint32_t rbits, part_min;      // bits of a rank; elements from which a rank scatter is done as a sort
  int res;                       // (lo[res], hi[res], val[res]) hold the first sort's keys and its order
  uint32_t *sa;                  // = val[res]: the order; every round reorders it inside its groups, in place
  uint32_t *nr, *vs;             // = hi[0], hi[1]: a round's new rank and suffix per list position.  Free once the heads are taken from
                                 // the first sort's keys (hi[res ^ 1]: a key buffer of the first sorted apply, before the first round)
  // The first sorted apply also takes lo[res ^ 1] (keys), val[res ^ 1] and rank (values: its last pass writes the ranks themselves).
  // The deferred sort takes lo[] (low words; free once the heads are taken and a provisional BWT is queued), val[res ^ 1] and k2
  // (high words), nrk and c->dl[3] (values; the one it leaves unused takes the heads of its result) beside the list in c->dl[0 .. 2]:
  // all free again when the round's apply is queued, which as a sort takes lo[] (keys), k2 and val[res ^ 1] (values) in its turn.
  uint64_t h;                    // symbols by which the rotations are ordered
  uint32_t m, nd;                // active elements; of them deferred in this round

  K1View(bce_hip_ctx *ctx, uint32_t n_) : K1Buffers(ctx, n_), pl(k1_plan(n_)), rbits(ceil_log2(n_)), part_min(k1_part_min()), res(ctx->k1_res),
                                          sa(val[res]), nr(hi[0]), vs(hi[1]), h(ctx->k1_h), m(0), nd(0) {}

  // A scatter dst[key] = value as a sort: cnt (destination, value) pairs sorted on rbits bits in two steps, the digit of a balanced
  // pass and then the rest.  The first step reads (k_in, v_in) and writes (k_a, v_a); the rest goes between (k_a, v_a) and
  // (k_b, v_b), where k_b may be k_in again.  *at_b: the result lies in (k_b, v_b), else in (k_a, v_a).
  int sort_by_dest(uint32_t cnt, uint32_t *k_in, uint32_t *v_in, uint32_t *k_a, uint32_t *v_a, uint32_t *k_b, uint32_t *v_b, int *at_b) {
    const uint32_t b1 = rbits / ((rbits + 9u) / 10u);
    uint32_t *pk[2] = {k_in, k_a}, *pv[2] = {v_in, v_a};
    BCE_TRY(radix_sort_pairs(c, pk, pv, cnt, 0, b1, at_b, 10));             // one pass: the input is left alone
    uint32_t *qk[2] = {k_a, k_b}, *qv[2] = {v_a, v_b};
    return radix_sort_pairs(c, qk, qv, cnt, b1, rbits - b1, at_b, 10);
  }

  // Ranks from the sorted keys (group heads, then one scatter of their indices -- or the sort that stands for it) and the first
  // active list.
  int first_ranks() {
    BCE_HIP_TRY(c, hipMemsetAsync(word(K1W_GROUPS), 0, 16, c->stream));     // the four result words
    hipLaunchKernelGGL(k1_heads_kernel, dim3(pl.nb), dim3(K1_T), 0, c->stream, hi[res], lo[res], c->k1_carry ? 0xFFFFFF00u : 0xFFFFFFFFu, n, pl.per_block,
                       nrk, blockmax);
    const bool sorted_apply = n >= part_min;
    if (sorted_apply) hipLaunchKernelGGL(k1_headidx_kernel, dim3(pl.nb), dim3(K1_T), 0, c->stream, nrk, blockmax, n, pl.per_block, k2);
    else hipLaunchKernelGGL(k1_apply_kernel, dim3(pl.nb), dim3(K1_T), 0, c->stream, nrk, blockmax, n, pl.per_block, sa, rank);
    hipLaunchKernelGGL(k1_active_kernel<0>, dim3(pl.nb), dim3(K1_T), 0, c->stream, nrk, n, pl.per_block, pl.nb, blockmax, act[0], word(K1W_ACTIVE), sa, actv[0]);
    hipLaunchKernelGGL(k1_active_kernel<1>, dim3(pl.nb), dim3(K1_T), 0, c->stream, nrk, n, pl.per_block, pl.nb, blockmax, act[0], word(K1W_ACTIVE), sa, actv[0]);
    if (sorted_apply) {
      // rank = the head indices (k2) sorted by suffix: the first pass reads the suffix array and leaves it alone, the last one
      // writes the rank array itself
      int at_b = 0;
      BCE_TRY(sort_by_dest(n, sa, k2, lo[res ^ 1], rank, hi[res ^ 1], val[res ^ 1], &at_b));
      if (at_b) BCE_HIP_TRY(c, hipMemcpyAsync(rank, val[res ^ 1], (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));   // (an odd number of passes behind the first: n > 2^30)
    }
    BCE_TRY(read_back(c, &m, word(K1W_ACTIVE), 4));
    lap("first ranks", h, m, 0);
    return BCE_HIP_OK;
  }

  // One doubling round on the groups that fit LDS, each sorted where it lies: sa reordered, the new ranks staged in (nr, vs),
  // flags; the larger groups' elements are flagged and counted (nd).
  int segmented_round() {
    const uint32_t nblk = (uint32_t)(((uint64_t)m + SEG_CH - 1) / SEG_CH);
    BCE_HIP_TRY(c, hipMemsetAsync(word(K1W_DEFERRED), 0, 4, c->stream));
    hipLaunchKernelGGL(k1_seg_sort_kernel, dim3(nblk), dim3(SEG_T), 0, c->stream, act[0], actv[0], m, sa, rank, n, (uint32_t)h, nr, vs, flag, word(K1W_DEFERRED));
    return read_back(c, &nd, word(K1W_DEFERRED), 4);
  }

  // The groups that do not fit LDS: one sort of all their elements by (group, second key), their suffixes back to their slots,
  // their ranks applied, their flags and vs written like the segmented round's.
  int sort_deferred() {
    for (int i = 0; i < 4; ++i) BCE_TRY(ensure(c, c->dl[i], (size_t)nd * 4));
    uint32_t *idx = c->dl[0].as<uint32_t>(), *slots = c->dl[1].as<uint32_t>(), *gid = c->dl[2].as<uint32_t>();
    const K1Plan ap = k1_plan(m);
    hipLaunchKernelGGL((k1_relist_kernel<0, 0>), dim3(ap.nb), dim3(K1_T), 0, c->stream, act[0], vs, flag, m, ap.per_block, ap.nb, blockmax, idx, slots,
                       word(K1W_DL_COUNT), word(K1W_BLOCKCNT2), gid);
    hipLaunchKernelGGL((k1_relist_kernel<1, 0>), dim3(ap.nb), dim3(K1_T), 0, c->stream, act[0], vs, flag, m, ap.per_block, ap.nb, blockmax, idx, slots,
                       word(K1W_DL_COUNT), word(K1W_BLOCKCNT2), gid);
    uint32_t cnts[2] = {0, 0};                   // K1W_DL_COUNT, K1W_DL_GROUPS
    BCE_TRY(read_back(c, cnts, word(K1W_DL_COUNT), 8));
    if (cnts[0] != nd || cnts[1] == 0 || cnts[1] > nd) { snprintf(c->err, sizeof c->err, "k1: deferred list %u / %u groups, expected %u elements", cnts[0], cnts[1], nd); return BCE_HIP_E_INTERNAL; }
    const uint32_t gbits = ceil_log2(cnts[1]);
    uint32_t *bl[2] = {lo[0], lo[1]};
    uint32_t *bh[2] = {val[res ^ 1], k2};
    uint32_t *bv[2] = {nrk, c->dl[3].as<uint32_t>()};
    const uint32_t ga = grid_for(nd);
    hipLaunchKernelGGL(k1_big_gather_kernel, dim3(ga), dim3(K1_T), 0, c->stream, idx, gid, actv[0], rank, n, nd, (uint32_t)h, rbits, bl[0], bh[0], bv[0]);
    int rb = 0;
    BCE_TRY(radix_sort_wide(c, bl, bh, bv, nd, 0, rbits + gbits, &rb, 9));
    const K1Plan dp = k1_plan(nd);
    uint32_t *snrk = bv[rb ^ 1];
    hipLaunchKernelGGL(k1_big_heads_kernel, dim3(dp.nb), dim3(K1_T), 0, c->stream, slots, bl[rb], bh[rb], bv[rb], nd, dp.per_block, sa, snrk, blockmax);
    hipLaunchKernelGGL(k1_apply_kernel, dim3(dp.nb), dim3(K1_T), 0, c->stream, snrk, blockmax, nd, dp.per_block, bv[rb], rank);
    hipLaunchKernelGGL(k1_defer_flags_kernel, dim3(ga), dim3(K1_T), 0, c->stream, snrk, idx, bv[rb], nd, flag, vs);
    return BCE_HIP_OK;
  }

  // rank[vs[i]] = nr[i] for the elements the segmented round sorted: a scatter, or from part_min elements up a sort by suffix
  // and a store stream in ascending order.
  int apply_ranks() {
    if (m >= part_min) {
      hipLaunchKernelGGL(k1_seg_pairs_kernel, dim3(grid_for(m)), dim3(K1_T), 0, c->stream, vs, flag, KF_DEFER, m, lo[0]);
      int at_b = 0;
      BCE_TRY(sort_by_dest(m, lo[0], nr, lo[1], k2, lo[0], val[res ^ 1], &at_b));
      hipLaunchKernelGGL(k1_scatter32_kernel, dim3(grid_for(m)), dim3(K1_T), 0, c->stream, at_b ? lo[0] : lo[1], at_b ? val[res ^ 1] : k2, m, n, rank);
    } else {
      hipLaunchKernelGGL(k1_seg_apply_kernel, dim3(grid_for(m)), dim3(K1_T), 0, c->stream, nr, vs, flag, m, rank);
    }
    return BCE_HIP_OK;
  }

  // The next round's list: the elements that are still in a group of two or more, with their new head bits.
  int relist() {
    const K1Plan ap = k1_plan(m);
    hipLaunchKernelGGL((k1_relist_kernel<0, 1>), dim3(ap.nb), dim3(K1_T), 0, c->stream, act[0], vs, flag, m, ap.per_block, ap.nb, blockmax, act[1], actv[1],
                       word(K1W_ACTIVE), nullptr, nullptr);
    hipLaunchKernelGGL((k1_relist_kernel<1, 1>), dim3(ap.nb), dim3(K1_T), 0, c->stream, act[0], vs, flag, m, ap.per_block, ap.nb, blockmax, act[1], actv[1],
                       word(K1W_ACTIVE), nullptr, nullptr);
    BCE_TRY(read_back(c, &m, word(K1W_ACTIVE), 4));
    std::swap(act[0], act[1]);
    std::swap(actv[0], actv[1]);
    h <<= 1;
    c->stats.sort_rounds++;
    lap("round", h, m, nd);
    return BCE_HIP_OK;
  }
};

// First half of the sort: the rotations ordered by their first c->k1_h symbols (one byte each), ties by position, in
// sa[c->k1_res]; the sorted keys beside them.  Nothing of the rank array yet.  want_by_bits (or null) and may_carry: common.h.
static int k1_first_sort_wide(bce_hip_ctx *c, const uint8_t *T, uint32_t n, bool sentinel, const uint8_t *want_by_bits, bool may_carry) {
  const size_t b4 = (size_t)n * 4;
  for (int i = 0; i < 2; ++i) { BCE_TRY(ensure(c, c->sa[i], b4)); BCE_TRY(ensure(c, c->key[i], b4)); BCE_TRY(ensure(c, c->khi[i], b4)); }
  BCE_TRY(ensure(c, c->rank, b4));
  BCE_TRY(ensure(c, c->k2, b4));
  BCE_TRY(ensure(c, c->nrk, b4));
  BCE_TRY(ensure(c, c->kflag, (size_t)n + 16));
  for (int i = 0; i < 2; ++i) { BCE_TRY(ensure(c, c->act[i], b4)); BCE_TRY(ensure(c, c->actv[i], b4)); }
  BCE_TRY(ensure(c, c->blk, (size_t)(K1_MAXB + K1W_END) * 4));
  K1Buffers v(c, n);
  const uint32_t g = v.g;

  // ---- alphabet: the symbols that occur, in byte order, ceil(log2) bits each ----
  const uint32_t nbytes = sentinel ? n - 1u : n;
  BCE_HIP_TRY(c, hipMemsetAsync(v.word(K1W_HIST), 0, 256 * 4, c->stream));
  hipLaunchKernelGGL(k1_bytehist_kernel, dim3(g < 1024u ? g : 1024u), dim3(K1_T), 0, c->stream, T, nbytes, v.word(K1W_HIST));
  uint32_t hist[256];
  BCE_TRY(read_back(c, hist, v.word(K1W_HIST), sizeof hist));
  uint16_t code[256];
  uint32_t sigma = sentinel ? 1u : 0u;
  for (int b = 0; b < 256; ++b) { code[b] = (uint16_t)sigma; if (hist[b]) ++sigma; }    // (absent bytes: any value, never read)
  uint32_t bits = ceil_log2(sigma);
  if (bits < 1) bits = 1;
  uint32_t nsym = 64u / bits;
  if (nsym > 16u) nsym = 16u;
  // (diagnostic: a narrower first key -- more of the order is left to the segmented rounds; measured at 10^8 B,
  //  text / natural corpus / binary corpus: 64 bits 16.9 / 33.3 / 28.2 ms, 54: 17.8 / 36.1 / 29.1, 48: 18.7 / 35.9 / 28.9,
  //  40: 19.5 / 38.1 / 30.7, 32: 23.3 / 41.9 / 32.7 -- every pass of the wide sort earns more than it costs in K1's
  //  total.  The one-shot route, where only the first sort stands before the coders, may ask for less: want_h)
  const uint32_t most = nsym;
  const uint32_t want_h = want_by_bits && bits <= 8u ? want_by_bits[bits] : 0u;
  if (want_h && want_h < nsym) nsym = want_h;
  c->k1_h_asked = nsym;
  if (const char *e = getenv("BCE_K1_KEYBITS")) { const uint32_t kb = (uint32_t)strtoul(e, nullptr, 10); if (kb >= bits) nsym = kb / bits < most ? kb / bits : most; }
  const uint32_t keybits = nsym * bits;
  const char *ce = getenv("BCE_HIP_CARRY_BYTE");
  const bool carry = may_carry && !sentinel && keybits + 8u <= 64u && !(ce && ce[0] == '0' && !ce[1]);
  const uint32_t first_bit = carry ? 8u : 0u;
  {
    if (!c->h_small) BCE_TRY(pin_alloc(c, &c->h_small, 4096));
    memcpy(c->h_small, code, sizeof code);
    BCE_HIP_TRY(c, hipMemcpyAsync(v.word(K1W_CODE), c->h_small, sizeof code, hipMemcpyHostToDevice, c->stream));
  }

  // ---- first sort: 64-bit keys of nsym symbols ----
  {
    const uint32_t per = K1_T * K1I_E;
    hipLaunchKernelGGL(k1_init64_kernel, dim3((uint32_t)(((uint64_t)n + per - 1) / per)), dim3(K1_T), 0, c->stream, T, n, nbytes,
                       reinterpret_cast<const uint16_t *>(v.word(K1W_CODE)), bits, nsym, carry ? 1u : 0u, v.lo[0], v.hi[0], v.val[0]);
  }
  int res = 0;
  BCE_TRY(radix_sort_wide(c, v.lo, v.hi, v.val, n, first_bit, keybits, &res, 9));     // (9-bit digits: a 10-bit pass costs 1.0 ms at 10^8, a 9-bit one 0.57)
  v.lap("first sort", nsym, n, 0);
  BCE_HIP_TRY(c, hipGetLastError());
  c->k1_res = res;
  c->k1_h = nsym;
  c->k1_carry = carry;
  return BCE_HIP_OK;
}

// Second half: ranks from the sorted keys, then the segmented rounds until nothing is active.  It reorders sa[c->k1_res] inside
// the groups the first half left tied, in place.  c->k1_first_final: the first half had already settled every rotation.
static int k1_finish_wide(bce_hip_ctx *c, uint32_t n) {
  K1View v(c, n);
  BCE_TRY(v.first_ranks());
  c->k1_first_final = v.m == 0 || v.h >= n;      // (no round follows: the order stays as the first sort left it)
  while (v.m > 0 && v.h < n) {
    BCE_TRY(v.segmented_round());
    if (v.nd) BCE_TRY(v.sort_deferred());
    BCE_TRY(v.apply_ranks());
    BCE_TRY(v.relist());
  }
  BCE_HIP_TRY(c, hipGetLastError());
  c->k1_unique = v.m == 0;
  c->sa_res = v.res;
  return BCE_HIP_OK;
}

// Sort the n cyclic rotations of T (sentinel = false), or the n = |T| + 1 rotations of T$ (sentinel = true: T holds n - 1
// bytes).  Leaves the order in c->sa[c->sa_res] and its inverse (the rank of the group head for tied rotations) in c->rank.
static int k1_sort_rotations(bce_hip_ctx *c, const uint8_t *T, uint32_t n, bool sentinel) {
  BCE_TRY(k1_first_sort_wide(c, T, n, sentinel, /*want_by_bits=*/nullptr, /*may_carry=*/false));
  return k1_finish_wide(c, n);
}

// ---- K1 in two halves (api.hip: the one-shot compression starts the enumeration between them) ----------------------------
// Where the rank scatters are the direct ones: not for one byte, not from K1_PART_MIN elements up.
bool k1_two_halves(const bce_hip_ctx *c) {
  return c->n >= 2 && c->n < k1_part_min();
}

static int k1_begin(bce_hip_ctx *c) {
  BCE_TRY(ensure(c, c->bwt, c->n));
  c->stats.sort_rounds = 0;
  c->k1_unique = false;
  c->k1_valid = false;
  c->k1_first_final = false;
  return BCE_HIP_OK;
}

int k1_first_sort(bce_hip_ctx *c, uint32_t *h_symbols, const uint8_t *want_by_bits) {
  BCE_TRY(k1_begin(c));
  BCE_TRY(k1_first_sort_wide(c, c->text.as<uint8_t>(), c->n, false, want_by_bits, /*may_carry=*/true));
  if (h_symbols) *h_symbols = c->k1_h;
  return BCE_HIP_OK;
}

// The BWT of the first sort's order (queued): it differs from the final one only inside groups of rows that share their
// first k1_h bytes.  Where the keys carried the byte it is read off them, in order; a gather from the text otherwise.
int k1_provisional_bwt(bce_hip_ctx *c) {
  const uint32_t n = c->n;
  if (c->k1_carry)
    hipLaunchKernelGGL(k1_bwt_carried_kernel, dim3(grid_for((n >> 2) + 1u)), dim3(K1_T), 0, c->stream, (const uint32_t *)c->key[c->k1_res].as<uint32_t>(), n,
                       c->bwt.as<uint8_t>());
  else hipLaunchKernelGGL(k1_bwt_kernel, dim3(grid_for(n)), dim3(K1_T), 0, c->stream, c->text.as<uint8_t>(), c->sa[c->k1_res].as<uint32_t>(), n,
                     c->bwt.as<uint8_t>());
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

int k1_finish(bce_hip_ctx *c) { return k1_finish_wide(c, c->n); }

// The BWT of the finished order and offset_.  have_bwt: c->bwt already holds it (the provisional one, the first sort having
// settled everything).
int k1_final_bwt(bce_hip_ctx *c, bool have_bwt) {
  const uint32_t n = c->n;
  const uint32_t g = grid_for(n);
  uint32_t *const d_off = k1_word(c, K1W_OFFSET);
  const uint32_t *sa = c->sa[c->sa_res].as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(d_off, 0xFF, 4, c->stream));
  if (!have_bwt) hipLaunchKernelGGL(k1_bwt_kernel, dim3(g), dim3(K1_T), 0, c->stream, c->text.as<uint8_t>(), sa, n, c->bwt.as<uint8_t>());
  hipLaunchKernelGGL(k1_offset_kernel, dim3(g), dim3(K1_T), 0, c->stream, c->rank.as<uint32_t>(), n, d_off);
  uint32_t off = 0;
  BCE_TRY(read_back(c, &off, d_off, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  if (off >= n) { snprintf(c->err, sizeof c->err, "k1: no rank-0 rotation found"); return BCE_HIP_E_INTERNAL; }
  c->offset = off;
  c->k1_valid = true;
  return BCE_HIP_OK;
}

int k1_bwt(bce_hip_ctx *c) {
  const uint32_t n = c->n;
  uint8_t *T = c->text.as<uint8_t>();
  BCE_TRY(k1_begin(c));
  if (n == 1) {
    BCE_HIP_TRY(c, hipMemcpyAsync(c->bwt.p, T, 1, hipMemcpyDeviceToDevice, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->offset = 0;
    return BCE_HIP_OK;
  }
  BCE_TRY(k1_sort_rotations(c, T, n, false));
  return k1_final_bwt(c, false);
}

// ---- the libdivsufsort seam (include/divsufsort_hip.h; bce.cpp:901) -------------------------------------------------------
// divbwt(T, U, A, n): the BWT of T[0, n) with an implicit smallest sentinel -- U[0] = T[n-1], then T[SA[i] - 1] for the
// suffixes in sorted order, the one with SA[i] = 0 left out; returns its 1-based position (the primary index).  Here: the
// rotation sort above on T$ (unique sentinel: rotations compare like suffixes), then one gather.
__global__ __launch_bounds__(K1_T) void k1_divbwt_gather_kernel(const uint8_t *__restrict__ T, const uint32_t *__restrict__ sa,
                                                                uint32_t m, uint32_t pidx, uint8_t *__restrict__ U) {
  for (uint64_t j = (uint64_t)blockIdx.x * K1_T + threadIdx.x; j < m; j += (uint64_t)gridDim.x * K1_T) {
    const uint32_t p = sa[j];                    // sa[0] = m - 1: the rotation that starts with $
    if (p != 0u) U[j < pidx ? j : j - 1u] = T[p - 1u];
  }
}

// What both entries of the seam begin with: the context's compression state is gone -- before the first allocation, which may
// give back its planes and node lists --, T (n bytes of host memory, or of device memory of the context's device) is copied
// into `text`, and the m = n + 1 rotations of T$ are sorted.  with_bwt: c->bwt is sized for them as well.
static int k1_sort_text_sentinel(bce_hip_ctx *c, const uint8_t *T_src, bool src_on_device, uint32_t n, bool with_bwt) {
  if (n == 0 || n >= 0x7FFFFFFFu) return BCE_HIP_E_ARG;
  const uint32_t m = n + 1u;
  c->stage = 0; c->k1_valid = false; c->enum_active = false; c->text_loaded = false;
  BCE_TRY(ensure(c, c->text, m));
  if (with_bwt) BCE_TRY(ensure(c, c->bwt, m));
  uint8_t *T = c->text.as<uint8_t>();
  BCE_HIP_TRY(c, hipMemcpyAsync(T, T_src, n, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  c->stats.sort_rounds = 0;
  return k1_sort_rotations(c, T, m, true);
}

int k1_divbwt(bce_hip_ctx *c, const uint8_t *T_host, uint8_t *U_host, uint32_t n, uint32_t *pidx_out) {
  BCE_TRY(k1_sort_text_sentinel(c, T_host, /*src_on_device=*/false, n, /*with_bwt=*/true));
  const uint32_t m = n + 1u;
  uint32_t pidx = 0;
  BCE_TRY(read_back(c, &pidx, c->rank.as<uint32_t>(), 4));   // row of suffix 0
  if (pidx == 0 || pidx > n) { snprintf(c->err, sizeof c->err, "divbwt: primary index %u out of range", pidx); return BCE_HIP_E_INTERNAL; }
  hipLaunchKernelGGL(k1_divbwt_gather_kernel, dim3(grid_for(m)), dim3(K1_T), 0, c->stream, c->text.as<uint8_t>(), c->sa[c->sa_res].as<uint32_t>(), m,
                     pidx, c->bwt.as<uint8_t>());
  BCE_HIP_TRY(c, hipMemcpyAsync(U_host, c->bwt.p, n, hipMemcpyDeviceToHost, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  *pidx_out = pidx;
  return BCE_HIP_OK;
}

// The same sort with its order kept: rows 1 .. n of sa[sa_res] are the suffix array of T, and with every group a singleton
// rank[i] is the row of suffix i (kd_sufsort.hip: kd_sa_gather).  T_src: n bytes of host memory, or of device memory of the
// context's device, copied into `text` either way.
int k1_suffix_array(bce_hip_ctx *c, const uint8_t *T_src, bool src_on_device, uint32_t n, uint32_t *d_sa, uint32_t *d_isa) {
  BCE_TRY(k1_sort_text_sentinel(c, T_src, src_on_device, n, /*with_bwt=*/false));
  if (!c->k1_unique) { snprintf(c->err, sizeof c->err, "suffix array: the sort left rotations of T$ tied"); return BCE_HIP_E_INTERNAL; }
  BCE_TRY(kd_sa_gather(c, c->sa[c->sa_res].as<uint32_t>(), c->rank.as<uint32_t>(), n, d_sa, d_isa));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
