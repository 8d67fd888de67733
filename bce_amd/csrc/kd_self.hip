// kd_self.hip -- what the indexed text repeats of ITSELF: all nearest smaller values over the suffix array, the longest previous
// factor of every text position, and the greedy LZ77 factorisation built on it (bce_hip_lpf / _lpf_device, bce_hip_self_parse /
// _self_parse_device, the hooks bce_hip_nsv_device and bce_hip_self_parse_of_lpf_device, `bce -gz`, `bce -gzd`).
//
// ANSV.  psv[r] / nsv[r]: the nearest row above / below r whose value is smaller (strictly) than row r's.  Blocks of SLF_BLOCK =
// 2048 rows, an implicit binary min-tree in two storeys (lpf_step.h):
//   tree    one workgroup per block: the rows into LDS, eleven halving levels, the 2047 inner nodes out to global memory (B words
//           per block, word 0 unused) and the block's minimum into the leaves of the top tree.
//   top     one workgroup: the top tree over the NB = 2^ceil(log2(blocks)) minima, level by level, a barrier between two levels.
//   solve   one workgroup per block: its tree back into LDS; every row climbs and descends there (at most 11 + 11 LDS loads a
//           side).  A row without an answer in its block climbs and descends the top tree (at most 2 log2(NB) loads), then descends
//           the found block's tree in global memory (11 loads).  So a row and side costs at most 2 log2(NB) + 11 <= 51 dependent
//           global loads for any input: no lane ever walks a block or a level.
// Extra memory: 4 bytes per row for the blocks' trees (rounded up to whole blocks) and 8 NB bytes for the top tree: 4 n + 8 KB +
// 16 (n / 2048 + 1) bytes at most, below 8 n for every n that has a second block.
// LPF.  solve's second instantiation: the rows are sa[r]; instead of storing psv / nsv it takes sa[] of both, runs rot_lcp twice
// with the bound min(max_len, n - i) and stores lpf and src at the text position i = sa[r] (or at its mirror n - 1 - i, for the
// chain).  Fused: the two row numbers never exist as arrays, which saves 8 n bytes written and read again.
// The chain.  kd_parse's, mirrored (lpf_step.h: self_mirror): lengths, sources and text are written at n - 1 - i, kd_parse runs on
// them unchanged, and its ops and literal bytes are turned round in place.
// No atomics: every value is written by the one lane that owns it.  Everything written is the feature's own (qb::slf_* of c->qbuf,
// and kd_parse's par_* temporaries) or the caller's outputs; sa, the text and the planes are only read.
#include "common.h"
#include "lpf_step.h"
#include "parse_step.h"

namespace bce {

namespace {

constexpr int SLF_T = 256;                   // lanes per workgroup (4 waves)
constexpr int SLF_ITEMS = 8;                 // rows per lane
constexpr uint32_t SLF_BLOCK = SLF_T * SLF_ITEMS;   // 2048

inline uint32_t slf_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + SLF_BLOCK - 1) / SLF_BLOCK); }
inline uint32_t slf_top_leaves(uint32_t nb) { uint32_t p = 1; while (p < nb) p <<= 1; return p; }

// inner: blocks * SLF_BLOCK words; top: 2 NB words, its leaves beyond the blocks prefilled with NSV_PAD
__global__ __launch_bounds__(SLF_T) void nsv_tree_kernel(const uint32_t *__restrict__ vals, uint32_t n, uint32_t *__restrict__ inner,
                                                         uint32_t *__restrict__ top, uint32_t NB) {
  __shared__ uint32_t t[2 * SLF_BLOCK];
  const uint32_t base = blockIdx.x * SLF_BLOCK;
#pragma unroll
  for (int k = 0; k < SLF_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * SLF_T + threadIdx.x;
    t[SLF_BLOCK + i] = i < n - base ? vals[base + i] : NSV_PAD;
  }
  if (threadIdx.x == 0) t[0] = NSV_PAD;
  __syncthreads();
  for (uint32_t w = SLF_BLOCK / 2; w >= 1u; w >>= 1) {
    for (uint32_t k = w + threadIdx.x; k < 2u * w; k += SLF_T) t[k] = nsv_min(t[2u * k], t[2u * k + 1u]);
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < SLF_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * SLF_T + threadIdx.x;
    inner[base + i] = t[i];
  }
  if (threadIdx.x == 0) top[NB + blockIdx.x] = t[1];
}

// one workgroup; every level reads what the level below wrote before the barrier
__global__ __launch_bounds__(SLF_T) void nsv_top_kernel(uint32_t *top, uint32_t NB) {
  for (uint32_t w = NB / 2; w >= 1u; w >>= 1) {
    for (uint32_t k = w + threadIdx.x; k < 2u * w; k += SLF_T) top[k] = nsv_min(top[2u * k], top[2u * k + 1u]);
    __syncthreads();
  }
}

// Lpf == false: psv / nsv of every row.  Lpf == true: vals is the suffix array; lpf / src (src may be null) at the text position,
// or at its mirror where `mirror` is set.
template <bool Lpf>
__global__ __launch_bounds__(SLF_T) void nsv_solve_kernel(const uint32_t *__restrict__ vals, uint32_t n, const uint32_t *__restrict__ inner,
                                                          const uint32_t *__restrict__ top, uint32_t NB, uint32_t *__restrict__ psv,
                                                          uint32_t *__restrict__ nsv, const uint8_t *__restrict__ text, uint32_t max_len,
                                                          uint32_t *__restrict__ lpf, uint32_t *__restrict__ src, bool mirror) {
  __shared__ uint32_t t[2 * SLF_BLOCK];
  const uint32_t base = blockIdx.x * SLF_BLOCK;
#pragma unroll
  for (int k = 0; k < SLF_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * SLF_T + threadIdx.x;
    t[i] = inner[base + i];
    t[SLF_BLOCK + i] = i < n - base ? vals[base + i] : NSV_PAD;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < SLF_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * SLF_T + threadIdx.x, r = base + i;
    if (i >= n - base) break;                                         // (the rows of a lane ascend)
    const uint32_t v = t[SLF_BLOCK + i];
    uint32_t p = nsv_tree_prev(t, SLF_BLOCK, i, v), q = nsv_tree_next(t, SLF_BLOCK, i, v);
    p = p != NSV_NONE ? base + p : nsv_far_prev(top, NB, inner, vals, n, SLF_BLOCK, blockIdx.x, v);
    q = q != NSV_NONE ? base + q : nsv_far_next(top, NB, inner, vals, n, SLF_BLOCK, blockIdx.x, v);
    if (!Lpf) { psv[r] = p; nsv[r] = q; continue; }
    uint32_t s;
    const uint32_t l = lpf_pick(text, n, v, p != NSV_NONE ? vals[p] : NSV_NONE, q != NSV_NONE ? vals[q] : NSV_NONE, max_len, &s);
    const uint32_t at = mirror ? self_mirror(n, v) : v;
    lpf[at] = l;
    if (src) src[at] = s;
  }
}

// out[n - 1 - i] = in[i]
template <class T>
__global__ __launch_bounds__(SLF_T) void self_mirror_kernel(const T *__restrict__ in, T *__restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * SLF_T + threadIdx.x;
  if (i < n) out[self_mirror(n, i)] = in[i];
}
__global__ __launch_bounds__(SLF_T) void self_fill_kernel(uint32_t *__restrict__ out, uint32_t n, uint32_t word) {
  const uint32_t i = blockIdx.x * SLF_T + threadIdx.x;
  if (i < n) out[i] = word;
}

// In place: element k against element count - 1 - k, each pair by the one lane k < count / 2.  ops: pairs of words.
__global__ __launch_bounds__(SLF_T) void self_turn_ops_kernel(uint32_t *__restrict__ ops, uint32_t nops) {
  const uint32_t k = blockIdx.x * SLF_T + threadIdx.x;
  if (k >= nops / 2u) return;
  const size_t a = 2 * (size_t)k, b = 2 * (size_t)self_mirror(nops, k);
  const uint32_t l = ops[a], s = ops[a + 1];
  ops[a] = ops[b]; ops[a + 1] = ops[b + 1];
  ops[b] = l; ops[b + 1] = s;
}
__global__ __launch_bounds__(SLF_T) void self_turn_bytes_kernel(uint8_t *__restrict__ lits, uint32_t nlits) {
  const uint32_t k = blockIdx.x * SLF_T + threadIdx.x;
  if (k >= nlits / 2u) return;
  const uint32_t m = self_mirror(nlits, k);
  const uint8_t x = lits[k];
  lits[k] = lits[m];
  lits[m] = x;
}

inline dim3 slf_grid(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + SLF_T - 1) / SLF_T)); }

}  // namespace

static_assert(SLF_BLOCK == NSV_TREE_BLOCK, "kd_maxrep.hip solves on the same blocks");

// the two storeys over vals[0, n), n >= 1, into slf_tree / slf_top; queued
int nsv_trees(bce_hip_ctx *c, const uint32_t *vals, uint32_t n, uint32_t *NB_out) {
  const uint32_t nb = slf_blocks(n), NB = slf_top_leaves(nb);
  BCE_TRY(ensure(c, c->qbuf[qb::slf_tree], (size_t)nb * SLF_BLOCK * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::slf_top], (size_t)NB * 8));
  uint32_t *inner = c->qbuf[qb::slf_tree].as<uint32_t>(), *top = c->qbuf[qb::slf_top].as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(top, 0xFF, (size_t)NB * 8, c->stream));
  hipLaunchKernelGGL(nsv_tree_kernel, dim3(nb), dim3(SLF_T), 0, c->stream, vals, n, inner, top, NB);
  hipLaunchKernelGGL(nsv_top_kernel, dim3(1), dim3(SLF_T), 0, c->stream, top, NB);
  BCE_HIP_TRY(c, hipGetLastError());
  *NB_out = NB;
  return BCE_HIP_OK;
}

// d_psv[r], d_nsv[r], r < n, of the n >= 1 words d_vals (NSV_NONE: no smaller value on that side).  Queued; the caller waits.
int kd_nsv(bce_hip_ctx *c, const uint32_t *d_vals, uint32_t n, uint32_t *d_psv, uint32_t *d_nsv) {
  uint32_t NB = 0;
  BCE_TRY(nsv_trees(c, d_vals, n, &NB));
  hipLaunchKernelGGL(nsv_solve_kernel<false>, dim3(slf_blocks(n)), dim3(SLF_T), 0, c->stream, d_vals, n, c->qbuf[qb::slf_tree].as<uint32_t>(),
                     c->qbuf[qb::slf_top].as<uint32_t>(), NB, d_psv, d_nsv, nullptr, 0u, nullptr, nullptr, false);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// d_lpf[i] and d_src[i] (unless null) of the context's text, i < n, or both at n - 1 - i (mirror).  sa: K1's suffix array, null for a
// text of one byte, which has no earlier text.  Queued; the caller waits.
int kd_lpf(bce_hip_ctx *c, const uint32_t *sa, uint32_t max_len, bool mirror, uint32_t *d_lpf, uint32_t *d_src) {
  const uint32_t n = c->n;
  if (!sa) {
    hipLaunchKernelGGL(self_fill_kernel, slf_grid(n), dim3(SLF_T), 0, c->stream, d_lpf, n, 0u);
    if (d_src) hipLaunchKernelGGL(self_fill_kernel, slf_grid(n), dim3(SLF_T), 0, c->stream, d_src, n, NSV_NONE);
    BCE_HIP_TRY(c, hipGetLastError());
    return BCE_HIP_OK;
  }
  uint32_t NB = 0;
  BCE_TRY(nsv_trees(c, sa, n, &NB));
  hipLaunchKernelGGL(nsv_solve_kernel<true>, dim3(slf_blocks(n)), dim3(SLF_T), 0, c->stream, sa, n, c->qbuf[qb::slf_tree].as<uint32_t>(),
                     c->qbuf[qb::slf_top].as<uint32_t>(), NB, nullptr, nullptr, c->text.as<uint8_t>(), max_len, d_lpf, d_src, mirror);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// The mirrors of n >= 1 lengths, sources (may be null) and text bytes, into slf_rlen / slf_rsrc / slf_rtext.  Queued.
int kd_self_mirror(bce_hip_ctx *c, const uint32_t *d_lpf, const uint32_t *d_src, const uint8_t *d_text, uint32_t n) {
  BCE_TRY(ensure(c, c->qbuf[qb::slf_rlen], (size_t)n * 4));
  if (d_src) BCE_TRY(ensure(c, c->qbuf[qb::slf_rsrc], (size_t)n * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::slf_rtext], (size_t)n));
  if (d_lpf) hipLaunchKernelGGL(self_mirror_kernel<uint32_t>, slf_grid(n), dim3(SLF_T), 0, c->stream, d_lpf, c->qbuf[qb::slf_rlen].as<uint32_t>(), n);
  if (d_src) hipLaunchKernelGGL(self_mirror_kernel<uint32_t>, slf_grid(n), dim3(SLF_T), 0, c->stream, d_src, c->qbuf[qb::slf_rsrc].as<uint32_t>(), n);
  hipLaunchKernelGGL(self_mirror_kernel<uint8_t>, slf_grid(n), dim3(SLF_T), 0, c->stream, d_text, c->qbuf[qb::slf_rtext].as<uint8_t>(), n);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// The chain over the mirrored arrays in slf_rlen / slf_rsrc (with_src) / slf_rtext: kd_parse as it is, then its ops and literal
// bytes turned round.  sizing, caps, BCE_HIP_E_OVERFLOW and *info as kd_parse.  Complete on return.
int kd_self_parse(bce_hip_ctx *c, uint32_t n, uint32_t min_len, bool with_src, bool sizing, uint32_t *d_ops, uint64_t ops_cap, uint8_t *d_lits,
                  uint64_t lits_cap, bce_hip_parse_info *info) {
  BCE_TRY(kd_parse(c, c->qbuf[qb::slf_rlen].as<uint32_t>(), with_src ? c->qbuf[qb::slf_rsrc].as<uint32_t>() : nullptr,
                   c->qbuf[qb::slf_rtext].as<uint8_t>(), n, min_len, sizing, d_ops, ops_cap, d_lits, lits_cap, info));
  if (sizing) return BCE_HIP_OK;
  const uint32_t nops = (uint32_t)info->nops, nlits = (uint32_t)info->nlits;
  if (nops >= 2u) hipLaunchKernelGGL(self_turn_ops_kernel, slf_grid(nops / 2u), dim3(SLF_T), 0, c->stream, d_ops, nops);
  if (nlits >= 2u) hipLaunchKernelGGL(self_turn_bytes_kernel, slf_grid(nlits / 2u), dim3(SLF_T), 0, c->stream, d_lits, nlits);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
