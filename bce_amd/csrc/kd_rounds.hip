// kd_rounds.hip -- the rounds of the GPU-assisted decoder outside the tail: a round is a query pass (classify every node,
// write the queries of the coded ones in stream order) and, once the host's decoders have answered, a children pass (the
// children and the new boundary rank of every node).  Six launches -- count / scan / write per pass, any number of nodes --
// or two (dec_small_kernel, up to DS_MAXNODES nodes).  The steps of a round are in kd_decode.h; kd_decode.hip drives.
#include "kd_decode.h"

namespace bce {

namespace {

// MODE 0: count the queries of each tile.  1: write them.  2: count the children.  3: write children and ranks.
template <int MODE>
__global__ __launch_bounds__(K3_T) void dec_tiles_kernel(DecArgs a) {
  __shared__ uint32_t tp[9];
  __shared__ uint32_t lds_cnt[K3_NPT][4][3];
  if (a.ctl->err) return;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) dec_tile_prefix(a, tp);
  __syncthreads();
  const uint32_t T = tp[8];
  for (uint32_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
    const uint32_t p = dec_plane_of(tile, tp);
    if (!((a.pmask >> p) & 1u)) continue;                        // (a whole tile: uniform over the block)
    const uint32_t ti = tile - tp[p];
    uint32_t *R = a.R + (size_t)p * ((size_t)a.n + 1);
    const uint32_t zi = a.zeros[p];
    Node nd[K3_NPT];
    DCls cl[K3_NPT];
    uint32_t valid[K3_NPT], isq[K3_NPT], ise[K3_NPT], zero[K3_NPT];
    uint32_t qr[K3_NPT], er[K3_NPT], d2[K3_NPT], tot[3];
    uint32_t bad = dec_load_tile(a, p, ti, R, lds_cnt, nd, cl, valid, isq, ise, zero, qr, er, tot);
    if (bad) a.ctl->err = 1;
    if (MODE == 3 && ((a.ctl->ovf >> p) & 1u)) continue;        // the children do not fit: the host grows the list and runs this again
    if (MODE == 0) {
      if (tid == 0) { a.tilecnt[(size_t)tile * 4 + 2] = tot[0]; a.tilecnt[(size_t)tile * 4 + 3] = tot[1]; }
      continue;
    }
    const uint32_t qb = a.ctl->qbase[p] + a.tileoff[(size_t)tile * 4 + 2];
    if (MODE == 1) {
      const uint32_t eb = a.ctl->ebase[p] + a.tileoff[(size_t)tile * 4 + 3];
#pragma unroll
      for (int it = 0; it < K3_NPT; ++it)
        if (isq[it]) {
          uint32_t word;
          uint4 esc;
          const bool escape = dec_make_query(a.cfg, p, nd[it], cl[it], word, esc);
          a.Q[qb + qr[it]] = word;
          if (escape) {
            if ((uint64_t)eb + er[it] < a.ecap) a.E[eb + er[it]] = esc;
            else a.ctl->err = 1;                                 // (more escapes than disjoint nodes of >= 32 positions: not an archive of ours)
          }
        }
      continue;
    }
    uint32_t has0[K3_NPT], has1[K3_NPT], rval[K3_NPT];
    Node c0[K3_NPT], c1[K3_NPT];
#pragma unroll
    for (int it = 0; it < K3_NPT; ++it) {
      uint32_t v;
      if (dec_take_answer(cl[it], isq[it], isq[it] ? a.res[qb + qr[it]] : 0u, v)) bad = 1;
      rval[it] = dec_children(nd[it], cl[it], v, zi, has0[it], c0[it], has1[it], c1[it]);
      has0[it] &= valid[it];
      has1[it] &= valid[it];
    }
    if (bad) a.ctl->err = 1;
    uint32_t r0[K3_NPT], r1[K3_NPT];
    tile_ranks(has0, has1, zero, lds_cnt, r0, r1, d2, tot);
    if (MODE == 2) {
      if (tid == 0) { a.tilecnt[(size_t)tile * 4 + 0] = tot[0]; a.tilecnt[(size_t)tile * 4 + 1] = tot[1]; }
      continue;
    }
    const uint32_t o0 = a.tileoff[(size_t)tile * 4 + 0], o1 = a.tileoff[(size_t)tile * 4 + 1];
    Node *dst = dec_nodes(a, a.par ^ 1u, (p + 1u) & 7u);
#pragma unroll
    for (int it = 0; it < K3_NPT; ++it) {
      if (has0[it]) dst[o0 + r0[it]] = c0[it];
      if (has1[it]) dst[a.cap[a.par ^ 1u][(p + 1u) & 7u] - 1u - (o1 + r1[it])] = c1[it];
      if (valid[it] && !cl[it].bad) R[nd[it].s + nd[it].x0] = rval[it];        // ranks[i].set(s + _x0, s1 + _1x0) :1277,1285,1350
    }
  }
}

// Per-plane exclusive scan of the tile counts (block p = plane p) and the round's bookkeeping by the block that
// finishes last.  QUERY: queries -> tileoff[.][2], query bases, DecInfo for the host.  !QUERY: children ->
// tileoff[.][0..1], next round's list sizes.
template <bool QUERY>
__global__ __launch_bounds__(1024) void dec_scan_kernel(DecArgs a) {
  __shared__ uint32_t tp[9];
  __shared__ uint32_t s_last;
  DecCtl *ctl = a.ctl;
  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  if (!((a.pmask >> p) & 1u)) return;                            // (the whole block)
  if (tid == 0) dec_tile_prefix(a, tp);
  __syncthreads();
  constexpr int K = QUERY ? 2 : 0;                               // the pair of tile counts this pass scans: [2], [3] or [0], [1]
  uint32_t r0 = 0, r1 = 0;
  if (!ctl->err) {
    for (uint32_t base = tp[p]; base < tp[p + 1]; base += 1024) {
      const uint32_t t = base + tid;
      const bool valid = t < tp[p + 1];
      const uint32_t v0 = valid ? a.tilecnt[(size_t)t * 4 + K] : 0u, v1 = valid ? a.tilecnt[(size_t)t * 4 + K + 1] : 0u;
      uint64_t tot;
      const uint64_t ex = block_excl_scan_sum64<1024>((uint64_t)v0 | ((uint64_t)v1 << 32), &tot);
      if (valid) {
        a.tileoff[(size_t)t * 4 + K] = r0 + (uint32_t)ex;
        a.tileoff[(size_t)t * 4 + K + 1] = r1 + (uint32_t)(ex >> 32);
      }
      r0 += (uint32_t)tot; r1 += (uint32_t)(tot >> 32);
    }
  }
  if (tid == 0) {
    ctl->ptot[p][K] = r0; ctl->ptot[p][K + 1] = r1;
    __threadfence();
    s_last = atomicAdd(&ctl->ticket, 1u) == (uint32_t)__popc(a.pmask) - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last || tid != 0) return;
  __threadfence();
  ctl->ticket = 0;
  const volatile uint32_t (*pt)[4] = ctl->ptot;
  const uint64_t curn = dec_round_nodes(ctl, a.par);
  if (QUERY) {
    uint32_t acc = 0, eacc = 0;
    for (int i = 0; i < 8; ++i) {                                 // (planes of an earlier part of this round lie first: their totals stand)
      const uint32_t q = (a.order >> (4 * i)) & 7u;
      if ((a.pmask >> q) & 1u) dec_publish_queries(a, q, acc, eacc, pt[q][2], pt[q][3]);
      if ((a.gmask >> q) & 1u) { acc += pt[q][2]; eacc += pt[q][3]; }   // (32 bits: a group's queries are bounded, see DecArgs::gmask)
    }
    dec_publish_info(a, curn);
  } else {
    uint64_t nextn = 0;
    uint32_t ovf = 0;
    for (uint32_t q = 0; q < 8; ++q) {
      if (((a.pmask >> q) & 1u) && dec_publish_children(a, q, pt[q][0], pt[q][1])) ovf |= 1u << q;
      nextn += (uint64_t)pt[q][0] + pt[q][1];
    }
    ctl->ovf |= ovf;
    if (a.final) {                                               // (every plane's totals are this round's by now)
      ctl->nodes_total += curn;
      ctl->next_nodes = nextn;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Rounds of up to ~2 M nodes in TWO launches instead of six (round 3).  Between the first wide rounds and the tail lie
// thousands of rounds of 2 K .. 1 M nodes (natural corpus: 4 900, binary corpus: 4 100) in which count / scan / write
// kernels of ~10 us each, three times per round, are pure launch overhead.  Here a pass is ONE kernel, as in
// k3_small_kernel: block = tile, classified once; the tile's counts go out in a 64-bit word tagged with the pass number
// (nothing to reset), the block waits for the words of the earlier tiles (all of them for the query offsets, those of
// its plane for the children), sums them and writes; the block of the last tile folds the words into the control block
// and the host's DecInfo.  A waiter only waits for smaller block indices (in-order dispatch, as k3_small_kernel); the
// wait is bounded and ends in err = 4 instead of a hang.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ds_ld(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t ds_wait(const unsigned long long *p, uint64_t epoch, uint64_t w, DecCtl *ctl) {
  uint32_t spins = 0;
  while ((w >> 33) != epoch) {
    __builtin_amdgcn_s_sleep(1);
    w = ds_ld(p);
    if (++spins == (1u << 22)) { ctl->err = 4; return epoch << 33; }
  }
  return w;
}
template <bool QUERY>
__global__ __launch_bounds__(K3_T) void dec_small_kernel(DecArgs a) {
  __shared__ uint32_t tp[9];
  __shared__ uint32_t lds_cnt[K3_NPT][4][3];
  __shared__ unsigned long long s_acc[2];
  __shared__ unsigned long long s_tot[8];
  DecCtl *ctl = a.ctl;
  if (ctl->err) return;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) dec_tile_prefix(a, tp);
  if (tid < 2) s_acc[tid] = 0;
  if (tid < 8) s_tot[tid] = 0;
  __syncthreads();
  const uint32_t T = tp[8], tile = blockIdx.x;
  if (tile >= T) return;
  const uint64_t epoch = ((uint64_t)a.round * 2u + (QUERY ? 1u : 2u)) & 0x7FFFFFFFull;
  const uint32_t p = dec_plane_of(tile, tp);
  const uint32_t ti = tile - tp[p];
  uint32_t *R = a.R + (size_t)p * ((size_t)a.n + 1);
  const uint32_t zi = a.zeros[p];
  Node nd[K3_NPT];
  DCls cl[K3_NPT];
  uint32_t valid[K3_NPT], isq[K3_NPT], ise[K3_NPT], zero[K3_NPT];
  uint32_t qr[K3_NPT], er[K3_NPT], d2[K3_NPT], tot[3];
  uint32_t bad = dec_load_tile(a, p, ti, R, lds_cnt, nd, cl, valid, isq, ise, zero, qr, er, tot);
  uint32_t has0[K3_NPT], has1[K3_NPT], rval[K3_NPT], r0[K3_NPT], r1[K3_NPT];
  Node c0[K3_NPT], c1[K3_NPT];
  uint32_t qb = 0;
  if (!QUERY) {
    qb = a.tileoff[(size_t)tile * 4 + 2];                      // (left there by the query pass of this round)
#pragma unroll
    for (int it = 0; it < K3_NPT; ++it) {
      uint32_t v;
      if (dec_take_answer(cl[it], isq[it], isq[it] ? a.res[qb + qr[it]] : 0u, v)) bad = 1;
      rval[it] = dec_children(nd[it], cl[it], v, zi, has0[it], c0[it], has1[it], c1[it]);
      has0[it] &= valid[it];
      has1[it] &= valid[it];
    }
    tile_ranks(has0, has1, zero, lds_cnt, r0, r1, d2, tot);
  }
  if (bad) { ctl->err = 1; __threadfence(); }
  // [10:0] first count, [21:11] second (queries / escapes, or child0 / child1: <= 1024 each), [63:33] pass tag
  if (tid == 0)
    __hip_atomic_store(&a.words[tile], (epoch << 33) | ((uint64_t)tot[1] << 11) | (uint64_t)tot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // look back: the query pass needs every earlier tile (the query buffer runs through the planes), the children pass
  // the earlier tiles of its own plane
  {
    constexpr int LB = (int)(DS_MAXTILES / K3_T);
    const uint32_t first = QUERY ? 0u : tp[p];
    uint64_t wv[LB], s0 = 0, s1 = 0;
#pragma unroll
    for (int q = 0; q < LB; ++q) { const uint32_t j = tid + (uint32_t)q * K3_T; wv[q] = (j >= first && j < tile) ? ds_ld(&a.words[j]) : 0ull; }
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const uint32_t j = tid + (uint32_t)q * K3_T;
      if (j >= first && j < tile) {
        wv[q] = ds_wait(&a.words[j], epoch, wv[q], ctl);
        s0 += wv[q] & 0x7FFu; s1 += (wv[q] >> 11) & 0x7FFu;
      }
    }
    if (s0) atomicAdd(&s_acc[0], (unsigned long long)s0);
    if (s1) atomicAdd(&s_acc[1], (unsigned long long)s1);
  }
  __syncthreads();
  const uint32_t o0 = (uint32_t)s_acc[0], o1 = (uint32_t)s_acc[1];
  if (QUERY) {
    if (tid == 0) a.tileoff[(size_t)tile * 4 + 2] = o0;
#pragma unroll
    for (int it = 0; it < K3_NPT; ++it)
      if (isq[it]) {
        uint32_t word;
        uint4 esc;
        const bool escape = dec_make_query(a.cfg, p, nd[it], cl[it], word, esc);
        a.Q[o0 + qr[it]] = word;
        if (escape) a.E[o1 + er[it]] = esc;
      }
  } else {
    Node *dst = dec_nodes(a, a.par ^ 1u, (p + 1u) & 7u);
    const uint32_t dcap = a.cap[a.par ^ 1u][(p + 1u) & 7u];
#pragma unroll
    for (int it = 0; it < K3_NPT; ++it) {
      // (the host runs this kernel only where twice the round's nodes fit every list: the bounds never bite)
      if (has0[it] && o0 + r0[it] < dcap) dst[o0 + r0[it]] = c0[it];
      if (has1[it] && o1 + r1[it] < dcap) dst[dcap - 1u - (o1 + r1[it])] = c1[it];
      if (valid[it] && !cl[it].bad) R[nd[it].s + nd[it].x0] = rval[it];
    }
  }
  // ---- the block of the last tile folds the pass into the control block (and the host's DecInfo) ----
  if (tile != T - 1u) return;
  {
    constexpr int LB = (int)(DS_MAXTILES / K3_T);
    uint64_t wv[LB];
#pragma unroll
    for (int q = 0; q < LB; ++q) { const uint32_t j = tid + (uint32_t)q * K3_T; wv[q] = j < T ? ds_ld(&a.words[j]) : 0ull; }
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const uint32_t j = tid + (uint32_t)q * K3_T;
      if (j < T) {
        const uint32_t pj = dec_plane_of(j, tp);
        wv[q] = ds_wait(&a.words[j], epoch, wv[q], ctl);
        atomicAdd(&s_tot[pj], (unsigned long long)((wv[q] & 0x7FFu) | (((wv[q] >> 11) & 0x7FFu) << 32)));
      }
    }
  }
  __syncthreads();
  if (tid != 0) return;
  const uint64_t curn = dec_round_nodes(ctl, a.par);
  if (QUERY) {
    uint32_t acc = 0, eacc = 0;
    for (uint32_t q = 0; q < 8; ++q) {
      const uint32_t tq = (uint32_t)s_tot[q], te = (uint32_t)(s_tot[q] >> 32);
      dec_publish_queries(a, q, acc, eacc, tq, te);
      acc += tq; eacc += te;
    }
    dec_publish_info(a, curn);
  } else {
    uint64_t nextn = 0;
    bool ovf = false;
    for (uint32_t q = 0; q < 8; ++q) {
      const uint32_t t0 = (uint32_t)s_tot[q], t1 = (uint32_t)(s_tot[q] >> 32);
      if (dec_publish_children(a, q, t0, t1)) ovf = true;
      nextn += (uint64_t)t0 + t1;
    }
    if (ovf && !ctl->err) ctl->err = 2;
    ctl->nodes_total += curn;
    ctl->next_nodes = nextn;
  }
}

}  // namespace

void dec_query_pass(hipStream_t stream, const DecArgs &a, uint32_t grid) {       // the queries of the planes in a.pmask
  hipLaunchKernelGGL((dec_tiles_kernel<0>), dim3(grid), dim3(K3_T), 0, stream, a);
  hipLaunchKernelGGL((dec_scan_kernel<true>), dim3(8), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL((dec_tiles_kernel<1>), dim3(grid), dim3(K3_T), 0, stream, a);
}
void dec_children_pass(hipStream_t stream, const DecArgs &a, uint32_t grid) {    // ... and their children and new boundary ranks
  hipLaunchKernelGGL((dec_tiles_kernel<2>), dim3(grid), dim3(K3_T), 0, stream, a);
  hipLaunchKernelGGL((dec_scan_kernel<false>), dim3(8), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL((dec_tiles_kernel<3>), dim3(grid), dim3(K3_T), 0, stream, a);
}
void dec_small_query_pass(hipStream_t stream, const DecArgs &a, uint32_t grid) {
  hipLaunchKernelGGL((dec_small_kernel<true>), dim3(grid), dim3(K3_T), 0, stream, a);
}
void dec_small_children_pass(hipStream_t stream, const DecArgs &a, uint32_t grid) {
  hipLaunchKernelGGL((dec_small_kernel<false>), dim3(grid), dim3(K3_T), 0, stream, a);
}

}  // namespace bce
