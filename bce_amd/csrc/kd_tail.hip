// kd_tail.hip -- the resident tail kernels of the GPU-assisted decoder.
// Deep tails.  A long repeat is a chain of forced nodes (all zeros / all ones / forced split): thousands to
// millions of rounds in which no decoder is asked anything.  One persistent workgroup keeps the lists in LDS and
// runs those rounds on the device (classify from R, children, the new ranks), and stops IN FRONT of the first
// round that holds a query nobody answers, does not fit, or is empty; the host then runs that round the normal way.
// What a launch did goes back in a TailReport (kd_decode.h); Decode::tail_kernels (kd_decode.hip) reads it.
#include "kd_decode.h"

namespace bce {

namespace {

// ---- what both kernels do on their way out (one lane) ----
__device__ __forceinline__ void tail_leave(const DecArgs &a, TailReport *report, TailReport r) {
  report->executed = r.executed; report->why = r.why; report->pending = r.pending; report->seq = r.seq; report->answered = r.answered;
  __threadfence_system();
  if (a.mbox) __hip_atomic_store(&a.mbox[2], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The launch cannot run a single round (nothing there, an error pending, or `outgrown`: more nodes than the kernel holds):
// nothing is touched, and answers the launch was given stay in hand.
__device__ __forceinline__ void tail_refuse(const DecArgs &a, TailReport *report, bool outgrown, uint32_t resume) {
  tail_leave(a, report, TailReport{0u, outgrown ? kTailOutgrown : kTailDone, 0u, a.seq_base, resume & kTailHaveAnswers});
}
// The closing report, after the lists and their counts have gone back: `total` nodes are left for the next round.
__device__ __forceinline__ void tail_report(const DecArgs &a, TailReport *report, uint64_t nodes_total, uint32_t total, TailReport r) {
  a.ctl->nodes_total = nodes_total;
  a.ctl->next_nodes = total;
  tail_leave(a, report, r);
}
// Stay resident over a query round (one lane; the queries and `info` are out and fenced): publish the round's number, wait for
// the host to post the same number back -- it polls the mailbox while the kernel runs -- for at most ~2 ms (wall_clock64: 100 MHz).
// False: nobody answered; the kernel leaves as it does without a mailbox, the host answers and launches again.
__device__ __forceinline__ bool tail_mbox_wait(uint32_t *mbox, uint32_t seq) {
  __hip_atomic_store(&mbox[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  const uint64_t t0 = wall_clock64();
  for (;;) {
    if (__hip_atomic_load(&mbox[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == seq) return true;
    if (wall_clock64() - t0 > 200000ull) return false;
    __builtin_amdgcn_s_sleep(4);
  }
}
// An answer: host memory, possibly written while the kernel runs
__device__ __forceinline__ uint32_t tail_answer(const DecArgs &a, uint32_t i) {
  return __hip_atomic_load(const_cast<uint32_t *>(&a.res[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Up to DT_CAP nodes, all planes together, in LDS.  resume & kTailHaveAnswers: the first round is the one a previous launch
// stopped at; its queries were answered by the host (a.res, in the order they were emitted).  At a round with queries the
// kernel EMITS them (a.Q / a.E / a.info, all host-visible) and waits at the mailbox, so that a query round costs no launch;
// without a mailbox, or when nobody answers in time, it leaves with kTailQuery and one launch + one sync is all the round
// costs.  It stops with kTailOutgrown if the children are more than DT_CAP (nothing of that round is written), kTailBad on
// an inconsistent node or answer, kTailDone when nothing is left, max_rounds have run, or (kTailLeaveWhenFew) a round is
// down to 64 nodes.
__global__ __launch_bounds__(DT_T) void dec_tail_kernel(DecArgs a, uint32_t max_rounds, TailReport *report, uint32_t resume) {
  __shared__ Node buf[2][DT_CAP];
  __shared__ uint32_t cnt[2][8][2];
  __shared__ uint32_t off[9], noff[9];
  __shared__ uint64_t ws[DT_T / 64];
  __shared__ uint64_t pstart[9];
  DecCtl *ctl = a.ctl;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  uint32_t par = a.par, cur = 0, executed = 0;
  if (tid < 16) cnt[par][tid >> 1][tid & 1] = ctl->cnt[par][tid >> 1][tid & 1];
  __syncthreads();
  if (tid == 0) {
    uint32_t acc = 0;
    for (int p = 0; p < 8; ++p) { off[p] = acc; acc += cnt[par][p][0] + cnt[par][p][1]; }
    off[8] = acc;
  }
  __syncthreads();
  uint32_t total = off[8];
  if (total > DT_CAP || total == 0 || ctl->err) {
    if (tid == 0) tail_refuse(a, report, total > DT_CAP, resume);
    return;
  }
  for (uint32_t q = tid; q < total; q += DT_T) {
    const uint32_t p = dec_plane_of(q, off);
    buf[0][q] = dec_nodes(a, par, p)[dec_list_index(q - off[p], cnt[par][p][0], a.cap[par][p])];
  }
  uint64_t nodes_total = ctl->nodes_total;
  uint32_t why = kTailDone;
  uint32_t seq = a.seq_base, pending = 0;                     // query rounds are numbered (see DecArgs::mbox)
  bool have_ans = (resume & kTailHaveAnswers) != 0;           // the answers of the round about to run are in res
  __shared__ uint32_t got_flag;
  __syncthreads();
  for (;;) {
    if (total == 0 || executed >= max_rounds) break;
    if ((resume & kTailLeaveWhenFew) && executed && total <= 64) break;    // few nodes again: the wave kernel is three times faster per round
    Node nd[DT_NPT];
    DCls cl[DT_NPT];
    uint32_t pl[DT_NPT];
    bool valid[DT_NPT];
    int stop = 0, badn = 0;
    uint64_t qmine = 0;                                       // queries | escape queries << 32 among my nodes
#pragma unroll
    for (int it = 0; it < DT_NPT; ++it) {
      const uint32_t q = tid * DT_NPT + (uint32_t)it;
      valid[it] = q < total;
      nd[it] = valid[it] ? buf[cur][q] : Node{0u, 1u, 1u};
      pl[it] = valid[it] ? dec_plane_of(q, off) : 0u;
      cl[it] = dec_classify(nd[it], a.R + (size_t)pl[it] * ((size_t)a.n + 1), a.n);
      if (valid[it] && cl[it].bad) badn = 1;
      if (valid[it] && cl[it].kind == 3u) {
        stop = 1;
        qmine += 1ull | ((cl[it].mx - cl[it].mn + 1u > (uint32_t)kMaxK) ? (1ull << 32) : 0ull);
      }
    }
    if (__syncthreads_or(badn)) { why = kTailBad; break; }
    const bool answered = have_ans;                          // this round's queries came back from the host
    uint32_t qx = 0;                                         // exclusive query rank of my first node (list order = stream order)
    if (__syncthreads_or(stop)) {
      // exclusive scan of (queries | escapes << 32) in list order, and the per-plane starts
      uint64_t qinc = wave_incl_sum64(qmine);
      if (lane == 63) ws[wid] = qinc;
      __syncthreads();
      uint64_t qbase = 0, qtot = 0;
#pragma unroll
      for (int i = 0; i < DT_T / 64; ++i) { const uint64_t t = ws[i]; if ((uint32_t)i < wid) qbase += t; qtot += t; }
      const uint64_t qex = qbase + qinc - qmine;
      __syncthreads();
      qx = (uint32_t)qex;
      if (!answered) {
        // emit the round's queries for the host; the lists stay as they are
        if (tid < 9) pstart[tid] = qtot;
        __syncthreads();
        {
          uint64_t run = qex;
#pragma unroll
          for (int it = 0; it < DT_NPT; ++it) {
            const uint32_t q = tid * DT_NPT + (uint32_t)it;
            if (valid[it] && q == off[pl[it]]) pstart[pl[it]] = run;
            if (valid[it] && cl[it].kind == 3u) {
              uint32_t word;
              uint4 esc;
              const bool escape = dec_make_query(a.cfg, pl[it], nd[it], cl[it], word, esc);
              a.Q[(uint32_t)run] = word;
              if (escape) a.E[(uint32_t)(run >> 32)] = esc;
              run += escape ? 1ull | (1ull << 32) : 1ull;
            }
          }
        }
        __syncthreads();
        if (tid == 0) {
          for (int p = 7; p >= 0; --p) if (off[p] == off[p + 1]) pstart[p] = pstart[p + 1];
          for (int p = 0; p < 8; ++p) {
            a.info->qbase[p] = (uint32_t)pstart[p];
            a.info->qtot[p] = (uint32_t)(pstart[p + 1] - pstart[p]);
            a.info->ebase[p] = (uint32_t)(pstart[p] >> 32);
            a.info->etot[p] = (uint32_t)((pstart[p + 1] - pstart[p]) >> 32);
          }
          a.info->cur_nodes = total;
          a.info->err = 0;
        }
        pending = seq;
        bool got = false;
        if (a.mbox) {                                          // stay resident: thread 0 waits, the flag in LDS tells the others
          __threadfence_system();
          __syncthreads();
          if (tid == 0) got_flag = tail_mbox_wait(a.mbox, seq) ? 1u : 0u;
          __syncthreads();
          got = got_flag != 0;
          __atomic_thread_fence(__ATOMIC_ACQUIRE);
        }
        if (!got) { why = kTailQuery; break; }
        ++seq; pending = 0; have_ans = true;
      }
    }
    uint32_t has0[DT_NPT], has1[DT_NPT], rval[DT_NPT];
    Node c0[DT_NPT], c1[DT_NPT];
    uint64_t mine = 0;
    int over = 0;
#pragma unroll
    for (int it = 0; it < DT_NPT; ++it) {
      const bool isq = valid[it] && cl[it].kind == 3u;
      uint32_t v, ans = 0;
      if (isq) { ans = tail_answer(a, qx); ++qx; }
      if (dec_take_answer(cl[it], isq, ans, v)) over = 1;
      rval[it] = dec_children(nd[it], cl[it], v, a.zeros[pl[it]], has0[it], c0[it], has1[it], c1[it]);
      if (!valid[it]) has0[it] = has1[it] = 0;
      mine += (uint64_t)has0[it] | ((uint64_t)has1[it] << 32);
    }
    if (__syncthreads_or(over)) { why = kTailBad; break; }   // an answer outside [mn, mx]: inconsistent archive
    // block exclusive scan of (child0 | child1 << 32) in list order
    uint64_t inc = wave_incl_sum64(mine);
    if (lane == 63) ws[wid] = inc;
    __syncthreads();
    uint64_t wbase = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < DT_T / 64; ++i) { const uint64_t t = ws[i]; if ((uint32_t)i < wid) wbase += t; tot += t; }
    const uint64_t ex = wbase + inc - mine;
    if (tid < 9) pstart[tid] = tot;
    __syncthreads();
    {
      uint64_t run = ex;
#pragma unroll
      for (int it = 0; it < DT_NPT; ++it) {
        const uint32_t q = tid * DT_NPT + (uint32_t)it;
        if (valid[it] && q == off[pl[it]]) pstart[pl[it]] = run;
        run += (uint64_t)has0[it] | ((uint64_t)has1[it] << 32);
      }
    }
    __syncthreads();
    if (tid == 0) {
      for (int p = 7; p >= 0; --p) if (off[p] == off[p + 1]) pstart[p] = pstart[p + 1];
      uint32_t acc = 0;
      for (int pn = 0; pn < 8; ++pn) {
        const int p = (pn + 7) & 7;
        const uint64_t d = pstart[p + 1] - pstart[p];
        cnt[par ^ 1u][pn][0] = (uint32_t)d;
        cnt[par ^ 1u][pn][1] = (uint32_t)(d >> 32);
        noff[pn] = acc;
        acc += (uint32_t)d + (uint32_t)(d >> 32);
      }
      noff[8] = acc;
    }
    __syncthreads();
    if (noff[8] > DT_CAP) { why = kTailOutgrown; break; }   // nothing of this round has been written yet
    {
      uint64_t run = ex;
#pragma unroll
      for (int it = 0; it < DT_NPT; ++it) {
        if (valid[it]) {
          const uint32_t p = pl[it], pn = (p + 1u) & 7u;
          const uint64_t rel = run - pstart[p];
          if (has0[it]) buf[cur ^ 1u][noff[pn] + (uint32_t)rel] = c0[it];
          if (has1[it]) buf[cur ^ 1u][noff[pn] + cnt[par ^ 1u][pn][0] + (uint32_t)(rel >> 32)] = c1[it];
          (a.R + (size_t)p * ((size_t)a.n + 1))[nd[it].s + nd[it].x0] = rval[it];
        }
        run += (uint64_t)has0[it] | ((uint64_t)has1[it] << 32);
      }
    }
    nodes_total += total;
    __syncthreads();                                         // also orders the R stores before the next round's loads
    if (tid < 9) off[tid] = noff[tid];
    __syncthreads();
    total = off[8];
    par ^= 1u; cur ^= 1u; ++executed; have_ans = false;
  }
  __syncthreads();
  for (uint32_t q = tid; q < total; q += DT_T) {
    const uint32_t p = dec_plane_of(q, off);
    dec_nodes(a, par, p)[dec_list_index(q - off[p], cnt[par][p][0], a.cap[par][p])] = buf[cur][q];
  }
  if (tid < 16) ctl->cnt[par][tid >> 1][tid & 1] = cnt[par][tid >> 1][tid & 1];
  if (tid == 0) tail_report(a, report, nodes_total, total, TailReport{executed, why, pending, seq, have_ans ? 1u : 0u});
}

// The same for at most 64 nodes (the very deep tails: a handful of chains): ONE wave, one node per lane, the new
// order from ballots instead of a block scan -- no workgroup barriers on the round's critical path.
// Like dec_tail_kernel it emits the queries of the round it stops at, waits at the mailbox, and resumes with the answers
// (kTailHaveAnswers).  It stops with kTailQuery when nobody answers, kTailOutgrown at more than 64 children (nothing of that
// round is written), kTailBad on an inconsistent node or answer, kTailDone when nothing is left or max_rounds have run.
__global__ __launch_bounds__(64) void dec_tail64_kernel(DecArgs a, uint32_t max_rounds, TailReport *report, uint32_t resume) {
  __shared__ Node nbuf[64];
  __shared__ uint32_t pbuf[64];
  DecCtl *ctl = a.ctl;
  const uint32_t lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t par = a.par, executed = 0, why = kTailDone;
  uint32_t cnt[8][2], total = 0;
#pragma unroll
  for (int p = 0; p < 8; ++p) { cnt[p][0] = ctl->cnt[par][p][0]; cnt[p][1] = ctl->cnt[par][p][1]; total += cnt[p][0] + cnt[p][1]; }
  if (total > 64 || total == 0 || ctl->err) {
    if (lane == 0) tail_refuse(a, report, total > 64, resume);
    return;
  }
  Node nd{0u, 1u, 1u};
  uint32_t pl = 0;
  {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p) {
      const uint32_t m = cnt[p][0] + cnt[p][1];
      if (lane >= acc && lane < acc + m) {
        nd = dec_nodes(a, par, p)[dec_list_index(lane - acc, cnt[p][0], a.cap[par][p])];
        pl = p;
      }
      acc += m;
    }
  }
  uint64_t nodes_total = ctl->nodes_total;
  uint32_t seq = a.seq_base, pending = 0;                     // query rounds are numbered; `pending` = the one I left at
  bool have_ans = (resume & kTailHaveAnswers) != 0;           // the answers of the round about to run are in res
  for (;;) {
    if (total == 0 || executed >= max_rounds) break;
    const bool valid = lane < total;
    const DCls cl = dec_classify(nd, a.R + (size_t)pl * ((size_t)a.n + 1), a.n);
    if (__ballot(valid && cl.bad)) { why = kTailBad; break; }
    const bool isq = valid && cl.kind == 3u;
    const bool ise = isq && cl.mx - cl.mn + 1u > (uint32_t)kMaxK;
    const uint64_t mq = __ballot(isq), me = __ballot(ise);
    const uint32_t qidx = (uint32_t)__popcll(mq & below), eidx = (uint32_t)__popcll(me & below);   // lane order = stream order
    const bool answered = have_ans;                            // this round's queries came back from the host
    if (mq && !answered) {
      // emit the round's queries (host-visible buffers); the lists stay as they are
      if (isq) {
        uint32_t word;
        uint4 esc;
        const bool escape = dec_make_query(a.cfg, pl, nd, cl, word, esc);
        a.Q[qidx] = word;
        if (escape) a.E[eidx] = esc;
      }
#pragma unroll
      for (uint32_t p = 0; p < 8; ++p) {
        const uint64_t pm = __ballot(valid && pl == p);
        const uint64_t lowp = pm ? (pm & (0ull - pm)) - 1ull : 0ull;         // lanes before plane p's first node (an empty plane: base 0)
        if (lane == p) {
          a.info->qbase[p] = (uint32_t)__popcll(mq & lowp);
          a.info->qtot[p] = (uint32_t)__popcll(mq & pm);
          a.info->ebase[p] = (uint32_t)__popcll(me & lowp);
          a.info->etot[p] = (uint32_t)__popcll(me & pm);
        }
      }
      if (lane == 0) { a.info->cur_nodes = total; a.info->err = 0; }
      pending = seq;
      bool got = false;
      if (a.mbox) {                                            // stay resident: lane 0 waits, the others learn the verdict from it
        __threadfence_system();
        uint32_t g = 0;
        if (lane == 0) g = tail_mbox_wait(a.mbox, seq) ? 1u : 0u;
        got = __builtin_amdgcn_readfirstlane((int)g) != 0;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
      }
      if (!got) { why = kTailQuery; break; }
      ++seq; pending = 0; have_ans = true;
    }
    uint32_t has0, has1;
    Node c0, c1;
    uint32_t v;
    if (__ballot(dec_take_answer(cl, isq, isq ? tail_answer(a, qidx) : 0u, v))) { why = kTailBad; break; }   // an answer outside [mn, mx]: inconsistent archive
    const uint32_t rval = dec_children(nd, cl, v, a.zeros[pl], has0, c0, has1, c1);
    if (!valid) has0 = has1 = 0;
    const uint64_t m0 = __ballot(has0), m1 = __ballot(has1);
    if (__popcll(m0) + __popcll(m1) > 64) { why = kTailOutgrown; break; }
    // next lists: plane pn takes the children of plane pn - 1: child0s in order, then child1s in order
    uint32_t base = 0, my0 = 0, my1 = 0, ncnt[8][2];
#pragma unroll
    for (uint32_t pn = 0; pn < 8; ++pn) {
      const uint32_t p = (pn + 7u) & 7u;
      const uint64_t pm = __ballot(valid && pl == p);
      const uint32_t t0 = (uint32_t)__popcll(m0 & pm), t1 = (uint32_t)__popcll(m1 & pm);
      if (pl == p) {
        my0 = base + (uint32_t)__popcll(m0 & pm & below);
        my1 = base + t0 + (uint32_t)__popcll(m1 & pm & below);
      }
      ncnt[pn][0] = t0; ncnt[pn][1] = t1;
      base += t0 + t1;
    }
    if (has0) { nbuf[my0] = c0; pbuf[my0] = (pl + 1u) & 7u; }
    if (has1) { nbuf[my1] = c1; pbuf[my1] = (pl + 1u) & 7u; }
    if (valid) (a.R + (size_t)pl * ((size_t)a.n + 1))[nd.s + nd.x0] = rval;
    nodes_total += total;
    __syncthreads();                                         // one wave: orders LDS and the R stores before the next loads
    total = base;
    nd = lane < total ? nbuf[lane] : Node{0u, 1u, 1u};
    pl = lane < total ? pbuf[lane] : 0u;
#pragma unroll
    for (int p = 0; p < 8; ++p) { cnt[p][0] = ncnt[p][0]; cnt[p][1] = ncnt[p][1]; }
    __syncthreads();
    par ^= 1u; ++executed; have_ans = false;
  }
  // hand the state back
  {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p) {
      const uint32_t m = cnt[p][0] + cnt[p][1];
      if (lane >= acc && lane < acc + m && lane < total)
        dec_nodes(a, par, p)[dec_list_index(lane - acc, cnt[p][0], a.cap[par][p])] = nd;
      acc += m;
    }
  }
  if (lane < 16) ctl->cnt[par][lane >> 1][lane & 1] = cnt[lane >> 1][lane & 1];
  if (lane == 0) tail_report(a, report, nodes_total, total, TailReport{executed, why, pending, seq, have_ans ? 1u : 0u});
}

}  // namespace

void dec_tail_launch(bce_hip_ctx *c, const DecArgs &a, bool wave, uint32_t max_rounds, TailReport *report, uint32_t resume) {
  if (wave) hipLaunchKernelGGL(dec_tail64_kernel, dim3(1), dim3(64), 0, c->stream, a, max_rounds, report, resume);
  else hipLaunchKernelGGL(dec_tail_kernel, dim3(1), dim3(DT_T), 0, c->stream, a, max_rounds, report, resume);
}

}  // namespace bce
