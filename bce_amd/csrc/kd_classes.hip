// kd_classes.hip -- how often, and where, patterns of byte CLASSES occur in the circular text: every position of a pattern is a set
// of bytes (a wildcard, a range, both cases of a letter), from the K2 planes and K1's suffix array (bce_hip_count_classes /
// _locate_classes and their _device forms, `bce -ge` / `-gel`).
//
// The search is class_step.h's: backward search that opens a frame at every class with two members or more.  Here a WAVE walks one
// pattern's tree, under a budget of nodes:
//   prepare  one pass over the batch's classes: class_summary of each (empty / its one member / wide) as 16 bits in cls_kind, so that
//            the walk reads one short per exact step instead of eight words; per pattern the number of wide classes and the
//            leftmost of them (cls_pat), and the refusals (offsets that decrease, more than BCE_HIP_CLASS_MAX_LEN classes, more
//            than BCE_HIP_CLASS_MAX_WIDE wide ones) into the flag word.  A refused pattern is skipped by the walk.
//   frames   wave-uniform, in LDS: (lo, hi, pos, the 256-bit set of the children that have rows and are not yet taken), 44 bytes,
//            BCE_CLASS_MAX_WIDE of them per wave.  Every lane writes the same words, so no lane reads what another wrote.
//   expand   at a wide class the 64 lanes share the 256 candidate bytes, lane + 64 q, q < 4: one step each for the members, 64
//            independent gather chains in flight; a ballot gives the frame's set and its popcount the nodes.
//   last     no wide class further left: every lane finishes its own children with the exact chain, counting the steps that had
//            rows, and the wave hands 64 intervals to the kernel's emit together (kd_near.hip's near_last_branch); no frame.
//   else     the children are taken one at a time in byte order: one uniform step gives the child's interval back, the wave runs
//            the exact steps down to the next wide class and expands there.
//   budget   looked at whenever the walk comes back to the stack, that is after every child taken and every finish: a wave-uniform
//            way out.  Between two looks lie one child's step and exact run (r + 1 steps), one expansion (at most 256) and, at the
//            last wide class, the finishes (256 steps for each of the `left` classes still to go): r + 1 + left <= m, so a walk
//            takes at most 256 m further steps after it has crossed its budget.
// Memory per wave: the frames.  Nothing grows with n, the answers or the budget; every loop is bounded by m, 256 or the budget.
// lo and hi stay in [0, n] on every level, as in count_kernel: every granule index is below ngran whatever the classes hold.
//
// Kernels, all one wave per pattern, four patterns a workgroup:
//   count   the rows of all answers, the nodes and the verdict: counts[p], work[p], status[p].
//   size    the rows, and in linear mode those whose hit runs across the end of the text; status[p].  An over-budget pattern has
//           no rows.  kd_locate.hip's scan (locate_scan) makes the CSR offsets.
//   fill    the search again for the patterns within budget (status[p] from the size pass); the wave writes (sa[row], pattern) of
//           every answer at a cursor of its own inside the pattern's segment: no atomics.  Then the locate's order -- two stable
//           radix_sort_pairs, on the position bits and on the pattern-id bits -- and one pass that keeps, in linear mode, the first
//           rows of each sorted segment (those across the end are its largest positions).
// Everything written is the locate's scratch (qb::loc_* of c->qbuf: the calls never run together), cls_* or the caller's outputs.
#include "common.h"
#include "class_step.h"
#include "scan_util.h"
#include "wave_walk.h"

namespace bce {

namespace {

constexpr int CLS_T = 256;                   // lanes per workgroup (4 waves = 4 patterns)
constexpr uint32_t CLS_WAVES = CLS_T / 64;
constexpr uint32_t CLS_MAXGRID = 8192;       // grid-stride kernels: workgroups at most
constexpr uint64_t CLS_MAXROWS = 0x7FFFFFFFull;
constexpr uint32_t CLS_BAD_ORDER = 1u, CLS_BAD_LEN = 2u, CLS_BAD_WIDE = 4u;   // bits of the flag word
constexpr uint32_t CLS_REFUSED = 0xFFFFFFFFu;                                 // cls_pat[2 p]: the walk skips pattern p

static_assert(BCE_CLASS_MAX_WIDE == BCE_HIP_CLASS_MAX_WIDE, "class_step.h and bce_hip.h name one bound");
static_assert(CLASS_OVER == BCE_HIP_CLASS_OVER, "class_step.h and bce_hip.h name one verdict");

struct ClsFrame {
  uint32_t lo, hi, pos;
  uint32_t set[8];
};

__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o); v = w < v ? w : v; }
  return v;
}

// kind[(off[p] - off[0]) + j] = class_summary of class j of pattern p; pinfo[2 p] = its wide classes (CLS_REFUSED: not to be
// walked), pinfo[2 p + 1] = the leftmost of them (m: none).  room: the classes kind[] holds -- a pattern that ends beyond it stands
// behind one that is refused anyway.
__global__ __launch_bounds__(CLS_T) void class_prepare_kernel(const uint32_t *__restrict__ masks, const uint64_t *__restrict__ off, uint32_t npat,
                                                              uint64_t room, uint16_t *__restrict__ kind, uint32_t *__restrict__ pinfo,
                                                              uint32_t *__restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * CLS_WAVES + (threadIdx.x >> 6);
  if (p >= npat) return;
  const uint64_t base = off[0], b = off[p], e = off[(size_t)p + 1];
  uint32_t why = 0;
  if (e < b || b < base) why = CLS_BAD_ORDER;
  else if (e - b > BCE_HIP_CLASS_MAX_LEN || e - base > room) why = CLS_BAD_LEN;
  if (why) {
    if (lane == 0) { atomicOr(bad, why); pinfo[2 * (size_t)p] = CLS_REFUSED; pinfo[2 * (size_t)p + 1] = 0; }
    return;
  }
  const uint32_t m = (uint32_t)(e - b);
  uint32_t wide = 0, first = m;
  for (uint32_t j = lane; j < m; j += 64u) {
    const uint32_t s = class_summary(masks + 8 * (b + j));
    kind[(b - base) + j] = (uint16_t)s;
    if (s >= CLASS_WIDE) { ++wide; first = j < first ? j : first; }
  }
  wide = (uint32_t)wave_sum64(wide);
  first = wave_min32(first);
  if (lane == 0) {
    if (wide > BCE_HIP_CLASS_MAX_WIDE) { atomicOr(bad, CLS_BAD_WIDE); wide = CLS_REFUSED; }
    pinfo[2 * (size_t)p] = wide;
    pinfo[2 * (size_t)p + 1] = first;
  }
}

// What a walk kernel is given besides its outputs.
struct ClsArgs {
  const Granule *gran;
  uint32_t ngran, n;
  Zeros8 z;
  const uint32_t *masks;
  const uint64_t *off;
  uint32_t npat;
  const uint16_t *kind;
  const uint32_t *pinfo;
  uint32_t max_nodes;
};

// A wave-uniform word kept in a vector register.  The walk is scalar-heavy -- interval, position, depth, node count, budget, and
// the mask, summary, plane and suffix-array pointers are all wave-uniform -- and with the eight `zeros` in scalar registers too the
// linear size kernel and the fill kernel ran out of them (8 and 3 spilled into vector lanes).  The vector file has room to spare.
__device__ __forceinline__ uint32_t in_vgpr(uint32_t s) {
  uint32_t v;
  asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}

// One pattern by one wave: S its masks, K its summaries, m classes, the leftmost wide one at first_wide.  fr: the wave's frames.
// emit(lo, rows) is called by all 64 lanes together: lane l brings the rows [lo, lo + rows) (rows == 0: nothing).  Returns the
// nodes: above max_nodes the walk has given up and what it has emitted is a part of the answer.
template <class Emit>
__device__ __forceinline__ uint32_t class_wave(const PlaneRank &R, const Zeros8 &zeros, const uint32_t *S, const uint16_t *K, uint32_t m, uint32_t n,
                                               uint32_t first_wide, uint32_t max_nodes, ClsFrame *fr, uint32_t lane, Emit &&emit) {
  Zeros8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z.v[j] = in_vgpr(zeros.v[j]);
  uint32_t nodes = 0;
  int d = -1;                                                        // the open frame
  uint32_t lo = 0, hi = n, pos = m;                                  // the node to open: the root first
  for (;;) {
    // the exact run down to the next wide class (class_run, the next summary fetched off the step's chain)
    bool live = true;
    uint32_t s = pos ? uni(K[pos - 1]) : 0u;
    while (pos > 0 && s < CLASS_WIDE) {
      const uint32_t next = pos > 1 ? uni(K[pos - 2]) : 0u;
      if (s < CLASS_ONE) { live = false; break; }
      fm_step(s & 0xFFu, z.v, lo, hi, R);
      lo = uni(lo); hi = uni(hi);
      if (lo >= hi) { live = false; break; }
      ++nodes;
      --pos;
      s = next;
    }
    if (live && pos == 0) emit(lo, lane == 0 ? hi - lo : 0u);
    if (live && pos > 0) {                                           // a wide class: its members with rows
      const uint32_t *mask = S + 8 * (size_t)(pos - 1);
      const bool last = pos - 1 == first_wide;
      uint32_t steps = 0;                                            // last: the steps of this lane's finishes that had rows
      if (!last) { ++d; fr[d].lo = lo; fr[d].hi = hi; fr[d].pos = pos; }
      for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t c = lane + 64u * q;
        uint32_t a = lo, b = lo;
        if (class_has(mask, c)) { b = hi; fm_step(c, z.v, a, b, R); }
        const bool has = a < b;
        const uint64_t born = __ballot(has);
        nodes += (uint32_t)__popcll(born);
        if (last) {
          if (has) {
            uint32_t left = pos - 1;
            uint32_t t = left ? K[left - 1] : 0u;
            while (left > 0 && a < b) {
              const uint32_t next = left > 1 ? K[left - 2] : 0u;
              if (t < CLASS_ONE) { b = a; break; }                   // (an empty class; no wide one stands left of first_wide)
              fm_step(t & 0xFFu, z.v, a, b, R);
              steps += a < b;
              --left;
              t = next;
            }
          }
          emit(a, b > a ? b - a : 0u);
        } else {
          fr[d].set[2 * q] = (uint32_t)born;
          fr[d].set[2 * q + 1] = (uint32_t)(born >> 32);
        }
      }
      if (last) nodes += (uint32_t)wave_sum64(steps);
    }
    // back at the stack: the budget, then the next child of the open frame
    if (nodes > max_nodes) break;
    uint32_t w = 0, bits = 0;
    while (d >= 0) {
      for (w = 0; w < 8u && (bits = uni(fr[d].set[w])) == 0u; ++w) {}
      if (w < 8u) break;
      --d;
    }
    if (d < 0) break;
    const uint32_t bit = (uint32_t)__builtin_ctz(bits);
    fr[d].set[w] = bits & (bits - 1u);
    lo = uni(fr[d].lo); hi = uni(fr[d].hi); pos = uni(fr[d].pos) - 1;
    fm_step(32u * w + bit, z.v, lo, hi, R);                          // (has rows: the expansion saw them)
    lo = uni(lo); hi = uni(hi);
  }
  return nodes;
}

// the wave's pattern, if it is to be walked
__device__ __forceinline__ bool class_pattern(const ClsArgs &A, uint32_t &p, const uint32_t *&S, const uint16_t *&K, uint32_t &m, uint32_t &first_wide) {
  p = blockIdx.x * CLS_WAVES + (threadIdx.x >> 6);
  if (p >= A.npat || A.pinfo[2 * (size_t)p] == CLS_REFUSED) return false;
  const uint64_t b = A.off[p];
  m = uni((uint32_t)(A.off[(size_t)p + 1] - b));
  S = A.masks + 8 * b;
  K = A.kind + (b - A.off[0]);
  first_wide = uni(A.pinfo[2 * (size_t)p + 1]);
  return true;
}

__global__ __launch_bounds__(CLS_T) void class_count_kernel(ClsArgs A, uint64_t *__restrict__ counts, uint64_t *__restrict__ work,
                                                            uint32_t *__restrict__ status) {
  __shared__ ClsFrame frames[CLS_WAVES][BCE_CLASS_MAX_WIDE];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p, m, first_wide;
  const uint32_t *S;
  const uint16_t *K;
  if (!class_pattern(A, p, S, K, m, first_wide)) return;
  uint64_t mine = 0;
  const uint32_t nodes = class_wave(PlaneRank{A.gran, A.ngran}, A.z, S, K, m, A.n, first_wide, A.max_nodes, frames[threadIdx.x >> 6], lane,
                                    [&](uint32_t, uint32_t rows) { mine += rows; });
  const uint64_t rows = wave_sum64(mine);
  const bool over = nodes > A.max_nodes;
  if (lane == 0) {
    counts[p] = over ? 0u : rows;
    if (work) work[p] = nodes;
    status[p] = over ? BCE_HIP_CLASS_OVER : 0u;
  }
}

// cnt[p] = the rows of pattern p; Linear: drop[p] = those whose hit does not end inside the text (two kernels: the cyclic one
// carries neither the pointers nor the row loop through its walk).  Over
// budget: neither has any.  sa == nullptr: the text of one byte, whose only rotation starts at 0.
template <bool Linear>
__global__ __launch_bounds__(CLS_T) void class_size_kernel(ClsArgs A, const uint32_t *__restrict__ sa, uint32_t *__restrict__ cnt,
                                                           uint32_t *__restrict__ drop, uint32_t *__restrict__ status) {
  __shared__ ClsFrame frames[CLS_WAVES][BCE_CLASS_MAX_WIDE];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p, m, first_wide;
  const uint32_t *S;
  const uint16_t *K;
  const bool run = class_pattern(A, p, S, K, m, first_wide);
  if (p >= A.npat) return;
  uint32_t mine = 0, out = 0, nodes = 0;                              // this lane's rows, and those of them across the end
  if (run) nodes = class_wave(PlaneRank{A.gran, A.ngran}, A.z, S, K, m, A.n, first_wide, A.max_nodes, frames[threadIdx.x >> 6], lane,
                              [&](uint32_t lo, uint32_t rows) {
    mine += rows;
    if (Linear) wave_rows(lo, rows, lane, [&](uint32_t, uint32_t row) { out += !fm_linear_hit(sa ? sa[row] : 0u, m, A.n); });
  });
  const uint64_t rows = wave_sum64(mine), across = wave_sum64(out);
  const bool over = nodes > A.max_nodes;
  if (lane == 0) {
    cnt[p] = over ? 0u : (uint32_t)rows;
    if (Linear) drop[p] = over ? 0u : (uint32_t)across;
    status[p] = over ? BCE_HIP_CLASS_OVER : 0u;
  }
}

// key[r], val[r] = (position, p) of every row r of pattern p's segment [start[p], start[p + 1]), in the order of the walk
__global__ __launch_bounds__(CLS_T) void class_fill_kernel(ClsArgs A, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ status,
                                                           const uint64_t *__restrict__ start, uint32_t *__restrict__ key,
                                                           uint32_t *__restrict__ val) {
  __shared__ ClsFrame frames[CLS_WAVES][BCE_CLASS_MAX_WIDE];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t p, m, first_wide;
  const uint32_t *S;
  const uint16_t *K;
  if (!class_pattern(A, p, S, K, m, first_wide) || status[p] != 0u) return;
  uint64_t cur = start[p];
  const uint64_t end = start[(size_t)p + 1];                          // (the size pass found as many rows: nothing is written past it)
  class_wave(PlaneRank{A.gran, A.ngran}, A.z, S, K, m, A.n, first_wide, A.max_nodes, frames[threadIdx.x >> 6], lane, [&](uint32_t lo, uint32_t rows) {
    cur += wave_rows(lo, rows, lane, [&](uint32_t o, uint32_t row) {
      const uint64_t r = cur + o;
      if (r < end) { key[r] = sa ? sa[row] : 0u; val[r] = p; }
    });
  });
}

// After the sorts: hit o < total of pattern p is the (o - hits[p])-th of p's sorted segment, which begins at cyc[p] (hits ==
// nullptr: cyclic mode, every row is a hit and o is its place).
__global__ __launch_bounds__(CLS_T) void class_out_kernel(const uint32_t *__restrict__ pos, const uint64_t *__restrict__ cyc,
                                                          const uint64_t *__restrict__ hits, uint32_t npat, uint64_t total,
                                                          uint32_t *__restrict__ out_pos) {
  for (uint64_t o = (uint64_t)blockIdx.x * CLS_T + threadIdx.x; o < total; o += (uint64_t)gridDim.x * CLS_T) {
    uint64_t s = o;
    if (hits) { const uint32_t p = fm_row_pattern(hits, npat, o); s = cyc[p] + (o - hits[p]); }
    out_pos[o] = pos[s];
  }
}

uint32_t wave_grid(uint32_t npat) { return (uint32_t)(((uint64_t)npat + CLS_WAVES - 1) / CLS_WAVES); }

// the flag word after a kernel: which refusal, if any (waits for the stream)
int class_verdict(bce_hip_ctx *c, const uint32_t *d_bad, const char *what) {
  uint32_t bad = 0;
  BCE_TRY(read_back(c, &bad, d_bad, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  if (bad & CLS_BAD_ORDER) { snprintf(c->err, sizeof c->err, "%s: pattern offsets decrease", what); return BCE_HIP_E_ARG; }
  if (bad & CLS_BAD_LEN) { snprintf(c->err, sizeof c->err, "%s: a pattern of more than %u classes", what, BCE_HIP_CLASS_MAX_LEN); return BCE_HIP_E_ARG; }
  if (bad & CLS_BAD_WIDE) {
    snprintf(c->err, sizeof c->err, "%s: a pattern with more than %u classes of two bytes or more", what, BCE_HIP_CLASS_MAX_WIDE);
    return BCE_HIP_E_ARG;
  }
  return BCE_HIP_OK;
}

// The prepare pass, queued; A: what the walk kernels take, d_bad: the flag word it may have raised.
int class_prepare(bce_hip_ctx *c, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, ClsArgs &A, uint32_t **d_bad) {
  uint64_t first = 0, last = 0;
  BCE_TRY(read_back(c, &first, d_off, 8));
  BCE_TRY(read_back(c, &last, d_off + npat, 8));
  const uint64_t most = (uint64_t)npat * BCE_HIP_CLASS_MAX_LEN;       // what a batch of npat patterns may hold
  const uint64_t room = last < first ? 0 : last - first < most ? last - first : most;
  BCE_TRY(ensure(c, c->qbuf[qb::cls_res], 8));
  BCE_TRY(ensure(c, c->qbuf[qb::cls_kind], (size_t)(room ? room : 1) * 2));
  BCE_TRY(ensure(c, c->qbuf[qb::cls_pat], (size_t)npat * 8));
  *d_bad = c->qbuf[qb::cls_res].as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(*d_bad, 0, 8, c->stream));
  A.gran = c->gran.as<Granule>();
  A.ngran = c->ngran;
  A.n = c->n;
  memcpy(A.z.v, c->zeros, sizeof A.z.v);
  A.masks = d_masks;
  A.off = d_off;
  A.npat = npat;
  A.kind = c->qbuf[qb::cls_kind].as<uint16_t>();
  A.pinfo = c->qbuf[qb::cls_pat].as<uint32_t>();
  A.max_nodes = max_nodes;
  hipLaunchKernelGGL(class_prepare_kernel, dim3(wave_grid(npat)), dim3(CLS_T), 0, c->stream, d_masks, d_off, npat, room,
                     c->qbuf[qb::cls_kind].as<uint16_t>(), c->qbuf[qb::cls_pat].as<uint32_t>(), *d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace

// d_counts[p] = the i in [0, n) with T[(i + j) mod n] in class j of pattern p for all j, p < npat, in the circular text of the
// context's planes; the classes of pattern p are d_masks[8 d_off[p], 8 d_off[p + 1]).  d_status[p]: 0, or BCE_HIP_CLASS_OVER when
// the pattern's search tree has more than max_nodes nodes (then d_counts[p] = 0); d_work[p] (unless null): the nodes counted.  All
// arrays: device memory of the context's device.  Queued on the context's stream; returns when the kernel is through (the flag
// word's way back is the wait).  Offsets that decrease, a pattern of more than BCE_HIP_CLASS_MAX_LEN classes or with more than
// BCE_HIP_CLASS_MAX_WIDE wide ones: BCE_HIP_E_ARG.  1 <= max_nodes <= BCE_HIP_CLASS_MAX_NODES is the caller's to keep.
int kd_class_count(bce_hip_ctx *c, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, uint64_t *d_counts,
                   uint64_t *d_work, uint32_t *d_status) {
  if (npat == 0) return BCE_HIP_OK;
  ClsArgs A;
  uint32_t *d_bad = nullptr;
  BCE_TRY(class_prepare(c, d_masks, d_off, npat, max_nodes, A, &d_bad));
  hipLaunchKernelGGL(class_count_kernel, dim3(wave_grid(npat)), dim3(CLS_T), 0, c->stream, A, d_counts, d_work, d_status);
  BCE_HIP_TRY(c, hipGetLastError());
  return class_verdict(c, d_bad, "count_classes");
}

// First half of a locate, as kd_near_size: d_hits[0, npat] receives the CSR offsets of the hits, *total their last word -- exact
// in both modes -- *rows the batch's cyclic rows, d_status[0, npat) the verdicts (an over-budget pattern has no hits).  Complete on
// return.  The refusals of kd_class_count; more than 2^31 - 1 rows: BCE_HIP_E_OVERFLOW, with d_hits, d_status and *total written.
// Leaves what kd_class_fill needs in loc_start / loc_lin and cls_kind / cls_pat.
int kd_class_size(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, bool linear,
                  uint64_t *d_hits, uint32_t *d_status, uint64_t *rows, uint64_t *total) {
  const size_t words = (size_t)npat * 4, starts = ((size_t)npat + 1) * 8;
  BCE_TRY(ensure(c, c->qbuf[qb::loc_res], 16));                                // (locate_scan's total word)
  BCE_TRY(ensure(c, c->qbuf[qb::loc_cnt], words));
  BCE_TRY(ensure(c, c->qbuf[qb::loc_start], starts));
  uint32_t *cnt = c->qbuf[qb::loc_cnt].as<uint32_t>(), *drop = nullptr;
  uint64_t *cyc = c->qbuf[qb::loc_start].as<uint64_t>();
  if (linear) {
    BCE_TRY(ensure(c, c->qbuf[qb::loc_drop], words));
    BCE_TRY(ensure(c, c->qbuf[qb::loc_lin], starts));
    drop = c->qbuf[qb::loc_drop].as<uint32_t>();
  }
  ClsArgs A;
  uint32_t *d_bad = nullptr;
  BCE_TRY(class_prepare(c, d_masks, d_off, npat, max_nodes, A, &d_bad));
  if (linear) hipLaunchKernelGGL(class_size_kernel<true>, dim3(wave_grid(npat)), dim3(CLS_T), 0, c->stream, A, sa, cnt, drop, d_status);
  else hipLaunchKernelGGL(class_size_kernel<false>, dim3(wave_grid(npat)), dim3(CLS_T), 0, c->stream, A, sa, cnt, drop, d_status);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(class_verdict(c, d_bad, "locate_classes"));
  BCE_TRY(locate_scan(c, cnt, nullptr, npat, cyc, rows));
  const uint64_t *hits = cyc;
  *total = *rows;
  if (linear) {
    hits = c->qbuf[qb::loc_lin].as<uint64_t>();
    BCE_TRY(locate_scan(c, cnt, drop, npat, c->qbuf[qb::loc_lin].as<uint64_t>(), total));
  }
  BCE_HIP_TRY(c, hipMemcpyAsync(d_hits, hits, starts, hipMemcpyDeviceToDevice, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*rows > CLS_MAXROWS) {
    snprintf(c->err, sizeof c->err, "locate_classes: the batch has %llu rows, one call gathers at most 2^31 - 1", (unsigned long long)*rows);
    return BCE_HIP_E_OVERFLOW;
  }
  return BCE_HIP_OK;
}

// Second half, straight after kd_class_size of the same batch (its rows <= 2^31 - 1, total and d_status): d_pos[0, total) receives
// the positions, each pattern's ascending.  Complete on return.
int kd_class_fill(bce_hip_ctx *c, const uint32_t *sa, const uint32_t *d_masks, const uint64_t *d_off, uint32_t npat, uint32_t max_nodes, bool linear,
                  uint64_t rows, uint64_t total, const uint32_t *d_status, uint32_t *d_pos) {
  if (total == 0) return BCE_HIP_OK;
  const uint32_t nrows = (uint32_t)rows;
  const size_t rbytes = (size_t)nrows * 4;
  for (DevBuf *b : {&c->qbuf[qb::loc_key0], &c->qbuf[qb::loc_key1], &c->qbuf[qb::loc_val0], &c->qbuf[qb::loc_val1]}) BCE_TRY(ensure(c, *b, rbytes));
  uint32_t *key[2] = {c->qbuf[qb::loc_key0].as<uint32_t>(), c->qbuf[qb::loc_key1].as<uint32_t>()};
  uint32_t *val[2] = {c->qbuf[qb::loc_val0].as<uint32_t>(), c->qbuf[qb::loc_val1].as<uint32_t>()};
  const uint64_t *cyc = c->qbuf[qb::loc_start].as<uint64_t>();
  ClsArgs A;                                                          // (cls_kind and cls_pat stand as the size pass left them)
  A.gran = c->gran.as<Granule>();
  A.ngran = c->ngran;
  A.n = c->n;
  memcpy(A.z.v, c->zeros, sizeof A.z.v);
  A.masks = d_masks;
  A.off = d_off;
  A.npat = npat;
  A.kind = c->qbuf[qb::cls_kind].as<uint16_t>();
  A.pinfo = c->qbuf[qb::cls_pat].as<uint32_t>();
  A.max_nodes = max_nodes;
  hipLaunchKernelGGL(class_fill_kernel, dim3(wave_grid(npat)), dim3(CLS_T), 0, c->stream, A, sa, d_status, cyc, key[0], val[0]);
  BCE_HIP_TRY(c, hipGetLastError());
  int res = 0;
  BCE_TRY(radix_sort_pairs(c, key, val, nrows, 0, ceil_log2(c->n), &res, 9));     // positions ascending
  const uint32_t *pos = key[res];
  if (npat > 1) {                                                    // stably back into patterns
    uint32_t *k2[2] = {val[res], val[res ^ 1]}, *v2[2] = {key[res], key[res ^ 1]};
    int r2 = 0;
    BCE_TRY(radix_sort_pairs(c, k2, v2, nrows, 0, ceil_log2(npat), &r2, 9));
    pos = v2[r2];
  }
  const uint64_t g = (total + CLS_T - 1) / CLS_T;
  hipLaunchKernelGGL(class_out_kernel, dim3((uint32_t)(g < CLS_MAXGRID ? g : CLS_MAXGRID)), dim3(CLS_T), 0, c->stream, pos, cyc,
                     linear ? c->qbuf[qb::loc_lin].as<uint64_t>() : (const uint64_t *)nullptr, npat, total, d_pos);
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
