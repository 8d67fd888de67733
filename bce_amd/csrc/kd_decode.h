// kd_decode.h -- what the files of the GPU-assisted decoder share (kd_decode.hip has the overview and the file map): the round
// kernels' arguments, the node rule and ONE copy of each step of a round; the tail hand-off; the switches, the sizes and the
// plain host functions through which one file reaches the kernels of another.
#pragma once
#include <stdlib.h>

#include <thread>
#include <vector>

#include "common.h"
#include "decoder_core.h"
#include "k3_args.h"
#include "scan_util.h"

namespace bce {

struct DecCtl {
  uint32_t cnt[2][8][2];     // [parity][plane][seg] node counts, as EnumCtl
  uint32_t ptot[8][4];       // per plane totals of the scan in flight: child0, child1, queries, escape queries
  uint32_t qbase[8];         // first query of each plane in this round's query buffer
  uint32_t ebase[8];         // first escape record (k > 31) of each plane
  uint32_t ticket, err;      // err: 1 inconsistent archive, 2 node list overflow in a one-launch round (cannot happen), 4 a wait too long
  uint32_t ovf, pad;         // bit q: plane q's children do not fit plane q + 1's list of the next parity (nothing of them written)
  uint64_t next_nodes;       // (8 planes of up to n / 2 + 2 nodes: more than 2^32)
  uint64_t nodes_total;
};
static_assert(sizeof(DecCtl) <= 4096, "read_back() moves it through 4 KB of pinned memory");

struct DecInfo {             // what the host needs after the query pass (pinned host memory)
  uint32_t qbase[8], qtot[8];
  uint32_t ebase[8], etot[8];
  uint64_t cur_nodes;
  uint32_t err, pad;
  uint64_t nodes_total;
};

constexpr uint32_t kEscape = 0x80000000u;

struct DecArgs {
  DecCtl *ctl;
  DecInfo *info;             // device pointer of the pinned DecInfo
  Node *list[2][8];          // [parity][plane]: cap[par][p] nodes each, child0s from the front, child1s from the back
  uint32_t *R;               // [8][n + 1] boundary ranks, kUnknown where not learnt yet
  uint32_t *tilecnt, *tileoff;   // [tiles][4]: 0 child0, 1 child1, 2 queries, 3 escape queries
  uint32_t *Q;               // queries of the round: k | ctx << 5 with the context resolved (k <= 31), or kEscape
  uint4 *E;                  // escape queries (k > 31) in the same order: (k, c1, c2, cs)
  const PlaneCfg *cfg;       // [8] the archive's context-bit tables (the preamble of each stream)
  const uint32_t *res;       // answers, same indexing
  uint32_t cap[2][8];
  uint32_t n, par;
  uint32_t zeros[8];         // zeros of plane p = C[(p+1)&7]: the child1 lists of plane p start there
  // Mailbox of the wave tail kernel (pinned, host-coherent; nullptr = leave at every query round):
  //   [0] device -> host: number of the query round whose queries are in Q / E / info
  //   [1] host -> device: number of the query round whose answers are in res
  //   [2] device -> host: set to 1 when the kernel has left
  uint32_t *mbox;
  uint32_t seq_base;         // number of the first query round of this launch (numbers never repeat within a decode)
  unsigned long long *words; // dec_small_kernel: one tagged count word per tile
  uint32_t round;            // ... and the round number the tags are made of
  // Six-launch rounds taken in two parts (the busiest plane first, see Decode::lane_round): the planes this launch works
  // on, the order in which the planes' queries lie in Q (4 bits each, first plane lowest), whether this children pass is
  // the round's last (it alone adds up the round)
  uint32_t pmask = 0xFFu, order = 0x76543210u, final = 1u;
  // Rounds with more nodes than the query budget run plane group by plane group: the planes of the group whose queries share
  // the query buffer now (the query bases count only these; each group's queries start at 0 -- below 2^32 by the budget, or a
  // plane's n / 2 + 2 nodes where one plane alone is more than the budget)
  uint32_t gmask = 0xFFu;
  uint64_t ecap = ~0ull;     // escape records the buffer E holds (dec_tiles_kernel<1> checks)
};

__device__ __forceinline__ Node *dec_nodes(const DecArgs &a, uint32_t par, uint32_t p) { return a.list[par][p]; }

__device__ __forceinline__ void dec_tile_prefix(const DecArgs &a, uint32_t tp[9]) {
  uint32_t acc = 0;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    tp[p] = acc;
    const uint32_t m = a.ctl->cnt[a.par][p][0] + a.ctl->cnt[a.par][p][1];
    acc += (m + K3_TILE - 1) / K3_TILE;
  }
  tp[8] = acc;
}

// Exclusive ranks of up to three flag sets over the nodes of a tile in list order (item, wave, lane), and the
// tile totals.  Two barriers; `lds` may be reused afterwards.
__device__ __forceinline__ void tile_ranks(const uint32_t (&f0)[K3_NPT], const uint32_t (&f1)[K3_NPT],
                                           const uint32_t (&f2)[K3_NPT], uint32_t (*lds)[4][3], uint32_t (&r0)[K3_NPT],
                                           uint32_t (&r1)[K3_NPT], uint32_t (&r2)[K3_NPT], uint32_t (&tot)[3]) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < K3_NPT; ++it) {
    const uint64_t b0 = __ballot(f0[it]), b1 = __ballot(f1[it]), b2 = __ballot(f2[it]);
    r0[it] = (uint32_t)__popcll(b0 & lt);
    r1[it] = (uint32_t)__popcll(b1 & lt);
    r2[it] = (uint32_t)__popcll(b2 & lt);
    if (lane == 0) {
      lds[it][w][0] = (uint32_t)__popcll(b0);
      lds[it][w][1] = (uint32_t)__popcll(b1);
      lds[it][w][2] = (uint32_t)__popcll(b2);
    }
  }
  __syncthreads();
  uint32_t run0 = 0, run1 = 0, run2 = 0;
#pragma unroll
  for (int it = 0; it < K3_NPT; ++it) {
    uint32_t b0 = run0, b1 = run1, b2 = run2;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const uint32_t x0 = lds[it][ww][0], x1 = lds[it][ww][1], x2 = lds[it][ww][2];
      if ((uint32_t)ww < w) { b0 += x0; b1 += x1; b2 += x2; }
      run0 += x0; run1 += x1; run2 += x2;
    }
    r0[it] += b0; r1[it] += b1; r2[it] += b2;
  }
  tot[0] = run0; tot[1] = run1; tot[2] = run2;
  __syncthreads();
}

// One node of BCE::code, decode mode (bce.cpp:1261-1351), split in two: what the ranks alone say ...
struct DCls { uint32_t s1, n1x, kind, mn, mx, bad; };   // kind 0: all zeros, 1: all ones, 2: forced split, 3: coded split
__device__ __forceinline__ DCls dec_classify(const Node &nd, const uint32_t *__restrict__ R, uint32_t n) {
  DCls c;
  const uint32_t x = nd.x0 + nd.x1;
  c.bad = ((uint64_t)nd.s + x > n || nd.x0 == 0 || nd.x1 == 0) ? 1u : 0u;
  const uint32_t s1 = c.bad ? 0u : R[nd.s], e1 = c.bad ? 0u : R[nd.s + x];
  if (s1 == kUnknown || e1 == kUnknown || e1 < s1 || e1 - s1 > x) c.bad = 1u;
  c.s1 = s1;
  c.n1x = c.bad ? 0u : e1 - s1;
  c.mn = c.mx = 0;
  if (c.n1x == 0) c.kind = 0;                                    // :1274-1279
  else if (c.n1x == x) c.kind = 1;                               // :1282-1287
  else {
    uint32_t mn = nd.x0 - c.n1x, mx = c.n1x - nd.x1;             // :1290-1294
    mn = ((int32_t)mn < 0) ? 0u : mn;
    mx = ((int32_t)mx < 0) ? 0u : mx;
    c.mn = mn;
    c.mx = nd.x0 - mx;
    c.kind = c.mx != c.mn ? 3u : 2u;
  }
  return c;
}
// ... and the children once the split n0x0 is known (:1337-1350).  Returns the value for R[s + x0].
__device__ __forceinline__ uint32_t dec_children(const Node &nd, const DCls &c, uint32_t n0x0, uint32_t zi, uint32_t &has0,
                                                 Node &c0, uint32_t &has1, Node &c1) {
  const uint32_t x = nd.x0 + nd.x1, s0 = nd.s - c.s1;
  has0 = has1 = 0;
  c0 = Node{0, 0, 0}; c1 = Node{0, 0, 0};
  if (c.kind == 0) { has0 = 1; c0 = Node{s0, nd.x0, nd.x1}; return c.s1; }
  if (c.kind == 1) { has1 = 1; c1 = Node{zi + c.s1, nd.x0, nd.x1}; return c.s1 + nd.x0; }
  const uint32_t n0x = x - c.n1x;
  const uint32_t n0x1 = n0x - n0x0;
  if (n0x0 && n0x1) { has0 = 1; c0 = Node{s0, n0x0, n0x1}; }
  const uint32_t n1x1 = nd.x1 - n0x1;
  const uint32_t n1x0 = c.n1x - n1x1;
  if (n1x0 && n1x1) { has1 = 1; c1 = Node{zi + c.s1, n1x0, n1x1}; }
  return c.s1 + n1x0;
}

// ---------------------------------------------------------------------------------------------------------
// The steps of a round, one copy each: the tile kernels, the one-launch kernel and the two tail kernels all run a round
// out of these.
// ---------------------------------------------------------------------------------------------------------

// Position i of a double-ended list of `cap` nodes: its c0 child0s from the front, the child1s from the back.
__device__ __forceinline__ uint32_t dec_list_index(uint32_t i, uint32_t c0, uint32_t cap) { return i < c0 ? i : cap - 1u - (i - c0); }

// The plane of position q where the planes' items lie one after the other: off[p] = plane p's first position, off[8] the end.
__device__ __forceinline__ uint32_t dec_plane_of(uint32_t q, const uint32_t *off) {
  uint32_t p = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k) p += (q >= off[k]) ? 1u : 0u;
  return p;
}

// The query of a coded node of plane p: get(k, _0x, _x1, _x) :1304.  k <= 31: one word, the context of get_context (:671-677)
// resolved here.  k > 31 (returns true): the word is kEscape and the record goes along in `esc`.  The caller stores them.
__device__ __forceinline__ bool dec_make_query(const PlaneCfg *cfg, uint32_t p, const Node &nd, const DCls &cl, uint32_t &word, uint4 &esc) {
  const uint32_t x = nd.x0 + nd.x1, k = cl.mx - cl.mn + 1u, c1 = x - cl.n1x, c2 = nd.x1;
  esc = make_uint4(k, c1, c2, x);                                // (always: these four are in registers either way)
  if (k > (uint32_t)kMaxK) { word = kEscape; return true; }
  word = k | (context_index(cfg[p].bits[k], c1, c2, x) << 5);
  return false;
}

// The split v of a node: mn where the ranks force it, mn + the decoder's answer where it was asked (isq).  Returns true if the
// answer is outside [mn, mx] (inconsistent archive; v is mn then).  Only a coded node can be inconsistent here: a forced split
// (kind 2) has v == mn == mx, and kinds 0 and 1 have mn == mx == 0 -- so testing the asked nodes alone is the same rule as
// testing every node of kind >= 2.
__device__ __forceinline__ bool dec_take_answer(const DCls &cl, bool isq, uint32_t answer, uint32_t &v) {
  v = cl.mn;
  if (!isq) return false;
  v += answer;
  if (v <= cl.mx) return false;
  v = cl.mn;
  return true;
}

// How a block begins tile ti of plane p's list: the nodes (item, wave, lane = list order; a tile's last items may be past the
// list: !valid), what the ranks R of the plane say about them, which of them ask the decoder (isq) and need an escape record
// (ise), and the exclusive ranks of both within the tile (qr, er; tot[0], tot[1] the tile's totals).  Returns nonzero if a node
// is inconsistent.  Two barriers; `lds` may be reused afterwards.
__device__ __forceinline__ uint32_t dec_load_tile(const DecArgs &a, uint32_t p, uint32_t ti, const uint32_t *R, uint32_t (*lds)[4][3],
                                                  Node (&nd)[K3_NPT], DCls (&cl)[K3_NPT], uint32_t (&valid)[K3_NPT],
                                                  uint32_t (&isq)[K3_NPT], uint32_t (&ise)[K3_NPT], uint32_t (&zero)[K3_NPT],
                                                  uint32_t (&qr)[K3_NPT], uint32_t (&er)[K3_NPT], uint32_t (&tot)[3]) {
  const uint32_t tid = threadIdx.x;
  const uint32_t c0n = a.ctl->cnt[a.par][p][0], M = c0n + a.ctl->cnt[a.par][p][1];
  const Node *src = dec_nodes(a, a.par, p);
  uint32_t bad = 0;
#pragma unroll
  for (int it = 0; it < K3_NPT; ++it) {
    const uint32_t q = ti * K3_TILE + (uint32_t)it * K3_T + tid;
    valid[it] = q < M ? 1u : 0u;
    const uint32_t qq = valid[it] ? q : ti * K3_TILE;
    nd[it] = src[dec_list_index(qq, c0n, a.cap[a.par][p])];
  }
#pragma unroll
  for (int it = 0; it < K3_NPT; ++it) {
    cl[it] = dec_classify(nd[it], R, a.n);
    bad |= cl[it].bad & valid[it];
    isq[it] = (valid[it] && cl[it].kind == 3u) ? 1u : 0u;
    ise[it] = (isq[it] && cl[it].mx - cl[it].mn + 1u > (uint32_t)kMaxK) ? 1u : 0u;
    zero[it] = 0;
  }
  uint32_t d2[K3_NPT];
  tile_ranks(isq, ise, zero, lds, qr, er, d2, tot);
  return bad;
}

// What the last block of a pass publishes (dec_scan_kernel, dec_small_kernel; one thread).  The nodes of the round:
__device__ __forceinline__ uint64_t dec_round_nodes(const DecCtl *ctl, uint32_t par) {
  uint64_t curn = 0;
  for (int q = 0; q < 8; ++q) curn += (uint64_t)ctl->cnt[par][q][0] + ctl->cnt[par][q][1];
  return curn;
}
// ... plane q's queries: where they begin in the query and escape buffers (for the kernel that writes them, and for the host)
// and how many they are,
__device__ __forceinline__ void dec_publish_queries(const DecArgs &a, uint32_t q, uint32_t qbase, uint32_t ebase, uint32_t qtot, uint32_t etot) {
  a.ctl->qbase[q] = qbase;
  a.ctl->ebase[q] = ebase;
  a.info->qbase[q] = qbase;
  a.info->qtot[q] = qtot;
  a.info->ebase[q] = ebase;
  a.info->etot[q] = etot;
}
// ... the rest of the host's DecInfo, its error word last,
__device__ __forceinline__ void dec_publish_info(const DecArgs &a, uint64_t curn) {
  a.info->cur_nodes = curn;
  a.info->nodes_total = a.ctl->nodes_total;
  __threadfence_system();
  a.info->err = a.ctl->err;
}
// ... and plane q's children, which are plane q + 1's nodes of the next round.  Returns true if they do not fit its list.
__device__ __forceinline__ bool dec_publish_children(const DecArgs &a, uint32_t q, uint32_t child0, uint32_t child1) {
  const uint32_t qn = (q + 1u) & 7u;
  a.ctl->cnt[a.par ^ 1u][qn][0] = child0;
  a.ctl->cnt[a.par ^ 1u][qn][1] = child1;
  return (uint64_t)child0 + child1 > a.cap[a.par ^ 1u][qn];
}

// ---------------------------------------------------------------------------------------------------------
// The tail hand-off: what one launch of a tail kernel (kd_tail.hip) leaves for Decode::tail_kernels (kd_decode.hip), and how
// the next launch is told to go on.
// ---------------------------------------------------------------------------------------------------------
enum TailStop : uint32_t {
  kTailDone = 0,             // nothing left, max_rounds run, or (workgroup kernel, leave-when-few) few nodes again
  kTailQuery = 1,            // stopped in front of a round with queries: they are in Q / E / info, nobody answered in time
  kTailOutgrown = 2,         // the round's nodes or children are more than the kernel holds; nothing of the round is written
  kTailBad = 3,              // an inconsistent node or an answer outside [mn, mx]
};
struct TailReport {
  uint32_t executed;         // rounds run by this launch
  uint32_t why;              // TailStop
  uint32_t pending;          // kTailQuery: the number of the query round whose queries are out (0 otherwise)
  uint32_t seq;              // the next query round's number
  uint32_t answered;         // the round the kernel stopped at has its answers in res already (the decoders have moved on)
};
// `resume` of a tail kernel launch:
constexpr uint32_t kTailHaveAnswers = 1u;    // the first round is the one a launch stopped at; its answers are in res, in query order
constexpr uint32_t kTailLeaveWhenFew = 2u;   // (workgroup kernel) leave once a round is down to 64 nodes: the wave kernel is faster

// ---------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t DS_MAXTILES = 2048;                     // dec_small_kernel: one block per tile, at most this many
constexpr uint32_t DS_MAXNODES = (DS_MAXTILES - 8u) * K3_TILE;
constexpr int DT_T = 1024;
constexpr int DT_NPT = 4;
constexpr uint32_t DT_CAP = DT_T * DT_NPT;      // nodes of all planes together that the workgroup tail kernel holds
constexpr uint32_t DT_ENTER = 2048;             // the host tries the tail kernels at or below this many nodes
constexpr uint32_t kHostTailMin = 20000;        // wave kernel rounds before a chain goes to the host, or n / 2500 if that is more (the copies cost ~n)

// The decoder's switches, read from the environment once per decode.  BCE_DEC_NO_* / FORCE_* / HOST_ENTER / GIVE_BACK force
// its routes (tests/test_gpu_decode_routes.py runs them all); BCE_DEC_TIMING, BCE_ALLOC_TRACE and BCE_DEC_TRACE print.
struct DecEnv {
  bool timing, alloc_trace, trace, no_small, no_split, no_tail, no_mailbox, no_host_tail, no_probe, force_host_tail, no_early_pin,
      give_back, tail_serial, tail_nopin;
  uint32_t host_enter;         // BCE_DEC_HOST_ENTER: how few nodes a round may hold for the host to take the tail early (8192)
  uint64_t capp_div;           // BCE_HIP_CAPP_DIV: the node lists start with n / capp_div + 4096 nodes (0: not set)
  bool mem() const { return timing || alloc_trace; }   // the device memory lines
};
inline DecEnv dec_env() {
  auto var = [](const char *name) -> const char * { return getenv(name); };
  DecEnv e;
  e.timing = var("BCE_DEC_TIMING"); e.alloc_trace = var("BCE_ALLOC_TRACE"); e.trace = var("BCE_DEC_TRACE");
  e.no_small = var("BCE_DEC_NO_SMALL"); e.no_split = var("BCE_DEC_NO_SPLIT"); e.no_tail = var("BCE_DEC_NO_TAIL");
  e.no_mailbox = var("BCE_DEC_NO_MAILBOX"); e.no_host_tail = var("BCE_DEC_NO_HOST_TAIL"); e.no_probe = var("BCE_DEC_NO_PROBE");
  e.force_host_tail = var("BCE_DEC_FORCE_HOST_TAIL"); e.no_early_pin = var("BCE_DEC_NO_EARLY_PIN"); e.give_back = var("BCE_DEC_GIVE_BACK");
  e.tail_serial = var("BCE_DEC_TAIL_SERIAL"); e.tail_nopin = var("BCE_DEC_TAIL_NOPIN");
  const char *h = var("BCE_DEC_HOST_ENTER"), *d = var("BCE_HIP_CAPP_DIV");
  e.host_enter = h ? (uint32_t)strtoul(h, nullptr, 10) : 8192u;
  e.capp_div = d ? strtoull(d, nullptr, 10) : 0;
  return e;
}

// A decode -- or a part of one run alone (the test hooks, the libdivsufsort seam) -- takes the context's scratch buffers: its
// compression state is gone.  While it runs c->dec_part names the part (1 rounds, 2 planes, 3 inverse BWT); PartEnd clears it.
inline void dec_drop_state(bce_hip_ctx *c) { c->stage = 0; c->enum_active = false; c->k1_valid = false; c->text_loaded = false; }
struct PartEnd { bce_hip_ctx *c; ~PartEnd() { c->dec_part = 0; } };

inline uint32_t plane_words(uint32_t n) { return (uint32_t)(((uint64_t)n + 31) / 32) + 3; }   // of a plane's bits, with slack
inline uint32_t plane_granules(uint32_t n) { return (uint32_t)((uint64_t)n / 96) + 2; }

// Device memory in use, sampled after an allocation stage (BCE_DEC_TIMING / BCE_ALLOC_TRACE); nullptr: nobody is asking.
inline void dec_sample_mem(size_t *peak_used) {
  size_t fr = 0, tot = 0;
  if (peak_used && hipMemGetInfo(&fr, &tot) == hipSuccess && tot - fr > *peak_used) *peak_used = tot - fr;
}

// kd_rounds.hip: the passes of a round over the planes of a.pmask, on `stream`.  Six launches (count / scan / write, twice) ...
void dec_query_pass(hipStream_t stream, const DecArgs &a, uint32_t grid);
void dec_children_pass(hipStream_t stream, const DecArgs &a, uint32_t grid);
// ... or two (dec_small_kernel: grid = the round's tiles, at most DS_MAXTILES)
void dec_small_query_pass(hipStream_t stream, const DecArgs &a, uint32_t grid);
void dec_small_children_pass(hipStream_t stream, const DecArgs &a, uint32_t grid);

// kd_tail.hip: one launch of the wave (<= 64 nodes) or the workgroup (<= DT_CAP nodes) tail kernel for at most max_rounds
// rounds; `report` is device memory, `resume` the bits above.
void dec_tail_launch(bce_hip_ctx *c, const DecArgs &a, bool wave, uint32_t max_rounds, TailReport *report, uint32_t resume);

// kd_backend.hip: R -> planes -> granules -> BWT bytes, and BWT -> text (see there).  peak_used: as dec_sample_mem.
int planes_stage(bce_hip_ctx *c, const uint32_t *R, uint32_t n, const uint32_t zeros[8], bool own_text, size_t *peak_used,
                 const uint32_t **words = nullptr, const uint32_t **rankw = nullptr);
int unbwt_stage(bce_hip_ctx *c, uint32_t n, uint32_t off, uint8_t *text, size_t *peak_used, uint64_t *lc, uint32_t *walkers);

// kd_host_tail.hip: the deep tail on the host (see there)
std::vector<int> tail_cpus(const DecEnv &env);
struct BigPin {
  bce_hip_ctx *c = nullptr;
  std::thread th;
  void *p = nullptr;
  size_t bytes = 0;
  bool registered = false;
  bool running = false, timing = false;
  double t_start = 0, t_done = 0;
  void start(bce_hip_ctx *ctx, size_t want);
  void settle();                                               // the buffer, if it came, becomes the context's
  ~BigPin() { settle(); }
};
int dec_host_tail(bce_hip_ctx *c, const DecEnv &env, const DecArgs &a, const DecCtl &ctl, std::vector<Decoder> &dec, uint32_t n,
                  uint32_t *round, uint64_t *nodes_total, uint64_t *queries_total, bool *bad_out);

}  // namespace bce
