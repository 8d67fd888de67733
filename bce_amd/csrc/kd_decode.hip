// kd_decode.hip -- GPU-assisted decoder (`bce -d`), SURVEY section 8f "next #1".
//
// BCE::decode (bce.cpp:1169-1233) walks the same 8 tries as the encoder (BCE::code mode 0, bce.cpp:1236-1374),
// but the split of every interval comes out of the plane's range decoder, whose state depends on every symbol
// before it: one strictly sequential stream per plane.  What is NOT sequential is everything around it, and
// that is where the reference spends its time (8n nodes, 3 rank look-ups each; then 8 cursor reads per byte for
// unbwt and one cache miss per byte for the inverse BWT).  So, per round:
//   GPU  (1) classify every node from the dense boundary-rank arrays R[p][x] = rank1_p(x) (known at every
//            boundary learnt so far); nodes whose split is forced need no symbol; the others become QUERIES
//            (k, c1, c2, cs) in stream order (count / scan / write, the K3 pattern),
//   host (2) the eight plane decoders answer their queries in order (8 threads: AdaptiveCoder::get,
//            bce.cpp:555-590; the adaptive counters live here because each answer feeds the next),
//   GPU  (3) children + the new boundary rank R[s + x0] from the answers (count / scan / write).
// After the last round: gap fill (between two known boundaries a plane is constant) -> rank granules ->
// wavelet-matrix access = unbwt::bytewise (bce.cpp:1043-1085) -> LF mapping by one radix pass -> inverse BWT by
// 2^18..2^19 concurrent walkers that stop at marked rows (segments are chained on the host, then written in
// place, rotated by `offset`, bce.cpp:1091-1093).
// The archive format, the model and the coder arithmetic are the reference's; parity = decode(reference
// archive) == input (tests/test_gpu_decode.py).  Inputs whose LF mapping is not one cycle (periodic inputs, on which
// the reference's decoder fails) are unrolled from the cycle through row 0.
// Where the text ends up is the caller's choice (DecDest): a host buffer (bce_hip_decompress_device), the caller's device
// memory, written by the walk itself (bce_hip_decompress_to_device), or the context's buffer, compared there with the
// original (bce_hip_verify_device / _host; kd_compare.hip).
// This file is the host driver (struct Decode: setup, the rounds and their routes, the stages after them) and the entry
// points.  The rest of the decoder:
//   kd_decode.h       what the files share: the kernels' arguments, the node rule, one copy of each step of a round, the
//                     tail hand-off (TailReport), the switches (DecEnv), and the host functions that reach the kernels
//   kd_rounds.hip     dec_tiles_kernel / dec_scan_kernel (six-launch rounds), dec_small_kernel (two-launch rounds)
//   kd_tail.hip       dec_tail_kernel (workgroup), dec_tail64_kernel (wave): forced rounds without the host
//   kd_host_tail.hip  dec_host_tail: the deep tail on eight host threads
//   kd_backend.hip    planes_stage, unbwt_stage (R -> planes -> BWT -> text), the test hooks, the libdivsufsort inverse seam
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "kd_decode.h"

namespace bce {

namespace {

// ---- the host's part of a round: the eight plane decoders answer their queries, in parallel ----
struct QueryPool {
  std::vector<Decoder> *dec = nullptr;
  const uint32_t *Q = nullptr;
  const uint4 *E = nullptr;
  uint32_t *res = nullptr;
  DecInfo info;
  std::thread th[8];
  std::mutex mu;
  std::condition_variable cv_go, cv_done;
  struct Job { const uint32_t *q; const uint4 *e; uint32_t *r; uint32_t cnt; };
  double t_begin[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_end[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double busy[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // seconds each plane's thread has spent answering, and how many queries (BCE_DEC_TIMING)
  uint64_t asked_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Job job[8] = {};
  uint64_t asked[8] = {0, 0, 0, 0, 0, 0, 0, 0}, answered[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool stop = false;

  static void answer(Decoder &d, const uint32_t *q, const uint4 *e, uint32_t *r, uint32_t cnt) {
    static_assert(sizeof(Decoder::Esc) == sizeof(uint4) && Decoder::kEscapeQuery == kEscape, "query formats");
    d.answer_batch(q, reinterpret_cast<const Decoder::Esc *>(e), r, cnt);
  }
  void worker(int p) {
    uint64_t seen = 0;
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_go.wait(lk, [&] { return stop || asked[p] != seen; });
        if (stop) return;
        seen = asked[p];
        j = job[p];
      }
      const double ta = now_s();
      answer((*dec)[p], j.q, j.e, j.r, j.cnt);
      t_begin[p] = ta;
      t_end[p] = now_s();
      busy[p] += t_end[p] - ta;
      asked_n[p] += j.cnt;
      {
        std::lock_guard<std::mutex> g(mu);
        answered[p] = seen;
      }
      cv_done.notify_all();
    }
  }
  void start() { for (int p = 0; p < 8; ++p) th[p] = std::thread([this, p] { worker(p); }); }
  // the planes of `mask` start on jobs[p] (queries, escape records, where the answers go, how many)
  void run_async(const Job jobs[8], uint32_t mask) {
    {
      std::lock_guard<std::mutex> g(mu);
      for (int p = 0; p < 8; ++p)
        if ((mask >> p) & 1u) { job[p] = jobs[p]; ++asked[p]; }
    }
    cv_go.notify_all();
  }
  void wait(uint32_t mask) {
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { for (int p = 0; p < 8; ++p) if (((mask >> p) & 1u) && answered[p] != asked[p]) return false; return true; });
  }
  uint32_t done_locked(uint32_t mask) const {
    uint32_t fin = 0;
    for (int p = 0; p < 8; ++p) if (((mask >> p) & 1u) && answered[p] == asked[p]) fin |= 1u << p;
    return fin;
  }
  uint32_t done(uint32_t mask) { std::lock_guard<std::mutex> g(mu); return done_locked(mask); }      // which of `mask` have answered
  uint32_t wait_any(uint32_t mask) {                                                                 // ... at least one of them (mask != 0)
    std::unique_lock<std::mutex> lk(mu);
    uint32_t fin = 0;
    cv_done.wait(lk, [&] { fin = done_locked(mask); return fin != 0 || mask == 0; });
    return fin;
  }
  void run(const DecInfo &in) {
    uint64_t total = 0;
    for (int p = 0; p < 8; ++p) total += in.qtot[p];
    if (total < 2048) {                                          // not worth waking anybody
      for (int p = 0; p < 8; ++p) answer((*dec)[p], Q + in.qbase[p], E + in.ebase[p], res + in.qbase[p], in.qtot[p]);
      return;
    }
    Job jobs[8];
    for (int p = 0; p < 8; ++p) jobs[p] = Job{Q + in.qbase[p], E + in.ebase[p], res + in.qbase[p], in.qtot[p]};
    run_async(jobs, 0xFFu);
    wait(0xFFu);
  }
  ~QueryPool() {
    { std::lock_guard<std::mutex> g(mu); stop = true; }
    cv_go.notify_all();
    for (int p = 0; p < 8; ++p) if (th[p].joinable()) th[p].join();
  }
};

struct Pinned {
  void *p = nullptr;
  size_t cap = 0;
  void **keep_p = nullptr;      // where the buffer lives on after this object (a slot of the context), if anywhere
  size_t *keep_cap = nullptr;
  Pinned() = default;
  Pinned(void **kp, size_t *kc) : p(*kp), cap(*kc), keep_p(kp), keep_cap(kc) {}
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  int ensure(bce_hip_ctx *c, size_t bytes, size_t least = (size_t)16 << 20) {
    if (bytes <= cap) return BCE_HIP_OK;
    size_t want = 2 * cap > bytes ? 2 * cap : bytes;          // pinning is slow (~0.15 s per GB): grow geometrically
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    if (want < least) want = least;
    const double t0 = now_s();
    // (the runtime's own pinned memory: kernels write here while the host reads -- see big_host_alloc in common.h)
    BCE_HIP_TRY(c, hipHostMalloc(&p, want, hipHostMallocCoherent | hipHostMallocMapped));   // the wave tail kernel reads answers written while it runs
    c->pin_s += now_s() - t0; c->pin_bytes += want; c->pin_calls++;
    cap = want;
    return BCE_HIP_OK;
  }
  ~Pinned() {
    if (keep_p) { *keep_p = p; *keep_cap = cap; }
    else if (p) (void)hipHostFree(p);
  }
};

struct Mailbox {               // a few host-coherent words the wave tail kernel and the host exchange while the kernel runs
  uint32_t *host = nullptr, *dev = nullptr;
  int open(bce_hip_ctx *c) {
    BCE_HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&host), 64, hipHostMallocCoherent | hipHostMallocMapped));
    for (int i = 0; i < 16; ++i) host[i] = 0;
    BCE_HIP_TRY(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), host, 0));
    return BCE_HIP_OK;
  }
  ~Mailbox() { if (host) (void)hipHostFree(host); }
};


// The node lists of a decode: one per (parity, plane), at most n / 2 + 2 nodes each (the worst case: disjoint intervals of width
// >= 2), and to begin with an eighth of n (what k3_begin starts the encoder with: text fills 0.02-0.03 n, random bytes 0.15-0.3 n)
// or what the context's buffer already holds.  A round whose children would not fit a list does not write them (the scan of
// the children pass checks; the one-launch kernel, which checks afterwards, is only used where twice the round's nodes fit):
// that one list -- the next parity's list of plane q + 1, which only plane q's children pass writes -- is replaced by a larger
// one and the pass runs again from the answers it already has (Decode::grow_lists).  Test knob 12 /
// BCE_HIP_CAPP_DIV as for the encoder.
uint32_t dec_full_capP(uint32_t n) { return (uint32_t)((uint64_t)n / 2 + 2); }
uint32_t dec_capP(const bce_hip_ctx *c, const DecEnv &env, uint32_t n, size_t archive_bytes, bool *forced_out) {
  const uint64_t full = dec_full_capP(n);
  uint64_t div = 8;
  bool forced = false;
  if (c->dbg_capp_div) { div = c->dbg_capp_div; forced = true; }
  if (env.capp_div >= 1) { div = env.capp_div; forced = true; }
  uint64_t cap = (uint64_t)n / div + 4096;
  // (the one-launch rounds need twice a round's nodes to fit: 4 M nodes per list at least, i.e. the worst case up to 8 MB of
  //  input -- with n / 8 a 1 MB input left them for its widest rounds and decoded in 32 ms instead of 16)
  if (!forced && cap < ((uint64_t)4 << 20)) cap = (uint64_t)4 << 20;
  // How full the lists get goes with how well the input compresses -- text (archive = 0.23 n) fills 0.03 n per list, random
  // bytes (1.0 n) 0.2-0.3 n -- and the archive's size is known before the first round: 0.25 x archive bytes nodes per list
  // spares a high-entropy archive most of the lists that grow in the middle of a round.
  if (!forced) { const uint64_t by_ratio = (uint64_t)(0.25 * (double)archive_bytes) + 4096; if (by_ratio > cap) cap = by_ratio; }
  *forced_out = forced;
  return (uint32_t)(cap < full ? cap : full);
}

// The query budget: the nodes whose queries one pass of a round holds (test knob 13; at least DT_CAP, so that the rounds the
// tail kernels hand back with their answers -- at most DT_CAP nodes -- are never split).
uint64_t dec_budget(const bce_hip_ctx *c) {
  if (!c->dbg_dec_budget) return (uint64_t)1 << 30;
  return c->dbg_dec_budget > DT_CAP ? c->dbg_dec_budget : DT_CAP;
}

struct Events {
  hipEvent_t e[8] = {};
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// Where a decode's text goes (decompress_device).  The inverse BWT's walk writes single bytes at any address, so the caller's
// device memory is written directly: kDevice needs no text buffer of the context's at all.
struct DecDest {
  enum Kind { kHost, kDevice, kCompare, kChecksum } kind;
  uint8_t *out = nullptr;        // kHost: the caller's host buffer, kDevice: the caller's device buffer (any alignment), of cap bytes
  size_t cap = 0;
  // kCompare: the text stays in the context's own buffer and is compared there with orig_n bytes, which are on the device
  // (orig_dev) or on the host (orig_host: uploaded into the BWT's buffer, idle once the walk has read it)
  const uint8_t *orig_dev = nullptr, *orig_host = nullptr;
  uint64_t orig_n = 0;
  uint64_t *first_diff = nullptr;
  // kChecksum: the text stays in the context's own buffer and only its CRC-32 is reported (kd_crc32.hip); kHost with `crc`: the
  // same word beside the copy to the host -- taken from the context's buffer, on the device, before the copy is queued
  uint32_t *crc = nullptr;
  bool own_text() const { return kind != kDevice; }            // the text lands in c->text

  static DecDest to_host(uint8_t *out, size_t cap, uint32_t *crc = nullptr) { DecDest d{kHost}; d.out = out; d.cap = cap; d.crc = crc; return d; }
  static DecDest to_device(void *d_out, size_t cap) { DecDest d{kDevice}; d.out = static_cast<uint8_t *>(d_out); d.cap = cap; return d; }
  static DecDest compare_with(const void *d_orig, const uint8_t *h_orig, uint64_t n, uint64_t *first_diff) {
    DecDest d{kCompare};
    d.orig_dev = static_cast<const uint8_t *>(d_orig); d.orig_host = h_orig; d.orig_n = n; d.first_diff = first_diff;
    return d;
  }
  static DecDest checksum_only(uint32_t *crc) { DecDest d{kChecksum}; d.crc = crc; return d; }
};

// What BCE_DEC_TIMING and BCE_ALLOC_TRACE report about the rounds
struct DecStats {
  double t_q = 0, t_copy = 0, t_host = 0, t_c = 0;      // query pass, copy out, host decoders, children pass (and the rest)
  uint64_t tail_rounds = 0, mbox_rounds = 0, small_rounds = 0, grouped_rounds = 0, list_grows = 0;
  size_t peak_used = 0;                                 // device memory in use, sampled after every allocation stage
  // six-launch rounds: their time, launching the first query passes, waiting for the first plane's, all lanes started,
  // waiting for the decoders, the last children pass; the lanes' begin / end times (dbg_r) and which plane ended last
  uint64_t split_rounds = 0;
  double t_split = 0, ts_issue = 0, ts_first = 0, ts_lanes = 0, ts_wait = 0, ts_rb = 0;
  double dbg_r[5] = {0, 0, 0, 0, 0};
  uint32_t dbg_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t wide_hist[32] = {0}, wide_nodes[32] = {0};   // rounds outside the tail by log2 of their node count
  double wide_time[32] = {0};
  uint64_t launches_wave = 0, launches_wg = 0, rounds_wave = 0, rounds_wg = 0, nodes_wave = 0, nodes_wg = 0;
  double t_wave = 0, t_wg = 0;
};

// How a round outside the tail kernels runs (Decode::plan)
struct RoundPlan {
  bool small, direct, lanes;   // one launch per pass (dec_small_kernel); queries and answers in pinned memory; six launches
  uint32_t ord[8];             // the planes, busiest first in six-launch rounds
  uint32_t gm[8];              // the plane groups (masks), ng of them
  int ng;
  uint64_t gmax;               // the most nodes of a group
  uint32_t grid, hb;           // the passes' grid; log2 of the node count (BCE_DEC_TIMING)
  double t0;                   // when the round began (BCE_DEC_TIMING)
};

// One decode: the state its stages share.  decompress_device runs the stages in order.
struct Decode {
  bce_hip_ctx *c;
  const DecEnv env = dec_env();
  ArchiveHead &hd;
  const DecDest &dest;
  const uint32_t n;
  const size_t rstride;                                        // of the boundary ranks R[8][n + 1]
  const uint32_t full_cap;                                     // the largest node list a decode can need
  DecArgs a;
  DecCtl ctl;                                                  // the control block as last read back
  DecInfo *info = nullptr;
  DecStats st;
  double tp0 = now_s(), t0 = 0;                                // when the stage / the round began
  // (query, escape-record and answer buffers stay with the context: pinning their ~150 MB anew was 0.05 s of every decode)
  Pinned pin_info, pin_q, pin_e, pin_res;
  Events ev;
  QueryPool pool;
  Mailbox mbox;                                                // of the wave tail kernel (see DecArgs::mbox)
  BigPin big_pin;
  DevBuf &Qbuf, &Ebuf, &Rsbuf;                                 // queries / escape queries / answers of a round (device side)
  TailReport *d_report = nullptr;                              // what a tail kernel launch did (device memory)
  // the rounds
  uint64_t cur_nodes = 0, nodes_total = 0, queries_total = 0;
  uint32_t round = 0;
  bool answered_pending = false;                               // pin_res holds the answers of the round about to run
  uint32_t next_seq = 1, last_answered = 0;                    // mailbox query rounds
  uint32_t prev_qtot[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // each plane's queries in the last round
  const uint64_t budget;                                       // nodes whose queries one pass of a round holds (see the plane groups)
  const bool host_tail_ok;
  bool host_has_ccx = false;
  uint32_t tail_after = 0;                                     // wave kernel rounds after which a chain goes to the host
  const uint64_t tail_min;                                     // nodes still to come that make a tail worth a copy of the ranks
  // Query-heavy tails (executables: something is coded in half of the rounds) go to the host as a whole: a query round costs the
  // resident kernels a mailbox round trip (~10 us), the host -- eight threads, one per plane -- nothing.  Whether a tail is
  // query-heavy is measured: the first kProbeRounds rounds of the tail kernels count their mailbox rounds.
  static constexpr uint32_t kProbeRounds = 1024;
  uint32_t probe_rounds = 0;
  uint64_t probe_mbox0 = 0;
  bool probe_done, query_heavy = false;

  Decode(bce_hip_ctx *ctx, ArchiveHead &h, const DecDest &to)
      : c(ctx), hd(h), dest(to), n(h.n), rstride((size_t)h.n + 1), full_cap(dec_full_capP(h.n)),
        pin_q(&ctx->dec_pin[0], &ctx->dec_pin_cap[0]), pin_e(&ctx->dec_pin[1], &ctx->dec_pin_cap[1]),
        pin_res(&ctx->dec_pin[2], &ctx->dec_pin_cap[2]), Qbuf(ctx->skey[0]), Ebuf(ctx->skey[1]), Rsbuf(ctx->sesc),
        budget(dec_budget(ctx)), host_tail_ok(!env.no_host_tail), tail_min((h.n >> 6) + (1u << 18)),
        probe_done(env.no_probe) {
    big_pin.timing = env.timing;
    if (env.force_host_tail) { probe_done = true; query_heavy = true; }
  }
  uint64_t left() const { return 8ull * (n - 1u) - nodes_total; }   // nodes still to come
  size_t *peak() { return env.mem() ? &st.peak_used : nullptr; }    // where device memory in use is sampled to, if anybody asks
  void sample_mem() { dec_sample_mem(peak()); }
  void progress() { if (c->progress) c->progress(nodes_total, 8ull * n, c->progress_user); }

  // ---- lists, boundary ranks, roots ----
  int setup(size_t archive_bytes) {
    uint32_t max_cap = 0;
    bool forced = false;
    const uint32_t start = dec_capP(c, env, n, archive_bytes, &forced);
    for (int par = 0; par < 2; ++par)
      for (int p = 0; p < 8; ++p) {
        uint64_t lc = start;
        const uint64_t held = c->dlist[par][p].cap / sizeof(Node);
        if (!forced && held > lc) lc = held < full_cap ? held : full_cap;
        BCE_TRY(ensure(c, c->dlist[par][p], (size_t)lc * sizeof(Node)));
        a.cap[par][p] = (uint32_t)lc;
        a.list[par][p] = c->dlist[par][p].as<Node>();
        if (lc > max_cap) max_cap = (uint32_t)lc;
      }
    BCE_TRY(ensure(c, c->ctl, sizeof(DecCtl) > sizeof(EnumCtl) ? sizeof(DecCtl) : sizeof(EnumCtl)));
    const size_t max_tiles = (size_t)8 * ((max_cap + K3_TILE - 1) / K3_TILE + 1);
    BCE_TRY(ensure(c, c->tilecnt, max_tiles * 16));
    BCE_TRY(ensure(c, c->tileoff, max_tiles * 16));
    DevBuf &Rbuf = c->dfs;                                        // 8 x (n + 1) boundary ranks
    BCE_TRY(ensure(c, Rbuf, 8 * rstride * 4));
    uint32_t *R = Rbuf.as<uint32_t>();
    BCE_HIP_TRY(c, hipMemsetAsync(R, 0xFF, 8 * rstride * 4, c->stream));
    memset(&ctl, 0, sizeof ctl);
    for (int i = 0; i < 8; ++i) {
      const uint32_t zero = 0, ones = n - hd.C[i];               // R[p][0] = 0, R[(i+7)&7][n] = n - C[i]  (:1207-1211)
      BCE_HIP_TRY(c, hipMemcpyAsync(R + (size_t)i * rstride, &zero, 4, hipMemcpyHostToDevice, c->stream));
      BCE_HIP_TRY(c, hipMemcpyAsync(R + (size_t)((i + 7) & 7) * rstride + n, &ones, 4, hipMemcpyHostToDevice, c->stream));
      BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));            // stack temporaries
      if (hd.C[i] && n - hd.C[i]) {                               // :1214-1216
        const Node root = {0u, hd.C[i], n - hd.C[i]};
        BCE_HIP_TRY(c, hipMemcpyAsync(a.list[0][i], &root, sizeof root, hipMemcpyHostToDevice, c->stream));
        BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
        ctl.cnt[0][i][0] = 1;
      }
    }
    BCE_HIP_TRY(c, hipMemcpyAsync(c->ctl.p, &ctl, sizeof ctl, hipMemcpyHostToDevice, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
    BCE_TRY(pin_info.ensure(c, sizeof(DecInfo), 4096));          // (a few words: not the 16 MB the query buffers start with -- 4 ms of pinning per decode)
    info = static_cast<DecInfo *>(pin_info.p);
    memset(info, 0, sizeof *info);

    a.ctl = c->ctl.as<DecCtl>();
    a.info = info;                                                // pinned host memory is device-accessible at the same address
    a.R = R;
    a.tilecnt = c->tilecnt.as<uint32_t>();
    a.tileoff = c->tileoff.as<uint32_t>();
    a.n = n;
    for (int p = 0; p < 8; ++p) a.zeros[p] = hd.C[(p + 1) & 7];
    {
      PlaneCfg hcfg[8];
      for (int p = 0; p < 8; ++p) hcfg[p] = hd.dec[p].cfg;
      BCE_TRY(ensure(c, c->dcfg, sizeof hcfg));
      BCE_HIP_TRY(c, hipMemcpy(c->dcfg.p, hcfg, sizeof hcfg, hipMemcpyHostToDevice));
      a.cfg = c->dcfg.as<PlaneCfg>();
    }
    pool.dec = &hd.dec;
    pool.start();

    if (env.timing) { fprintf(stderr, "gpu decode: setup %.3f s\n", now_s() - tp0); tp0 = now_s(); }
    for (int i = 0; i < 8; ++i) cur_nodes += ctl.cnt[0][i][0];
    if (!env.no_mailbox) BCE_TRY(mbox.open(c));
    // (ski rental: the copies cost ~1.2 ns per input byte, a round ~1.0 us less on the host than in the wave kernel, so the
    //  switch pays once n / 830 rounds are still to come -- which nobody knows -- and is made after that many have gone by)
    tail_after = n / 2500u > kHostTailMin ? n / 2500u : kHostTailMin;
    // With eight CPUs on one L3 for its threads the host does a node of a tail round in ~20 ns (measured: 18.8 M nodes of the
    // binary corpus in 0.37 s, against 1.4 s in the resident kernels; the natural corpus' 20 M nodes in 0.6 s against 1.1 s):
    // then every tail that is worth the copy goes there and nothing is probed.
    // ... every LONG tail, that is: the copy and the threads cost ~0.1 s, which a tail of a few hundred rounds (text) does not have
    // to spare -- so the resident kernels always get the first kProbeRounds rounds.
    const size_t tail_ncpu = tail_cpus(env).size();
    host_has_ccx = std::thread::hardware_concurrency() >= 8u && !env.tail_serial && tail_ncpu == 8;
    if (env.timing) fprintf(stderr, "gpu decode: host tail CPUs: %zu of one L3 domain in the affinity mask, %u hardware threads: tails go to the host early %d\n",
                            tail_ncpu, std::thread::hardware_concurrency(), (int)host_has_ccx);
    BCE_TRY(ensure(c, c->smwords, (size_t)DS_MAXTILES * 8));
    BCE_HIP_TRY(c, hipMemsetAsync(c->smwords.p, 0, (size_t)DS_MAXTILES * 8, c->stream));      // pass tags of an earlier decode
    a.words = c->smwords.as<unsigned long long>();
    BCE_TRY(ensure(c, c->runs, 64));
    d_report = c->runs.as<TailReport>();
    return BCE_HIP_OK;
  }

  // ---- the rounds (BCE::code mode 0, :1246-1371) ----
  int rounds() {
    while (cur_nodes) {
      t0 = now_s();
      a.par = round & 1u;
      // Rounds of a few thousand nodes cost the GPU ~40 us each (two launches, two syncs) whatever they hold; eight host threads
      // do 8192 nodes in about that time and 1024 in a tenth of it.  Where the host takes the tail anyway (a CCX for its
      // threads) it takes it from here on, provided the tail is LONG -- at least 512 more rounds at the present width, and worth
      // the copy of the ranks: text's few hundred tail rounds stay on the device.
      // (past the half-way mark with 64 rounds' worth of the present width still to come, its pinned buffer is started: the
      //  widths of text fall geometrically from their peak -- the ratio stays under ~50 until next to nothing is left --, a long
      //  tail does not)
      if (host_tail_ok && host_has_ccx && !big_pin.running && left() <= 4ull * (n - 1u) && left() >= tail_min &&
          left() >= 64ull * cur_nodes && !env.no_early_pin)
        big_pin.start(c, 8 * ((size_t)n + 1) * 4);
      if (host_tail_ok && host_has_ccx && !answered_pending && !env.no_tail && cur_nodes <= env.host_enter &&
          left() >= tail_min && left() >= 512ull * cur_nodes && left() <= 8ull * (n - 1u) / 8u) {
        BCE_TRY(to_host("tail", true));
        st.t_c += now_s() - t0;
        break;
      }
      if (cur_nodes <= DT_ENTER && !env.no_tail) {
        BCE_TRY(tail_kernels());
        a.par = round & 1u;
        st.t_c += now_s() - t0;
        t0 = now_s();
        progress();
        if (!cur_nodes) break;
      }
      RoundPlan rp = {};
      BCE_TRY(plan(rp));
      uint64_t queries = 0;
      BCE_TRY(rp.lanes ? lane_round(rp, &queries) : group_round(rp, &queries));
      end_round(rp, queries);
    }
    return BCE_HIP_OK;
  }

  // The rest of the rounds on the host (dec_host_tail).  The BCE_DEC_TIMING line names the `tail` and, if asked, the width it
  // began at.
  int to_host(const char *tail, bool say_width) {
    bool bad = false;
    const double th = now_s();
    const uint32_t r0 = round;
    big_pin.settle();
    BCE_TRY(dec_host_tail(c, env, a, ctl, hd.dec, n, &round, &nodes_total, &queries_total, &bad));
    if (bad) { snprintf(c->err, sizeof c->err, "decode: inconsistent archive (round %u)", round); return BCE_HIP_E_INTERNAL; }
    if (env.timing) {
      char width[64] = "";
      if (say_width) snprintf(width, sizeof width, " from %llu nodes a round on", (unsigned long long)cur_nodes);
      fprintf(stderr, "gpu decode: %u rounds of the %s on the host%s, %.3f s with the copies\n", round - r0, tail, width, now_s() - th);
    }
    cur_nodes = 0;
    return BCE_HIP_OK;
  }

  uint64_t answer_tail(const DecArgs &at) {               // the queries in pin_q / pin_e -> answers in pin_res
    const DecInfo in = *info;
    uint64_t qt = 0;
    for (int p = 0; p < 8; ++p) {
      QueryPool::answer(hd.dec[p], at.Q + in.qbase[p], at.E + in.ebase[p], static_cast<uint32_t *>(pin_res.p) + in.qbase[p], in.qtot[p]);
      qt += in.qtot[p];
    }
    return qt;
  }

  // Few nodes: the tail kernels run the forced rounds on the device; at a round with queries the workgroup kernel emits them
  // straight into pinned memory, the host answers (inline: they are few) and the kernel resumes with the answers -- one launch
  // and one sync per query round.
  int tail_kernels() {
    BCE_TRY(pin_q.ensure(c, (size_t)(DT_CAP + 16) * 4));
    BCE_TRY(pin_e.ensure(c, (size_t)(DT_CAP + 16) * sizeof(uint4)));
    BCE_TRY(pin_res.ensure(c, (size_t)(DT_CAP + 16) * 4));
    DecArgs at = a;
    at.Q = static_cast<uint32_t *>(pin_q.p);
    at.E = static_cast<uint4 *>(pin_e.p);
    at.res = static_cast<const uint32_t *>(pin_res.p);
    bool resume = false, force_wg = false;
    answered_pending = false;
    for (;;) {
      TailReport done = {};
      // the whole tail on the host (see above): nothing of this round has been asked or answered yet
      if (host_tail_ok && query_heavy && !resume && !answered_pending && cur_nodes && cur_nodes <= DT_CAP && left() >= tail_min &&
          left() <= 8ull * (n - 1u) / 8u)
        return to_host("tail", false);
      const bool wave = !force_wg && cur_nodes <= 64;
      at.par = round & 1u;
      const double t_launch = now_s();
      at.mbox = mbox.dev;
      at.seq_base = next_seq;
      if (at.mbox) __atomic_store_n(&mbox.host[2], 0u, __ATOMIC_RELEASE);
      const bool probing = host_tail_ok && !probe_done && left() >= tail_min;   // (a tail worth a copy of the ranks)
      if (probing && probe_rounds == 0) probe_mbox0 = st.mbox_rounds;
      const uint32_t probe_left = kProbeRounds > probe_rounds ? kProbeRounds - probe_rounds : 1u;
      const uint32_t max_wave = !host_tail_ok ? (1u << 30) : (probing && probe_left < tail_after ? probe_left : tail_after);
      const uint32_t have = resume ? kTailHaveAnswers : 0u;
      if (wave) dec_tail_launch(c, at, true, max_wave, d_report, have);
      else dec_tail_launch(c, at, false, probing ? probe_left : (1u << 30), d_report, have | kTailLeaveWhenFew);
      if (at.mbox) {
        // (before the copies below are queued: a device-to-host copy into pageable memory blocks the host until the kernel is done)
        // the tail kernel stays resident over query rounds: serve its mailbox until it says it has left
        const double t_poll = now_s();
        for (uint32_t spins = 0;; ++spins) {
          if (__atomic_load_n(&mbox.host[0], __ATOMIC_ACQUIRE) == next_seq) {
            queries_total += answer_tail(at);
            __atomic_store_n(&mbox.host[1], next_seq, __ATOMIC_RELEASE);
            last_answered = next_seq++;
            ++st.mbox_rounds;
            continue;
          }
          if (__atomic_load_n(&mbox.host[2], __ATOMIC_ACQUIRE)) break;
          if ((spins & 1023u) == 1023u && (hipStreamQuery(c->stream) != hipErrorNotReady || now_s() - t_poll > 30.0)) break;   // a failed launch never raises the flag
          __builtin_ia32_pause();
        }
      }
      static_assert(sizeof(TailReport) == 20, "five words, as the tail kernels write them");
      BCE_TRY(read_back(c, &done, d_report, sizeof done));
      BCE_TRY(read_back(c, &ctl, c->ctl.p, sizeof ctl));
      BCE_HIP_TRY(c, hipGetLastError());
      if (env.trace) fprintf(stderr, "tail: round %u wave %d resume %d -> done %u why %u next %llu\n", round, (int)wave, (int)resume, done.executed, done.why, (unsigned long long)ctl.next_nodes);
      round += done.executed; st.tail_rounds += done.executed;
      if (wave) { ++st.launches_wave; st.rounds_wave += done.executed; st.nodes_wave += ctl.nodes_total - nodes_total; st.t_wave += now_s() - t_launch; }
      else { ++st.launches_wg; st.rounds_wg += done.executed; st.nodes_wg += ctl.nodes_total - nodes_total; st.t_wg += now_s() - t_launch; }
      cur_nodes = ctl.next_nodes;
      nodes_total = ctl.nodes_total;
      // a resumed launch that could not even start its round (children outgrow the kernel, or an inconsistency):
      // the decoders have ALREADY answered this round's queries -- whoever runs the round must reuse the answers
      const bool stuck = done.answered != 0 && (done.why == kTailOutgrown || done.why == kTailBad);
      resume = false;
      force_wg = false;
      if (done.why == kTailQuery) {                            // queries of round `round` are in pin_q / pin_e
        // (a wave kernel that gave up waiting may have been answered through the mailbox at the same moment)
        if (!(at.mbox && done.pending != 0 && done.pending == last_answered)) {
          queries_total += answer_tail(at);
          if (at.mbox) { last_answered = done.pending; next_seq = done.pending + 1u; }
        }
        resume = true;
        continue;
      }
      if (wave && done.why == kTailOutgrown && cur_nodes <= DT_CAP) {   // the children outgrow one wave: the workgroup kernel
        force_wg = true;
        resume = stuck;                                        // ... with the answers, if this round already has them
        continue;
      }
      answered_pending = stuck;
      if (probing) {
        probe_rounds += done.executed;
        if (probe_rounds >= kProbeRounds) { probe_done = true; query_heavy = host_has_ccx || (st.mbox_rounds - probe_mbox0) * 3u >= probe_rounds * 2u; /* two rounds in three ask the decoders something */ }
      }
      if (host_tail_ok && done.why == kTailDone && !stuck && cur_nodes &&
          ((wave && done.executed >= tail_after && cur_nodes <= 64) || (query_heavy && cur_nodes <= DT_CAP)))
        return to_host("deep tail", false);                    // a long chain of a few nodes: the rest of the rounds on the host
      if (done.why == kTailDone && done.executed && cur_nodes && cur_nodes <= DT_ENTER) continue;   // handed back (few nodes again) or out of max_rounds
      return BCE_HIP_OK;                                       // nothing left, too many nodes (kTailOutgrown) or an inconsistent node (kTailBad)
    }
  }

  // How a round outside the tail kernels runs: its passes, the order of its planes, its plane groups and its buffers.
  int plan(RoundPlan &rp) {
    // Rounds of up to kDirectNodes nodes exchange their queries and answers through pinned host memory (as the tail kernels do):
    // the kernels write / read it over the bus, and the round is two launches and two syncs with no copy in between.
    // (dec_small_kernel writes the children before it knows their number: only where twice the round's nodes fit every list)
    constexpr uint64_t kDirectNodes = 1u << 18;
    uint32_t min_next_cap = ~0u;
    for (int p = 0; p < 8; ++p) min_next_cap = std::min(min_next_cap, a.cap[(round & 1u) ^ 1u][p]);
    rp.small = cur_nodes <= DS_MAXNODES && !env.no_small && 2ull * cur_nodes <= min_next_cap && cur_nodes <= budget;
    rp.direct = rp.small && cur_nodes <= kDirectNodes && !answered_pending;
    rp.lanes = !rp.small && !answered_pending && !env.no_split;  // six launches, plane by plane (see lane_round)
    uint64_t pnodes[8];
    for (int p = 0; p < 8; ++p) pnodes[p] = (uint64_t)ctl.cnt[round & 1u][p][0] + ctl.cnt[round & 1u][p][1];
    {
      // the tile arrays for this round's lists (a list that grew may hold more tiles than they were made for)
      uint64_t tiles = 8;
      for (int p = 0; p < 8; ++p) tiles += (pnodes[p] + K3_TILE - 1) / K3_TILE;
      BCE_TRY(ensure(c, c->tilecnt, (size_t)tiles * 16));
      BCE_TRY(ensure(c, c->tileoff, (size_t)tiles * 16));
      a.tilecnt = c->tilecnt.as<uint32_t>();
      a.tileoff = c->tileoff.as<uint32_t>();
    }
    for (int i = 0; i < 8; ++i) rp.ord[i] = (uint32_t)i;
    if (rp.lanes) {
      // (the bulk of the queries moves from plane p to plane p + 1 with every round -- a node's children are the next plane's
      //  nodes -- and the busiest decoder with it: plane p is as busy as plane p - 1 was last round.  Node counts say less:
      //  how many of a plane's nodes are forced differs from plane to plane.)
      uint64_t weight[8];
      for (int q = 0; q < 8; ++q) weight[q] = ((uint64_t)prev_qtot[(q + 7) & 7] << 1) + (pnodes[q] ? 1u : 0u);
      std::stable_sort(rp.ord, rp.ord + 8, [&](uint32_t x, uint32_t y) { return weight[x] > weight[y]; });
    }
    // Plane groups: consecutive runs of `ord` (busiest first in the six-launch rounds, plane order otherwise) with at most `budget`
    // nodes together -- one group of all eight planes when the round is within the budget, which is then run exactly as it
    // always was.  A plane alone may hold more than the budget (up to n / 2 + 2 nodes): it is a group of its own.
    uint64_t emax = 0;
    {
      uint64_t acc = 0;
      for (int i = 0; i < 8; ++i) {
        const uint32_t p = rp.ord[i];
        if (rp.ng == 0 || acc + pnodes[p] > budget) { rp.gm[rp.ng++] = 0; acc = 0; }
        rp.gm[rp.ng - 1] |= 1u << p;
        acc += pnodes[p];
      }
      for (int g = 0; g < rp.ng; ++g) {
        uint64_t gn = 0;
        for (int p = 0; p < 8; ++p) if ((rp.gm[g] >> p) & 1u) gn += pnodes[p];
        // an escape query (k > 31) needs a node of at least 32 positions, and a plane's nodes are disjoint intervals of [0, n]:
        // at most n / 32 + 1 of them per plane, however many nodes the group holds
        const uint64_t ebound = std::min<uint64_t>(gn, (uint64_t)__builtin_popcount(rp.gm[g]) * ((uint64_t)n / 32 + 1));
        rp.gmax = std::max(rp.gmax, gn);
        emax = std::max(emax, ebound);
      }
    }
    if (rp.ng > 1 && answered_pending) { snprintf(c->err, sizeof c->err, "decode: a resumed round of %llu nodes is over the query budget", (unsigned long long)cur_nodes); return BCE_HIP_E_INTERNAL; }
    if (rp.direct) {
      BCE_TRY(pin_q.ensure(c, (size_t)(cur_nodes + 16) * 4));
      BCE_TRY(pin_e.ensure(c, (size_t)(cur_nodes + 16) * sizeof(uint4)));
      BCE_TRY(pin_res.ensure(c, (size_t)(cur_nodes + 16) * 4));
      a.Q = static_cast<uint32_t *>(pin_q.p);
      a.E = static_cast<uint4 *>(pin_e.p);
      a.res = static_cast<const uint32_t *>(pin_res.p);
      a.ecap = cur_nodes + 16;
    } else {
      BCE_TRY(ensure(c, Qbuf, (size_t)(rp.gmax + 16) * 4));
      BCE_TRY(ensure(c, Ebuf, (size_t)(emax + 16) * sizeof(uint4)));
      BCE_TRY(ensure(c, Rsbuf, (size_t)(rp.gmax + 16) * 4));
      a.Q = Qbuf.as<uint32_t>();
      a.E = Ebuf.as<uint4>();
      a.res = Rsbuf.as<uint32_t>();
      a.ecap = emax + 16;
    }
    if (rp.ng > 1) { ++st.grouped_rounds; c->dec_split_rounds++; }
    if (cur_nodes >= (1u << 20)) sample_mem();
    const uint64_t want = (cur_nodes + K3_TILE - 1) / K3_TILE + 8;
    rp.grid = (uint32_t)(want < 2048 ? want : 2048);
    rp.t0 = env.timing ? now_s() : 0.0;
    if (env.timing) { while ((2ull << rp.hb) <= cur_nodes && rp.hb < 31) ++rp.hb; st.wide_hist[rp.hb]++; st.wide_nodes[rp.hb] += cur_nodes; }
    a.round = round;
    return BCE_HIP_OK;
  }

  // A six-launch round plane by plane.  The round's time is the busiest planes' sequential decoders (text: planes 0 and 1 hold
  // half of all queries) with the query passes in front of them and the children passes behind.  The planes of a round do not
  // meet (plane p's children are plane p + 1's nodes of the NEXT round), so each plane is a lane of its own -- query pass, copy
  // out, decoder, answers in, children pass -- and the lanes start in the order of their node counts: the busiest decoder starts
  // as soon as ITS queries are out and only its own children pass is left when it is done; everything else runs beside it.
  // Over the query budget the lanes run group by group, each group with the whole query and answer buffers to itself.
  int lane_round(const RoundPlan &rp, uint64_t *queries) {
    const uint32_t *ord = rp.ord;
    const double ts0 = now_s();
    for (int i = 0; i < 8; ++i) if (!ev.e[i]) BCE_HIP_TRY(c, hipEventCreateWithFlags(&ev.e[i], hipEventDisableTiming));
    uint32_t order = 0;
    for (int i = 0; i < 8; ++i) order |= ord[i] << (4 * i);
    BCE_TRY(pin_q.ensure(c, (size_t)(rp.gmax + 16) * 4));        // (a plane's queries lie at its base: the bases are exact, the size is a bound)
    BCE_TRY(pin_res.ensure(c, (size_t)(rp.gmax + 16) * 4));
    a.order = order;
    a.final = 0;
    uint64_t qtotal = 0;
    uint32_t new_qtot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t launched = 0;                                       // planes whose decoders ran (all groups)
    int lo = 0;                                                  // the group's first lane in `ord`
    for (int g = 0; g < rp.ng; ++g) {
      const bool last_group = g + 1 == rp.ng;
      const uint32_t gmask = rp.gm[g];
      const int L = __builtin_popcount(gmask);
      a.gmask = gmask;
      auto ask = [&](int i) -> int {                             // the query pass of lane i of the group
        a.pmask = 1u << ord[lo + i];
        a.final = 0;
        dec_query_pass(c->stream, a, rp.grid);
        BCE_HIP_TRY(c, hipEventRecord(ev.e[i], c->stream));
        return BCE_HIP_OK;
      };
      BCE_TRY(ask(0));                                           // (launching costs the host ~60 us a lane: the busiest decoder does not wait for all eight)
      if (L > 1) BCE_TRY(ask(1));
      const double tsa = now_s();
      if (g == 0) st.ts_issue += tsa - ts0;
      QueryPool::Job jobs[8] = {};
      struct Settle {                                            // no decoder outlives this group (its buffers, an early return)
        QueryPool &pool; uint32_t mask;
        ~Settle() { if (mask) pool.wait(mask); }
      } settle{pool, 0u};
      uint32_t glaunched = 0, children_done = 0;                 // planes whose decoders run / whose children pass is queued
      auto children = [&](uint32_t p, bool last) -> int {
        if (jobs[p].cnt) BCE_HIP_TRY(c, hipMemcpyAsync(Rsbuf.as<uint32_t>() + (jobs[p].r - static_cast<uint32_t *>(pin_res.p)), jobs[p].r, (size_t)jobs[p].cnt * 4, hipMemcpyHostToDevice, c->stream));
        a.pmask = 1u << p;
        a.final = last && last_group ? 1u : 0u;
        dec_children_pass(c->stream, a, rp.grid);
        children_done |= 1u << p;
        return BCE_HIP_OK;
      };
      for (int i = 0; i < L; ++i) {
        const uint32_t p = ord[lo + i];
        if (i > 0 && i + 1 < L) BCE_TRY(ask(i + 1));             // one lane ahead of the one being waited for
        BCE_HIP_TRY(c, hipEventSynchronize(ev.e[i]));
        if (i == 0 && g == 0) st.ts_first += now_s() - tsa;
        const DecInfo in = *info;                                // (plane p's fields and those of the planes before it; the rest are being written)
        if (in.err) { snprintf(c->err, sizeof c->err, "decode: inconsistent archive (round %u)", round); return BCE_HIP_E_INTERNAL; }
        const uint32_t qn = in.qtot[p], en = in.etot[p], qb = in.qbase[p], eb = in.ebase[p];
        new_qtot[p] = qn;
        qtotal += qn;
        if ((size_t)eb + en + 1 > pin_e.cap / sizeof(uint4)) {   // escape records are few, their number is not known ahead: grow between decoders
          if (settle.mask) { pool.wait(settle.mask); }
          BCE_TRY(pin_e.ensure(c, 2 * ((size_t)eb + en + 1) * sizeof(uint4)));
        }
        if (qn) {
          BCE_HIP_TRY(c, hipMemcpyAsync(static_cast<uint32_t *>(pin_q.p) + qb, a.Q + qb, (size_t)qn * 4, hipMemcpyDeviceToHost, c->copy_stream));
          if (en) BCE_HIP_TRY(c, hipMemcpyAsync(static_cast<uint4 *>(pin_e.p) + eb, a.E + eb, (size_t)en * sizeof(uint4), hipMemcpyDeviceToHost, c->copy_stream));
          BCE_HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
          jobs[p] = QueryPool::Job{static_cast<const uint32_t *>(pin_q.p) + qb, static_cast<const uint4 *>(pin_e.p) + eb, static_cast<uint32_t *>(pin_res.p) + qb, qn};
          pool.run_async(jobs, 1u << p);
          settle.mask |= 1u << p;
          glaunched |= 1u << p;
        } else {
          jobs[p] = QueryPool::Job{nullptr, nullptr, static_cast<uint32_t *>(pin_res.p) + qb, 0u};
          BCE_TRY(children(p, i == L - 1 && (glaunched & ~children_done) == 0u));   // nothing to ask: its children pass at once (the round's last one only if nobody is out)
        }
        // decoders that have finished meanwhile: their children passes go out between the copies
        const uint32_t fin = pool.done(glaunched & ~children_done);
        for (uint32_t q = 0; q < 8; ++q)
          if ((fin >> q) & 1u) { settle.mask &= ~(1u << q); BCE_TRY(children(q, i == L - 1 && (children_done | (1u << q)) == gmask)); }
      }
      const double tsb = now_s();
      st.ts_lanes += tsb - tsa;
      while (children_done != gmask) {
        const uint32_t fin = pool.wait_any(glaunched & ~children_done);
        for (uint32_t q = 0; q < 8; ++q)
          if ((fin >> q) & 1u) { settle.mask &= ~(1u << q); BCE_TRY(children(q, (children_done | (1u << q)) == gmask)); }
      }
      launched |= glaunched;
      const double tsc = now_s();
      st.ts_wait += tsc - tsb;
      // (the next group reuses the query and answer buffers: this read-back also waits for the last copy of answers)
      BCE_TRY(read_back(c, &ctl, c->ctl.p, sizeof ctl));
      st.ts_rb += now_s() - tsc;
      BCE_HIP_TRY(c, hipGetLastError());
      BCE_TRY(settle_group(rp.grid));
      lo += L;
    }
    a.pmask = 0xFFu; a.order = 0x76543210u; a.final = 1u; a.gmask = 0xFFu;
    if (env.timing) {
      double last = 0; int lastp = -1;
      for (int q = 0; q < 8; ++q) if (((launched >> q) & 1u) && pool.t_end[q] > last) { last = pool.t_end[q]; lastp = q; }
      if ((launched >> ord[0]) & 1u) { st.dbg_r[0] += pool.t_begin[ord[0]] - ts0; st.dbg_r[1] += pool.t_end[ord[0]] - ts0; }
      if (lastp >= 0) { st.dbg_r[2] += last - ts0; st.dbg_r[3] += pool.t_begin[lastp] - ts0; st.dbg_last[lastp]++; }
      st.dbg_r[4] += now_s() - ts0;
    }
    for (int q = 0; q < 8; ++q) prev_qtot[q] = new_qtot[q];
    ++st.split_rounds;
    st.t_split += now_s() - ts0;
    *queries = qtotal;
    return BCE_HIP_OK;
  }

  // One pass over all planes (or the planes of one group after the other): query pass, the decoders, children pass.
  int group_round(const RoundPlan &rp, uint64_t *queries) {
    uint64_t round_q = 0;
    for (int g = 0; g < rp.ng; ++g) {
      const uint32_t gm = rp.gm[g];
      a.pmask = a.gmask = gm;
      a.final = g + 1 == rp.ng ? 1u : 0u;
      if (rp.small) {
        dec_small_query_pass(c->stream, a, rp.grid);
        ++st.small_rounds;
      } else {
        dec_query_pass(c->stream, a, rp.grid);
      }
      BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
      BCE_HIP_TRY(c, hipGetLastError());
      DecInfo in = *info;
      for (int p = 0; p < 8; ++p)                                  // (the query pass of a group writes its own planes' fields only)
        if (!((gm >> p) & 1u)) { in.qbase[p] = in.qtot[p] = in.ebase[p] = in.etot[p] = 0; }
      { const double t1 = now_s(); st.t_q += t1 - t0; t0 = t1; }
      if (in.err == 2) { snprintf(c->err, sizeof c->err, "decode: node list overflow in a one-launch round (round %u)", round); return BCE_HIP_E_INTERNAL; }
      if (in.err) { snprintf(c->err, sizeof c->err, "decode: inconsistent archive (round %u)", round); return BCE_HIP_E_INTERNAL; }
      uint64_t qtotal = 0, etotal = 0;
      for (int p = 0; p < 8; ++p) { qtotal += in.qtot[p]; etotal += in.etot[p]; if ((gm >> p) & 1u) prev_qtot[p] = in.qtot[p]; }
      if (qtotal && answered_pending) {
        // the tail kernel emitted exactly these queries (same order) and the decoders answered them: do not ask twice
        BCE_HIP_TRY(c, hipMemcpyAsync(Rsbuf.p, pin_res.p, qtotal * 4, hipMemcpyHostToDevice, c->stream));
      } else if (qtotal) {
        if (!rp.direct) {
          BCE_TRY(pin_q.ensure(c, qtotal * 4));
          BCE_TRY(pin_e.ensure(c, (etotal + 1) * sizeof(uint4)));
          BCE_TRY(pin_res.ensure(c, qtotal * 4));
          BCE_HIP_TRY(c, hipMemcpyAsync(pin_q.p, a.Q, qtotal * 4, hipMemcpyDeviceToHost, c->stream));
          if (etotal) BCE_HIP_TRY(c, hipMemcpyAsync(pin_e.p, a.E, etotal * sizeof(uint4), hipMemcpyDeviceToHost, c->stream));
          BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
          { const double t1 = now_s(); st.t_copy += t1 - t0; t0 = t1; }
        }
        pool.Q = static_cast<const uint32_t *>(pin_q.p);
        pool.E = static_cast<const uint4 *>(pin_e.p);
        pool.res = static_cast<uint32_t *>(pin_res.p);
        pool.run(in);
        { const double t1 = now_s(); st.t_host += t1 - t0; t0 = t1; }
        if (!rp.direct) BCE_HIP_TRY(c, hipMemcpyAsync(Rsbuf.p, pin_res.p, qtotal * 4, hipMemcpyHostToDevice, c->stream));
      }
      answered_pending = false;
      if (rp.small) dec_small_children_pass(c->stream, a, rp.grid);
      else dec_children_pass(c->stream, a, rp.grid);
      // the next round's size: read the control block (the query pass of the next round would tell, but its grid needs it)
      BCE_TRY(read_back(c, &ctl, c->ctl.p, sizeof ctl));
      BCE_HIP_TRY(c, hipGetLastError());
      BCE_TRY(settle_group(rp.grid));
      round_q += qtotal;
    }
    a.pmask = a.gmask = 0xFFu; a.final = 1u;
    st.t_c += now_s() - t0;
    *queries = round_q;
    return BCE_HIP_OK;
  }

  // The bookkeeping every round outside the tail kernels ends with
  void end_round(const RoundPlan &rp, uint64_t queries) {
    if (env.timing) st.wide_time[rp.hb] += now_s() - rp.t0;
    cur_nodes = ctl.next_nodes;
    nodes_total = ctl.nodes_total;
    progress();
    queries_total += queries;
    ++round;
  }

  // A children pass found that the children of the planes in `ovf` do not fit their lists (it wrote none of them; the counts
  // are in the control block): each such list -- plane q + 1's of the next parity, which only plane q's pass writes, so it
  // holds nothing yet -- is replaced by one of 1.25 x the need (exactly the need if the device has no more room, after the
  // other phases' buffers have gone back), and the pass runs again from the answers already in the answer buffer.  A plane's
  // decoder is never asked twice.
  int grow_lists(uint32_t ovf) {
    const uint32_t out = (round & 1u) ^ 1u;
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t q = 0; q < 8; ++q) {
      if (!((ovf >> q) & 1u)) continue;
      const uint32_t qn = (q + 1u) & 7u;
      const uint64_t need = (uint64_t)ctl.cnt[out][qn][0] + ctl.cnt[out][qn][1];
      const uint32_t had = a.cap[out][qn];
      if (need <= had || need > full_cap) {
        snprintf(c->err, sizeof c->err, "decode: round %u reports a list of %llu nodes (it holds %u, n = %u)", round, (unsigned long long)need, had, n);
        return BCE_HIP_E_INTERNAL;
      }
      release(c->dlist[out][qn]);
      a.list[out][qn] = nullptr; a.cap[out][qn] = 0;
      uint64_t want = need + need / 4;
      if (want > full_cap) want = full_cap;
      int rc = ensure(c, c->dlist[out][qn], (size_t)want * sizeof(Node), kAllocListFirst);
      if (rc == BCE_HIP_E_NOMEM) {
        want = need;
        rc = ensure(c, c->dlist[out][qn], (size_t)want * sizeof(Node), kAllocListFallback);
      }
      if (rc != BCE_HIP_OK) {
        if (rc == BCE_HIP_E_NOMEM) snprintf(c->err, sizeof c->err, "decode: no device memory for a node list of %llu nodes (round %u, n = %u)", (unsigned long long)need, round, n);
        return rc;
      }
      a.list[out][qn] = c->dlist[out][qn].as<Node>();
      a.cap[out][qn] = (uint32_t)want;
      c->dec_list_grows++;
      ++st.list_grows;
      if (env.mem())
        fprintf(stderr, "gpu decode: round %u does not fit the node lists: the children of plane %u (%llu nodes) in plane %u's list of %u (parity %u), grown in place to %llu\n",
                round, q, (unsigned long long)need, qn, had, out, (unsigned long long)want);
    }
    BCE_HIP_TRY(c, hipMemsetAsync(&a.ctl->ovf, 0, sizeof(uint32_t), c->stream));
    return BCE_HIP_OK;
  }

  // After the children passes of a group, with `ctl` just read back: errors, and the lists that must grow
  int settle_group(uint32_t grid) {
    for (int tries = 0;; ++tries) {
      if (ctl.err) {
        if (ctl.err == 4) snprintf(c->err, sizeof c->err, "decode: a two-launch round waited too long for a predecessor tile (round %u)", round);
        else if (ctl.err == 2) snprintf(c->err, sizeof c->err, "decode: node list overflow in a one-launch round (round %u)", round);
        else snprintf(c->err, sizeof c->err, "decode: inconsistent archive (round %u)", round);
        return BCE_HIP_E_INTERNAL;
      }
      if (!ctl.ovf) return BCE_HIP_OK;
      if (tries == 2) { snprintf(c->err, sizeof c->err, "decode: node lists still too small after growing (round %u)", round); return BCE_HIP_E_INTERNAL; }
      const uint32_t ovf = ctl.ovf;
      BCE_TRY(grow_lists(ovf));
      const uint32_t pm = a.pmask, fin = a.final;
      a.pmask = ovf;
      a.final = 0;                                               // (the round's totals were added up by its last pass already)
      dec_children_pass(c->stream, a, grid);
      a.pmask = pm; a.final = fin;
      BCE_TRY(read_back(c, &ctl, c->ctl.p, sizeof ctl));
      BCE_HIP_TRY(c, hipGetLastError());
    }
  }

  void report_rounds() {
    if (env.timing) { fprintf(stderr, "gpu decode: %u rounds (%llu of them in the tail kernels, %llu query rounds answered through the mailbox), %llu nodes, %llu queries: %.3f s (query pass %.3f, copy out %.3f, host decoders %.3f, children pass %.3f)\n",
                              round, (unsigned long long)st.tail_rounds, (unsigned long long)st.mbox_rounds, (unsigned long long)nodes_total, (unsigned long long)queries_total, now_s() - tp0, st.t_q, st.t_copy, st.t_host, st.t_c); tp0 = now_s(); }
    if (env.timing) fprintf(stderr, "gpu decode: tail probe: %u rounds, %llu query rounds through the mailbox since it began; query-heavy %d\n",
                            probe_rounds, (unsigned long long)(probe_rounds ? st.mbox_rounds - probe_mbox0 : 0), (int)query_heavy);
    if (env.mem()) fprintf(stderr, "gpu decode: %llu rounds over the query budget of %llu nodes run in plane groups, %llu node lists grown in place; device memory in use during the rounds: %.1f GB at most\n",
                           (unsigned long long)st.grouped_rounds, (unsigned long long)budget, (unsigned long long)st.list_grows, st.peak_used / 1e9);
    if (!env.timing) return;
    fprintf(stderr, "gpu decode: %llu six-launch rounds plane by plane (busiest first): %.3f s (launching the query passes %.3f, the first plane's %.3f, all lanes started after %.3f, waiting for decoders %.3f, last children pass %.3f)\n",
            (unsigned long long)st.split_rounds, st.t_split, st.ts_issue, st.ts_first, st.ts_lanes, st.ts_wait, st.ts_rb);
    fprintf(stderr, "gpu decode: decoder threads (answers through the pool only):");
    for (int p = 0; p < 8; ++p) fprintf(stderr, " plane %d %.1f M in %.3f s (%.1f ns);", p, pool.asked_n[p] * 1e-6, pool.busy[p], pool.asked_n[p] ? pool.busy[p] * 1e9 / pool.asked_n[p] : 0.0);
    fprintf(stderr, "\n");
    fprintf(stderr, "gpu decode: lanes: busiest plane's decoder began %.3f, ended %.3f; the last decoder began %.3f, ended %.3f; all children passes queued %.3f (sums over the rounds, from the round's start); last to end: %u %u %u %u %u %u %u %u\n",
            st.dbg_r[0], st.dbg_r[1], st.dbg_r[3], st.dbg_r[2], st.dbg_r[4], st.dbg_last[0], st.dbg_last[1], st.dbg_last[2], st.dbg_last[3], st.dbg_last[4], st.dbg_last[5], st.dbg_last[6], st.dbg_last[7]);
    fprintf(stderr, "gpu decode: %llu rounds in two launches (dec_small_kernel); rounds outside the tail by node count:", (unsigned long long)st.small_rounds);
    for (int b = 0; b < 32; ++b) if (st.wide_hist[b]) fprintf(stderr, " [2^%d) %llu rounds %.1f M nodes %.3f s;", b, (unsigned long long)st.wide_hist[b], st.wide_nodes[b] * 1e-6, st.wide_time[b]);
    fprintf(stderr, "\n");
    fprintf(stderr, "gpu decode: tail kernels: wave %llu launches (%llu rounds, %llu nodes) %.3f s, workgroup %llu launches (%llu rounds, %llu nodes) %.3f s\n",
            (unsigned long long)st.launches_wave, (unsigned long long)st.rounds_wave, (unsigned long long)st.nodes_wave, st.t_wave,
            (unsigned long long)st.launches_wg, (unsigned long long)st.rounds_wg, (unsigned long long)st.nodes_wg, st.t_wg);
  }

  // From here on the lists and the rounds' query buffers are idle (an allocation that finds the device full gets them back:
  // ctx_trim).  Where what follows would not fit twice into the device memory that is free beside them, they go back now, so
  // that the planes and the inverse BWT never allocate on top of them: 16 lists of 541 M nodes and ~10 GB of query buffers at
  // 2^31 bytes.  At 10^8 bytes they stay with the context for its next decode.  (BCE_DEC_GIVE_BACK=1: always.)
  int give_back() {
    auto more = [](const DevBuf &b, size_t want) -> uint64_t { return want > b.cap ? want - b.cap : 0; };
    const size_t b4n = (size_t)n * 4, wb = (size_t)8 * plane_words(n) * 4;
    const uint64_t post = more(c->sa[0], std::max<size_t>(8 * rstride, b4n)) + more(c->sa[1], b4n) + more(c->key[0], std::max(wb, b4n)) +
                          more(c->key[1], std::max(wb, b4n)) + more(c->rank, b4n) + more(c->gran, (size_t)8 * plane_granules(n) * sizeof(Granule)) +
                          more(c->bwt, n) + (dest.own_text() ? more(c->text, n) : 0);
    size_t fr = 0, tot = 0;
    if (env.give_back || (hipMemGetInfo(&fr, &tot) == hipSuccess && fr < 2 * post)) {
      BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
      size_t freed = 0;
      for (auto &par : c->dlist) for (DevBuf &b : par) { freed += b.cap; release(b); }
      for (DevBuf *b : {&Qbuf, &Ebuf, &Rsbuf, &c->tilecnt, &c->tileoff}) { freed += b->cap; release(*b); }
      if (env.mem()) fprintf(stderr, "gpu decode: after the rounds: %.1f GB of node lists and query buffers given back (%.1f GB were free, the planes and the inverse BWT add %.1f GB)\n",
                             freed / 1e9, fr / 1e9, post / 1e9);
    }
    return BCE_HIP_OK;
  }

  // ---- R -> planes -> granules -> BWT bytes ----
  int planes() {
    BCE_TRY(planes_stage(c, a.R, n, a.zeros, dest.own_text(), peak()));
    if (env.timing) { BCE_HIP_TRY(c, hipStreamSynchronize(c->stream)); fprintf(stderr, "gpu decode: planes + unbwt %.3f s\n", now_s() - tp0); tp0 = now_s(); }
    return BCE_HIP_OK;
  }

  // ---- inverse BWT ----
  // The text is written where the destination wants it: into the context's buffer and copied to the host from there (kHost),
  // straight into the caller's device memory (kDevice), or into the context's buffer and compared there (kCompare).
  int inverse_bwt() {
    uint8_t *const text = dest.own_text() ? c->text.as<uint8_t>() : dest.out;
    uint64_t lc = 0;
    uint32_t walkers = 0;
    BCE_TRY(unbwt_stage(c, n, hd.offset % n, text, peak(), &lc, &walkers));
    const bool single_cycle = lc == n;
    if (dest.crc && dest.own_text()) BCE_TRY(checksum());
    if (dest.kind == DecDest::kHost) BCE_HIP_TRY(c, hipMemcpyAsync(dest.out, c->text.p, n, hipMemcpyDeviceToHost, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
    BCE_HIP_TRY(c, hipGetLastError());
    if (dest.kind == DecDest::kDevice && env.timing) fprintf(stderr, "gpu decode: text left on the device (%u B written in place, no copy to the host)\n", n);
    if (dest.kind == DecDest::kCompare) BCE_TRY(compare());
    if (env.timing) fprintf(stderr, "gpu decode: inverse BWT (%s, %u walkers) %.3f s\n", single_cycle ? "one cycle" : "periodic", walkers, now_s() - tp0);
    if (env.mem()) fprintf(stderr, "gpu decode: device memory in use over the whole decode (sampled after every allocation stage): %.1f GB at most\n", st.peak_used / 1e9);
    if (env.timing) fprintf(stderr, "gpu decode: this context so far: device allocations %u calls %.1f MB %.3f s, pinned (query / answer buffers) %u calls %.1f MB %.3f s\n",
                            c->alloc_calls, c->alloc_bytes / 1e6, c->alloc_s, c->pin_calls, c->pin_bytes / 1e6, c->pin_s);
    return BCE_HIP_OK;
  }

  // ---- kChecksum (and kHost with a checksum asked for): the CRC-32 of the decoded text, on the device (kd_crc32.hip) ----
  int checksum() {
    const double tc0 = now_s();
    uint32_t v = 0;
    BCE_TRY(kd_crc32(c, c->text.as<uint8_t>(), n, &v));
    *dest.crc = v;
    if (env.timing) fprintf(stderr, "gpu decode: CRC-32 of the %u B of text on the device: %.6f s\n", n, now_s() - tc0);
    return BCE_HIP_OK;
  }

  // ---- kCompare: the decoded text against the original, on the device (kd_compare.hip) ----
  // The common prefix is compared; where the sizes differ and the prefix agrees, the first index one of them lacks differs.
  int compare() {
    const double tc0 = now_s();
    const uint64_t m = std::min<uint64_t>(n, dest.orig_n);
    const uint8_t *orig = dest.orig_dev;
    if (!orig && m) {                                             // (the walk has read the BWT: its n bytes are free for the original)
      BCE_HIP_TRY(c, hipMemcpyAsync(c->bwt.p, dest.orig_host, m, hipMemcpyHostToDevice, c->stream));
      orig = c->bwt.as<uint8_t>();
    }
    uint64_t fd = UINT64_MAX;
    BCE_TRY(kd_compare(c, c->text.as<uint8_t>(), orig, m, &fd));
    if (fd == UINT64_MAX && dest.orig_n != n) fd = m;
    *dest.first_diff = fd;
    if (env.timing) fprintf(stderr, "gpu decode: text left on the device, compared there with %llu B %s: %.6f s\n", (unsigned long long)dest.orig_n,
                            dest.orig_dev ? "of device memory" : "uploaded from the host", now_s() - tc0);
    return BCE_HIP_OK;
  }
};

}  // namespace

}  // namespace bce

using namespace bce;

// `bce -d` on the GPU: archive -> original bytes (see the header of this file).  The context is only used for its
// device, stream and scratch buffers; any compression state in it is dropped.
// The text goes where `dest` says (DecDest): to the caller's host buffer, to the caller's device memory, or nowhere -- compared
// on the device with the original.  For the host destination the launches, copies and allocations are what they always were.
static int decompress_device(bce_hip_ctx *c, const uint8_t *archive, size_t len, const DecDest &dest, size_t *out_len) {
  if (!c) return BCE_HIP_E_ARG;
  PartEnd part_end{c};
  if (!archive || !out_len) return BCE_HIP_E_ARG;
  const bool cmp = dest.kind == DecDest::kCompare || dest.kind == DecDest::kChecksum;   // (no buffer of the caller's)
  if (dest.kind == DecDest::kChecksum && !dest.crc) return BCE_HIP_E_ARG;
  if (dest.crc && !dest.own_text()) return BCE_HIP_E_ARG;      // (the checksum is taken from the context's buffer: kDevice has none)
  if (dest.kind == DecDest::kCompare && (!dest.first_diff || (dest.orig_n && !dest.orig_dev && !dest.orig_host))) return BCE_HIP_E_ARG;
  ArchiveHead hd;
  if (parse_archive(archive, len, hd, /*header_only=*/true) != 0) return BCE_HIP_E_ARG;
  *out_len = hd.n;
  if (!cmp) {
    if (!dest.out) return BCE_HIP_OK;
    if (dest.cap < hd.n) return BCE_HIP_E_OVERFLOW;
  }
  if (parse_archive(archive, len, hd, false) != 0) return BCE_HIP_E_ARG;
  BCE_HIP_TRY(c, hipSetDevice(c->device));
  c->coder->drain();
  dec_drop_state(c);                                            // the scratch buffers below belong to the decoder now
  PhaseScope phase(c, 4);
  Decode d(c, hd, dest);
  c->dec_part = 1;
  BCE_TRY(d.setup(len));
  BCE_TRY(d.rounds());
  d.report_rounds();
  c->dec_part = 2;
  BCE_TRY(d.give_back());
  BCE_TRY(d.planes());
  c->dec_part = 3;                                              // (... and the boundary ranks, once access_kernel has read them)
  return d.inverse_bwt();
}

extern "C" int bce_hip_decompress_device(bce_hip_ctx *c, const uint8_t *archive, size_t len, uint8_t *out, size_t cap,
                                         size_t *out_len) {
  return bce_guarded(c, [&] { return decompress_device(c, archive, len, DecDest::to_host(out, cap), out_len); });
}

// The same decode with the text left in the caller's DEVICE memory (of the context's device, any alignment, cap bytes): the walk
// of the inverse BWT writes it there, nothing of it crosses to the host.
extern "C" int bce_hip_decompress_to_device(bce_hip_ctx *c, const uint8_t *archive, size_t len, void *d_out, size_t cap,
                                            size_t *out_len) {
  return bce_guarded(c, [&] { return decompress_device(c, archive, len, DecDest::to_device(d_out, cap), out_len); });
}

// Decode and compare with the original on the device: *first_diff = UINT64_MAX (equal), the first index that differs, or
// min(n, decoded size) when only the sizes differ.
extern "C" int bce_hip_verify_device(bce_hip_ctx *c, const uint8_t *archive, size_t len, const void *d_original, size_t n,
                                     uint64_t *first_diff) {
  return bce_guarded(c, [&] {
    if (n && !d_original) return (int)BCE_HIP_E_ARG;
    size_t decoded = 0;
    return decompress_device(c, archive, len, DecDest::compare_with(d_original, nullptr, n, first_diff), &decoded);
  });
}

extern "C" int bce_hip_verify_host(bce_hip_ctx *c, const uint8_t *archive, size_t len, const uint8_t *original, size_t n,
                                   uint64_t *first_diff) {
  return bce_guarded(c, [&] {
    if (n && !original) return (int)BCE_HIP_E_ARG;
    size_t decoded = 0;
    return decompress_device(c, archive, len, DecDest::compare_with(nullptr, original, n, first_diff), &decoded);
  });
}

// bce_hip_decompress_device that also reports the CRC-32 of the text: computed on the device from the context's buffer, before the
// copy to the host is queued (`bce -d` on a version-2 container).  out == NULL: only the size, *crc untouched.
extern "C" int bce_hip_decompress_device_crc32(bce_hip_ctx *c, const uint8_t *archive, size_t len, uint8_t *out, size_t cap,
                                               size_t *out_len, uint32_t *crc) {
  if (!c || !crc) return BCE_HIP_E_ARG;
  return bce_guarded(c, [&] {
    uint32_t v = 0;
    const int rc = decompress_device(c, archive, len, DecDest::to_host(out, cap, &v), out_len);
    if (rc == BCE_HIP_OK && out) *crc = v;
    return rc;
  });
}

// Decode into the context's own buffer and report the size and the CRC-32 of the text: nothing of it goes to the host, no second
// buffer is held (`bce -t archive` on a version-2 container).
extern "C" int bce_hip_decode_crc32(bce_hip_ctx *c, const uint8_t *archive, size_t len, size_t *decoded, uint32_t *crc) {
  if (!c || !crc || !decoded) return BCE_HIP_E_ARG;
  return bce_guarded(c, [&] {
    uint32_t v = 0;
    size_t n = 0;
    const int rc = decompress_device(c, archive, len, DecDest::checksum_only(&v), &n);
    if (rc == BCE_HIP_OK) { *decoded = n; *crc = v; }
    return rc;
  });
}
