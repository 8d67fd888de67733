// kd_host_tail.hip -- the GPU-assisted decoder's tail rounds on the host (Decode::to_host in kd_decode.hip decides when).
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "kd_decode.h"

namespace bce {

namespace {

// The very deep tail on the host.  A chain of a few nodes that goes on for millions of rounds (a megabyte run, a
// whole-file duplicate) costs the wave kernel ~2 us per round -- the latency of one dependent load after the other
// -- while a CPU core does the same round out of its caches in ~0.1 us.  So once the wave kernel has spent
// max(kHostTailMin, n / 2500) rounds on <= 64 nodes, the boundary ranks (8 x 4(n+1) B) and the node lists come to the host, the rounds
// are finished here exactly as `bce -ds` runs them (decoder.cpp, BCE::code mode 0, bce.cpp:1246-1371, same decoders),
// and the ranks go back for the plane fill.  The copies are ~2 x 60 ms per 10^8 bytes.
__global__ void dec_scatter_kernel(uint32_t *__restrict__ R, const uint64_t *__restrict__ idx, const uint32_t *__restrict__ val, uint64_t m) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) R[idx[i]] = val[i];
}

}  // namespace

// Eight CPUs of the calling thread's L3 domain that its affinity mask allows (empty: fewer than eight, or no sysfs):
// where the eight threads of dec_host_tail sit so that their per-round barrier stays inside one CCX.
std::vector<int> tail_cpus(const DecEnv &env) {
  std::vector<int> ccx;
  cpu_set_t aff;
  if (env.tail_nopin || sched_getaffinity(0, sizeof aff, &aff) != 0) return ccx;
  char path[128];
  snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", sched_getcpu());
  if (FILE *f = fopen(path, "r")) {
    char buf[512] = {0};
    if (fgets(buf, sizeof buf, f)) {
      for (char *q = buf; *q && ccx.size() < 8;) {
        char *e;
        long lo = strtol(q, &e, 10), hi = lo;
        if (e == q) break;
        if (*e == '-') { q = e + 1; hi = strtol(q, &e, 10); }
        for (long v = lo; v <= hi && ccx.size() < 8; ++v) if (v >= 0 && v < CPU_SETSIZE && CPU_ISSET((int)v, &aff)) ccx.push_back((int)v);
        if (*e != ',') break;
        q = e + 1;
      }
    }
    fclose(f);
  }
  if (ccx.size() != 8) ccx.clear();
  return ccx;
}

// The host tail's pinned copy of the boundary ranks is 32 (n + 1) bytes; pinning them takes ~0.15 s per GB the first time a
// context needs them (3.2 GB at 10^8 bytes: 0.5 s, a third of a whole decode).  Once a decode looks like it will end in
// a long tail (see the caller) the allocation is started on a thread of its own, beside the GPU's rounds.
// (struct BigPin: kd_decode.h -- a Decode holds one)
void BigPin::start(bce_hip_ctx *ctx, size_t want) {
  if (running || ctx->h_big_cap >= want) return;
  c = ctx; bytes = want;
  const int dev = ctx->device;
  try {
    t_start = now_s();
    th = std::thread([this, dev] { p = big_host_alloc(bytes, dev, &registered); t_done = now_s(); });
    running = true;
  } catch (...) { running = false; }                          // (no thread: dec_host_tail allocates as before)
}
void BigPin::settle() {                                        // the buffer, if it came, becomes the context's
  if (!running) return;
  const double t0 = now_s();
  th.join();
  running = false;
  if (timing) fprintf(stderr, "gpu decode: pinned %.1f GB beside the rounds: %.3f s, the tail waited %.3f s of them\n", bytes / 1e9, t_done - t_start, now_s() - t0);
  if (p) {
    if (c->h_big) big_host_free(c, c->h_big, c->h_big_cap, c->h_big_registered);
    c->h_big = p; c->h_big_cap = bytes; c->h_big_registered = registered; p = nullptr;
    if (registered) c->reg_maps++;
  }
}

int dec_host_tail(bce_hip_ctx *c, const DecEnv &env, const DecArgs &a, const DecCtl &ctl, std::vector<Decoder> &dec, uint32_t n,
                  uint32_t *round, uint64_t *nodes_total, uint64_t *queries_total, bool *bad_out) {
  const uint32_t par = *round & 1u;
  std::vector<Node> cur[8][2], nxt[8][2];
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint32_t p = 0; p < 8; ++p) {
    const uint32_t c0 = ctl.cnt[par][p][0], c1 = ctl.cnt[par][p][1];
    const Node *base = a.list[par][p];
    cur[p][0].resize(c0);
    if (c0) BCE_HIP_TRY(c, hipMemcpy(cur[p][0].data(), base, (size_t)c0 * sizeof(Node), hipMemcpyDeviceToHost));
    cur[p][1].resize(c1);
    if (c1) {
      BCE_HIP_TRY(c, hipMemcpy(cur[p][1].data(), base + (a.cap[par][p] - c1), (size_t)c1 * sizeof(Node), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < c1 / 2; ++i) std::swap(cur[p][1][i], cur[p][1][c1 - 1u - i]);     // child1 lists grow downwards
    }
  }
  const size_t stride = (size_t)n + 1;
  // 3.2 GB at 10^8 bytes: into pinned memory the context keeps (a copy into fresh pageable memory ran at a fifth of the bus)
  const double tcp0 = now_s();
  if (c->h_big_cap < 8 * stride * 4) {
    if (c->h_big) { big_host_free(c, c->h_big, c->h_big_cap, c->h_big_registered); c->h_big = nullptr; c->h_big_cap = 0; }
    c->h_big = big_host_alloc(8 * stride * 4, c->device, &c->h_big_registered);
    if (c->h_big && c->h_big_registered) c->reg_maps++;
    if (!c->h_big) { snprintf(c->err, sizeof c->err, "host tail: no pinned memory for the boundary ranks"); return BCE_HIP_E_NOMEM; }
    c->h_big_cap = 8 * stride * 4;
  }
  uint32_t *Rh = static_cast<uint32_t *>(c->h_big);
  const double tcp1 = now_s();
  BCE_HIP_TRY(c, hipMemcpyAsync(Rh, a.R, 8 * stride * 4, hipMemcpyDeviceToHost, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (env.timing) fprintf(stderr, "gpu decode: host tail: pinned buffer %.3f s, boundary ranks to the host %.3f s (%.1f GB)\n", tcp1 - tcp0, now_s() - tcp1, 8 * stride * 4 / 1e9);
  // what the host learns goes back as (index, value) pairs, kept per plane (the planes are worked on side by side)
  // (each plane's output on cache lines of its own: the headers of neighbouring std::vectors share a line, and eight threads
  //  appending to neighbouring vectors took 13 us per round for what is 3 us of work)
  struct alignas(128) PlaneOut {
    std::vector<Node> o0, o1;                  // the children: next round's lists of plane i + 1
    std::vector<uint64_t> wi;
    std::vector<uint32_t> wv;
    uint64_t nodes = 0, queries = 0;
  };
  std::unique_ptr<PlaneOut[]> po(new PlaneOut[8]);
  // beyond that many pairs (per plane) the whole array goes back: the pinned copy runs at the bus' rate (3.2 GB in 56 ms),
  // while a pair costs two appends here, a place in two pageable arrays and a scattered store there (~7 ns: 18 M pairs of
  // the natural corpus took longer than the whole array)
  const size_t pairs_max = std::min<size_t>(stride / 8 + 1, (size_t)1 << 18);
  std::atomic<bool> bad_flag{false};
  // One plane of one round (BCE::code mode 0, bce.cpp:1261-1351): reads and writes plane i's boundary ranks only, appends to the
  // lists of plane i + 1 only -- the planes of a round are independent, which is the reference's own OpenMP split (:1250-1252).
  auto do_plane = [&](uint32_t i) {
    uint32_t *R = Rh + (size_t)i * stride;
    const uint32_t zi = a.zeros[i];
    PlaneOut &P = po[i];
    // a child is plane i + 1's node in the NEXT round: its three boundary ranks are asked for now (two random lines of a
    // 4(n + 1)-byte array: DRAM), so that they are in the cache (this core's, or the L3 it shares with the plane's thread)
    // by the time the round gets there -- in the chains a round is ~10 nodes and was mostly waiting for these lines
    const uint32_t *Rn = Rh + (size_t)((i + 1u) & 7u) * stride;
    auto ask = [&](uint32_t cs, uint32_t cx0, uint32_t cx1) {
      __builtin_prefetch(Rn + cs, 0, 3);
      __builtin_prefetch(Rn + cs + cx0 + cx1, 0, 3);
      __builtin_prefetch(Rn + cs + cx0, 1, 3);
    };
    std::vector<Node> &o0 = P.o0, &o1 = P.o1;
    std::vector<uint64_t> &wi = P.wi;
    std::vector<uint32_t> &wv = P.wv;
    uint64_t nn = 0, qq = 0;
    for (int j = 0; j < 2; ++j)
      for (const Node &nd : cur[i][j]) {
        const uint32_t s = nd.s, x0 = nd.x0, x1 = nd.x1, x = x0 + x1;
        if ((uint64_t)s + x > n || R[s] == kUnknown || R[s + x] == kUnknown) { bad_flag.store(true); return; }
        const uint32_t s1 = R[s], n1x = R[s + x] - s1, s0 = s - s1;
        if (n1x > x) { bad_flag.store(true); return; }
        uint32_t n1x0;
        if (!n1x) { o0.push_back(Node{s0, x0, x1}); ask(s0, x0, x1); n1x0 = 0; }
        else if (n1x == x) { o1.push_back(Node{zi + s1, x0, x1}); ask(zi + s1, x0, x1); n1x0 = x0; }
        else {
          const uint32_t n0x = x - n1x;
          uint32_t mn = x0 - n1x, mx = n1x - x1;
          mn = ((int32_t)mn < 0) ? 0u : mn;
          mx = ((int32_t)mx < 0) ? 0u : mx;
          mx = x0 - mx;
          uint32_t n0x0 = mn;
          if (mx != mn) { n0x0 = mn + dec[i].get_adaptive(mx - mn + 1, n0x, x1, x); ++qq; }
          if (n0x0 > mx) { bad_flag.store(true); return; }
          const uint32_t n0x1 = n0x - n0x0;
          if (n0x0 && n0x1) { o0.push_back(Node{s0, n0x0, n0x1}); ask(s0, n0x0, n0x1); }
          const uint32_t n1x1 = x1 - n0x1;
          n1x0 = n1x - n1x1;
          if (n1x0 && n1x1) { o1.push_back(Node{zi + s1, n1x0, n1x1}); ask(zi + s1, n1x0, n1x1); }
        }
        R[s + x0] = s1 + n1x0;
        if (wi.size() <= pairs_max) { wi.push_back((uint64_t)i * stride + s + x0); wv.push_back(s1 + n1x0); }
        ++nn;
      }
    P.nodes += nn; P.queries += qq;
  };
  // Rounds of a few nodes run on this thread (a round of two nodes is ~0.2 us: no barrier is worth that); from kParMin nodes
  // on the eight planes go to eight threads -- this one and seven helpers that spin on the round number (and doze off when
  // nothing has come for a while).  The GPU's resident tail kernels managed 35-160 ns per node on such rounds (dependent
  // loads, a mailbox round trip per query round); a host core does a node in ~40-100 ns, eight of them side by side.
  constexpr size_t kParMin = 16;              // (a round on eight threads costs ~1 us of barrier; a node ~0.1 us)
  constexpr uint32_t kParkAfter = 4096;       // serial rounds in a row after which the helpers stop spinning
  struct Pool {
    std::atomic<uint64_t> epoch{0};
    std::atomic<uint32_t> done{0};
    std::atomic<bool> quit{false}, parked{false};
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::thread> th;
  } pool;
  bool threaded = !env.tail_serial && std::thread::hardware_concurrency() >= 8u;
  // The eight threads meet at a barrier every round: on cores that share an L3 (one CCX of the EPYC hosts) that is ~1 us, across
  // the package 4-5 us -- more than the round's work.  So for the duration of the tail they sit on eight CPUs of this
  // thread's L3 domain, if the affinity mask has that many (otherwise wherever the scheduler puts them).
  std::vector<int> ccx;
  cpu_set_t old_aff;
  bool repin = false;
  if (threaded && sched_getaffinity(0, sizeof old_aff, &old_aff) == 0) {
    ccx = tail_cpus(env);
    if (ccx.size() == 8) {
      cpu_set_t one; CPU_ZERO(&one); CPU_SET(ccx[0], &one);
      repin = sched_setaffinity(0, sizeof one, &one) == 0;
    }
  }
  struct Unpin { bool on; cpu_set_t *aff; ~Unpin() { if (on) (void)sched_setaffinity(0, sizeof *aff, aff); } } unpin{repin, &old_aff};
  if (env.timing) fprintf(stderr, "gpu decode: host tail on %s\n", !threaded ? "one thread" : repin ? "eight threads of one L3 domain" : "eight threads, not pinned");
  if (threaded) try {
    for (uint32_t w = 1; w < 8; ++w)
      pool.th.emplace_back([&, w] {
        if (repin) { cpu_set_t one; CPU_ZERO(&one); CPU_SET(ccx[w], &one); (void)sched_setaffinity(0, sizeof one, &one); }
        uint64_t seen = 0;
        for (;;) {
          const uint64_t e = pool.epoch.load(std::memory_order_acquire);
          if (e != seen) {
            seen = e;
            do_plane(w);
            pool.done.fetch_add(1, std::memory_order_release);
            continue;
          }
          if (pool.quit.load(std::memory_order_acquire)) return;
          if (pool.parked.load(std::memory_order_acquire)) {             // the chains have begun: sleep until rounds get wide again
            std::unique_lock<std::mutex> lk(pool.mu);
            pool.cv.wait(lk, [&] { return !pool.parked.load() || pool.quit.load(); });
            continue;
          }
          __builtin_ia32_pause();
        }
      });
  } catch (...) {                                                          // no threads to be had: the rounds run on this one
    { std::lock_guard<std::mutex> lk(pool.mu); pool.quit.store(true, std::memory_order_release); }
    pool.cv.notify_all();
    for (auto &t : pool.th) t.join();
    pool.th.clear();
    threaded = false;
  }
  uint64_t par_rounds = 0, par_nodes = 0, ser_nodes = 0;
  double par_time = 0, ser_time = 0;
  uint32_t rounds = 0, serial_run = 0;
  auto unpark = [&] { { std::lock_guard<std::mutex> lk(pool.mu); pool.parked.store(false); } pool.cv.notify_all(); };
  // `live`: the planes that have nodes this round.  The chains of the deep tail are a node or two in one or two planes for
  // hundreds of thousands of rounds: such a round touches those planes' lists only (a round over all eight planes' sixteen
  // lists, empty or not, cost more than its two nodes).
  uint32_t live = 0;
  for (uint32_t i = 0; i < 8; ++i) if (!cur[i][0].empty() || !cur[i][1].empty()) live |= 1u << i;
  while (live && !bad_flag.load(std::memory_order_relaxed)) {
    size_t tot = 0;
    for (uint32_t m = live; m; m &= m - 1) { const int i = __builtin_ctz(m); tot += cur[i][0].size() + cur[i][1].size(); }
    const bool par_round = threaded && tot >= kParMin;
    const double tr0 = env.timing && (par_round || (rounds & 63u) == 0) ? now_s() : 0.0;
    if (par_round) {
      if (pool.parked.load(std::memory_order_relaxed)) unpark();
      serial_run = 0;
      pool.done.store(0, std::memory_order_relaxed);
      pool.epoch.fetch_add(1, std::memory_order_release);
      do_plane(0);
      while (pool.done.load(std::memory_order_acquire) < 7u) __builtin_ia32_pause();
      ++par_rounds;
    } else {
      for (uint32_t m = live; m && !bad_flag.load(std::memory_order_relaxed); m &= m - 1) do_plane((uint32_t)__builtin_ctz(m));
      if (threaded && ++serial_run == kParkAfter) pool.parked.store(true, std::memory_order_release);
    }
    if (env.timing) {                                                     // (serial rounds: one in 64 is timed -- the clock costs as much as the round)
      if (par_round) { par_time += now_s() - tr0; par_nodes += tot; }
      else { if ((rounds & 63u) == 0) ser_time += 64.0 * (now_s() - tr0); ser_nodes += tot; }
    }
    ++rounds;
    uint32_t next_live = 0;
    for (uint32_t m = live; m; m &= m - 1) {                               // plane i's children are plane i + 1's nodes
      const int i = __builtin_ctz(m), q = (i + 1) & 7;
      cur[q][0].swap(po[i].o0); po[i].o0.clear();
      cur[q][1].swap(po[i].o1); po[i].o1.clear();
      if (!cur[q][0].empty() || !cur[q][1].empty()) next_live |= 1u << q;
    }
    for (uint32_t m = live; m; m &= m - 1) {                               // a plane that was worked on and got nothing new
      const int q = __builtin_ctz(m);
      if (!((live >> ((q + 7) & 7)) & 1u)) { cur[q][0].clear(); cur[q][1].clear(); }
    }
    live = next_live;
  }
  { std::lock_guard<std::mutex> lk(pool.mu); pool.quit.store(true, std::memory_order_release); }
  pool.cv.notify_all();
  for (auto &t : pool.th) t.join();
  const bool bad = bad_flag.load();
  uint64_t nodes = 0, queries = 0;
  bool whole = false;
  std::vector<uint64_t> widx;
  std::vector<uint32_t> wval;
  for (int i = 0; i < 8; ++i) {
    nodes += po[i].nodes; queries += po[i].queries;
    if (po[i].wi.size() > pairs_max) whole = true;
  }
  if (!whole)
    for (int i = 0; i < 8; ++i) { widx.insert(widx.end(), po[i].wi.begin(), po[i].wi.end()); wval.insert(wval.end(), po[i].wv.begin(), po[i].wv.end()); }
  if (env.timing) fprintf(stderr, "gpu decode: host tail: %llu of %u rounds on eight threads (%llu nodes, %.3f s), the others on one (%llu nodes, %.3f s)\n",
                           (unsigned long long)par_rounds, rounds, (unsigned long long)par_nodes, par_time, (unsigned long long)ser_nodes, ser_time);
  *bad_out = bad;
  if (bad) return BCE_HIP_OK;
  const double tcp2 = now_s();
  if (env.timing) fprintf(stderr, "gpu decode: host tail: %u rounds, %llu nodes in %.3f s\n", rounds, (unsigned long long)nodes, tcp2 - tcp0);
  if (whole) {                                                           // (more than an eighth of everything: the whole array)
    BCE_HIP_TRY(c, hipMemcpyAsync(a.R, Rh, 8 * stride * 4, hipMemcpyHostToDevice, c->stream));
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else if (!widx.empty()) {
    const size_t m = widx.size();
    BCE_TRY(ensure(c, c->skey[0], m * 8));
    BCE_TRY(ensure(c, c->skey[1], m * 4));
    BCE_HIP_TRY(c, hipMemcpy(c->skey[0].p, widx.data(), m * 8, hipMemcpyHostToDevice));
    BCE_HIP_TRY(c, hipMemcpy(c->skey[1].p, wval.data(), m * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(dec_scatter_kernel, dim3((unsigned)((m + 255) / 256 < 4096 ? (m + 255) / 256 : 4096)), dim3(256), 0, c->stream,
                       a.R, c->skey[0].as<uint64_t>(), c->skey[1].as<uint32_t>(), (uint64_t)m);
    BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
    BCE_HIP_TRY(c, hipGetLastError());
  }
  *round += rounds; *nodes_total += nodes; *queries_total += queries;
  return BCE_HIP_OK;
}

}  // namespace bce
