// k4_cost.hip -- the archive's size without coding it: the sum of the model's code lengths, taken where K4 left them.
//
// K4 (k4_model.hip) leaves one packed (cum, freq, total, escape bits) record per symbol in `sout`, in stream order (round, plane,
// s).  What the host coder would do with a record -- one uniform bit per escape bit, then set(cum, freq, total)
// (host_coder.cpp, RangeCoder::encode_run) -- narrows its range by a known factor, so the length of plane p's stream is the sum of
// log2(total / freq) over p's records (bce_cost.h: Q24 integers, the same words on host and device).  One pass over the 8 bytes per
// record that are already in HBM gives the eight sums; no device-to-host copy, no flush slot, no coder thread.
//
// Which plane a record belongs to is not in the record: it is its place in the stream.  The host knows the flush's runs
// (bce_hip_ctx::run_log: per (round, plane) one [start, start + count)); sorted by start they tile [0, nsym), and the kernel gets
// their starts and planes.  A workgroup takes tiles of KC_TILE consecutive records.  A tile that lies inside ONE run -- the
// wide rounds, where a run has 10^5 .. 10^7 records: nearly every record of a large input -- is summed in registers, reduced in
// the wave by shuffles and added once per wave to the workgroup's sums in LDS.  A tile that holds a run boundary (narrow rounds, the
// tail) goes wave by wave: 64 consecutive records inside one run are reduced the same way, and only a wave that holds a boundary
// itself looks every lane's run up and adds lane by lane.  At the end one 64-bit
// atomic per plane and workgroup goes to the sixteen words in device memory: integer sums, so the order does not matter.
#include "bce_cost.h"
#include "common.h"

#include <algorithm>

namespace bce {

constexpr int KC_T = 256;                  // threads per workgroup
constexpr int KC_PER = 8;                  // records per thread and tile: 8 loads in flight per lane
constexpr uint32_t KC_TILE = KC_T * KC_PER;

struct K4CostArgs {
  const uint64_t *out;                     // K4's records of this flush, [nsym]
  const uint32_t *starts;                  // [nruns] first record of each run, ascending, starts[0] = 0
  const uint8_t *planes;                   // [nruns]
  unsigned long long *acc;                 // [0..7] cost sums (Q24), [8..15] record counts
  uint32_t nruns, nsym;
};

// the last run in [lo, hi] that starts at or before record i (starts[lo] <= i)
__device__ __forceinline__ uint32_t kc_run_of(const uint32_t *__restrict__ starts, uint32_t lo, uint32_t hi, uint32_t i) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (starts[mid] <= i) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

__device__ __forceinline__ uint64_t kc_wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;                                // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(KC_T) void k4_cost_kernel(K4CostArgs a) {
  __shared__ uint32_t tab[kLog2Steps + 1];
  __shared__ unsigned long long sacc[16];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t i = tid; i <= kLog2Steps; i += KC_T) tab[i] = kLog2TableDev.t[i];
  if (tid < 16) sacc[tid] = 0;
  __syncthreads();
  const uint32_t ntiles = (a.nsym + KC_TILE - 1u) / KC_TILE;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t t0 = tile * KC_TILE, t1 = a.nsym - t0 < KC_TILE ? a.nsym : t0 + KC_TILE;
    uint64_t rec[KC_PER];
#pragma unroll
    for (int j = 0; j < KC_PER; ++j) {     // a wave's load covers 512 contiguous bytes
      const uint32_t i = t0 + (uint32_t)j * KC_T + tid;
      rec[j] = i < t1 ? a.out[i] : 0ull;
    }
    const uint32_t r0 = kc_run_of(a.starts, 0, a.nruns - 1u, t0);       // (the same for every lane)
    const uint32_t r1 = kc_run_of(a.starts, r0, a.nruns - 1u, t1 - 1u);
    if (r0 == r1) {
      uint64_t cost = 0;
      uint32_t cnt = 0;
#pragma unroll
      for (int j = 0; j < KC_PER; ++j) {
        const uint32_t i = t0 + (uint32_t)j * KC_T + tid;
        if (i < t1) { cost += record_cost_q24_with(tab, rec[j]); ++cnt; }
      }
      cost = kc_wave_sum64(cost);
      const uint64_t n = kc_wave_sum64((uint64_t)cnt);
      if (lane == 0 && n) {
        const uint32_t p = a.planes[r0] & 7u;
        atomicAdd(&sacc[p], (unsigned long long)cost);
        atomicAdd(&sacc[8 + p], (unsigned long long)n);
      }
    } else {
      // a run boundary in the tile: wave by wave, 64 consecutive records each.  A wave's records inside one run -- every run of
      // 64 records and more has such waves -- are reduced like a tile's; only a wave that holds a boundary itself looks each
      // lane's run up, between the wave's first and last run, and adds lane by lane.
#pragma unroll
      for (int j = 0; j < KC_PER; ++j) {
        const uint32_t w0 = t0 + (uint32_t)j * KC_T + (tid & ~63u);   // the wave's first record (the same for its lanes)
        if (w0 >= t1) continue;
        const uint32_t w1 = t1 - w0 < 64u ? t1 - 1u : w0 + 63u, i = w0 + lane;
        const uint32_t ra = kc_run_of(a.starts, r0, r1, w0), rb = kc_run_of(a.starts, ra, r1, w1);
        const uint32_t cst = i < t1 ? record_cost_q24_with(tab, rec[j]) : 0u;
        if (ra == rb) {
          const uint64_t cost = kc_wave_sum64((uint64_t)cst);
          if (lane == 0) {
            const uint32_t p = a.planes[ra] & 7u;
            atomicAdd(&sacc[p], (unsigned long long)cost);
            atomicAdd(&sacc[8 + p], (unsigned long long)(w1 - w0 + 1u));
          }
        } else if (i < t1) {
          const uint32_t p = a.planes[kc_run_of(a.starts, ra, rb, i)] & 7u;
          atomicAdd(&sacc[p], (unsigned long long)cst);
          atomicAdd(&sacc[8 + p], 1ull);
        }
      }
    }
  }
  __syncthreads();
  if (tid < 16 && sacc[tid]) atomicAdd(&a.acc[tid], sacc[tid]);
}

// the flush's kernels run on this stream (k4_flush_async makes the same choice)
static hipStream_t k4_cost_stream(bce_hip_ctx *c) { return (c->overlap && c->k4_stream && !c->scan_mode) ? c->k4_stream : c->stream; }

int k4_cost_begin(bce_hip_ctx *c) {
  BCE_TRY(ensure(c, c->cost_acc, 16 * sizeof(uint64_t)));
  // (an estimate that failed midway may have left a cost kernel on the model's own stream: nothing of it adds to these zeros)
  if (c->k4_stream) BCE_HIP_TRY(c, hipStreamSynchronize(c->k4_stream));
  BCE_HIP_TRY(c, hipMemsetAsync(c->cost_acc.p, 0, 16 * sizeof(uint64_t), c->stream));
  // (a flush on the model's own stream waits for the main stream's rounds first: the zeros are there before any sum)
  return BCE_HIP_OK;
}

// Behind k4_flush_async(..., copy_out = false) of the same nsym records: add their costs to the context's sums.  `slot` lends
// its events: ev_copy, which in an encode follows the records' copy, follows the cost kernel here (account_slot: t_model).
int k4_cost_async(bce_hip_ctx *c, uint64_t nsym64, FlushSlot &slot) {
  if (nsym64 == 0) return BCE_HIP_OK;
  const uint32_t nsym = (uint32_t)nsym64;                              // (< 2^31: k4_flush_async has checked)
  // the flush's runs in stream order; they must tile [0, nsym)
  struct Run { uint64_t start; uint32_t count, plane; };
  std::vector<Run> runs;
  size_t total = 0;
  for (int p = 0; p < 8; ++p) total += c->run_log[p].size();
  runs.reserve(total);
  for (int p = 0; p < 8; ++p)
    for (const RunEntry &e : c->run_log[p])
      if (e.count) runs.push_back(Run{e.start, e.count, (uint32_t)p});
  std::sort(runs.begin(), runs.end(), [](const Run &x, const Run &y) { return x.start < y.start; });
  uint64_t at = 0;
  for (const Run &r : runs) {
    if (r.start != at) break;
    at += r.count;
  }
  if (at != nsym64 || runs.empty()) {
    snprintf(c->err, sizeof c->err, "k4 cost: the runs of this flush do not tile its %llu records", (unsigned long long)nsym64);
    return BCE_HIP_E_INTERNAL;
  }
  // starts | planes, through pinned memory of the slot (its last use is over: the caller has waited for the slot's ev_copy)
  const size_t nruns = runs.size(), planes_off = nruns * sizeof(uint32_t), bytes = planes_off + nruns;
  if (slot.h_cost_runs_cap < bytes) {
    if (slot.h_cost_runs) { (void)hipHostFree(slot.h_cost_runs); slot.h_cost_runs = nullptr; slot.h_cost_runs_cap = 0; }
    const size_t cap = bytes < 4096 ? 4096 : bytes + bytes / 2;
    BCE_TRY(pin_alloc(c, &slot.h_cost_runs, cap));
    slot.h_cost_runs_cap = cap;
  }
  uint8_t *host = static_cast<uint8_t *>(slot.h_cost_runs);
  for (size_t i = 0; i < nruns; ++i) {
    reinterpret_cast<uint32_t *>(host)[i] = (uint32_t)runs[i].start;
    host[planes_off + i] = (uint8_t)runs[i].plane;
  }
  hipStream_t ks = k4_cost_stream(c);
  BCE_TRY(ensure(c, c->cost_runs, bytes < 4096 ? 4096 : bytes + bytes / 2));
  // (on the stream the copy follows the cost kernel of the flush before, the last reader of the table it replaces)
  BCE_HIP_TRY(c, hipMemcpyAsync(c->cost_runs.p, host, bytes, hipMemcpyHostToDevice, ks));
  K4CostArgs a;
  a.out = c->sout.as<uint64_t>();
  a.starts = c->cost_runs.as<uint32_t>();
  a.planes = c->cost_runs.as<uint8_t>() + planes_off;
  a.acc = c->cost_acc.as<unsigned long long>();
  a.nruns = (uint32_t)nruns; a.nsym = nsym;
  const uint32_t ntiles = (nsym + KC_TILE - 1u) / KC_TILE;
  const uint32_t grid = ntiles < 2048u ? ntiles : 2048u;
  hipLaunchKernelGGL(k4_cost_kernel, dim3(grid), dim3(KC_T), 0, ks, a);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_HIP_TRY(c, hipEventRecord(slot.ev_copy, ks));
  return BCE_HIP_OK;
}

// the sixteen words, once everything queued has run
int k4_cost_end(bce_hip_ctx *c, uint64_t acc[16]) {
  if (c->k4_stream) BCE_HIP_TRY(c, hipStreamSynchronize(c->k4_stream));
  return read_back(c, acc, c->cost_acc.p, 16 * sizeof(uint64_t));
}

}  // namespace bce
