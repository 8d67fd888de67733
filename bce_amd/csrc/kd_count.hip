// kd_count.hip -- how often byte strings occur in the circular text, from the K2 planes (bce_hip_count / _count_device, `bce -g`).
//
// After K1 and K2 the context holds a counting index of its input: the BWT of all cyclic rotations as an LSB-first wavelet
// matrix with a rank directory.  Backward search (fm_step.h) narrows the interval (lo, hi) = (0, n) by one last-to-first step
// per pattern byte, last byte first; hi - lo at the end is the number of rotations that start with the pattern.
//   - One lane per pattern.  A step is eight levels, a level two rank granules (one for lo, one for hi): two independent
//     16-byte loads issued together, then the next level's addresses depend on them.  So a pattern of m bytes is a chain of
//     8 m dependent gathers, and the kernel is bound by their latency: what hides it is waves, not work per lane.  The kernel
//     needs few registers and no LDS, so eight waves per SIMD are resident.
//   - The next pattern byte is loaded before the current byte's eight levels, off the chain.
//   - A lane whose interval is empty stops; its wave goes on until all its lanes are done.
//   - lo and hi stay in [0, n] on every level (a one-bit lands at zeros[j] + rank1 <= n, a zero-bit at i - rank1 <= zeros[j]),
//     and K2 lays out granules for n + 1 positions: every granule index is below ngran, whatever the pattern's bytes.
//   - Nothing is written but one 8-byte count per lane, and a flag word when two offsets decrease.
#include "common.h"
#include "fm_step.h"

namespace bce {

namespace {

constexpr int CNT_T = 256;                   // lanes per workgroup (4 waves)

struct Zeros8 { uint32_t v[8]; };

__global__ __launch_bounds__(CNT_T) void count_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, Zeros8 z,
                                                      const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off,
                                                      uint32_t npat, uint64_t *__restrict__ out, uint32_t *__restrict__ bad) {
  const uint32_t p = blockIdx.x * CNT_T + threadIdx.x;
  if (p >= npat) return;
  const uint64_t b = off[p], e = off[(size_t)p + 1];
  if (e < b) { *bad = 1u; out[p] = 0; return; }                   // (every lane that sees it stores the same word)
  uint32_t lo = 0, hi = n;
  uint32_t c = e > b ? pat[e - 1] : 0u;
  for (uint64_t k = e; k > b && lo < hi; --k) {
    const uint32_t next = k - 1 > b ? pat[k - 2] : 0u;
    fm_step(c, z.v, lo, hi, [&](int j, uint32_t ia, uint32_t ib, uint32_t &ra, uint32_t &rb) {
      const Granule *G = gran + (size_t)j * ngran;                // (64-bit: 8 ngran passes 2^32 granule bytes long before n = 2^31)
      const uint32_t ga = div96(ia), gb = div96(ib);
      const Granule qa = G[ga], qb = G[gb];                       // both loads go out before either rank
      ra = granule_rank1(qa, ia - ga * 96u);
      rb = granule_rank1(qb, ib - gb * 96u);
    });
    c = next;
  }
  out[p] = hi - lo;
}

}  // namespace

// d_out[p] = occurrences of d_pat[d_off[p], d_off[p + 1]) in the circular text of the context's planes, p < npat.  All three
// arrays: device memory of the context's device.  Queued on the context's stream behind whatever wrote them; returns when the
// kernel is through (the flag word's way back is the wait, as kd_compare's result word).  Offsets that decrease: BCE_HIP_E_ARG.
int kd_count(bce_hip_ctx *c, const uint8_t *d_pat, const uint64_t *d_off, uint32_t npat, uint64_t *d_out) {
  if (npat == 0) return BCE_HIP_OK;
  BCE_TRY(ensure(c, c->qbuf[qb::cnt_res], 8));
  uint32_t *d_bad = c->qbuf[qb::cnt_res].as<uint32_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
  Zeros8 z;
  memcpy(z.v, c->zeros, sizeof z.v);
  const uint32_t grid = (uint32_t)(((uint64_t)npat + CNT_T - 1) / CNT_T);
  hipLaunchKernelGGL(count_kernel, dim3(grid), dim3(CNT_T), 0, c->stream, c->gran.as<Granule>(), c->ngran, c->n, z, d_pat, d_off, npat,
                     d_out, d_bad);
  BCE_HIP_TRY(c, hipGetLastError());
  uint32_t bad = 0;
  BCE_TRY(read_back(c, &bad, d_bad, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  if (bad) { snprintf(c->err, sizeof c->err, "count: pattern offsets decrease"); return BCE_HIP_E_ARG; }
  return BCE_HIP_OK;
}

}  // namespace bce
