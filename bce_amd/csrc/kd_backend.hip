// kd_backend.hip -- the back end of the GPU-assisted decoder: boundary ranks R -> plane bits -> rank granules -> BWT bytes ->
// text (planes_stage, unbwt_stage: Decode::planes / inverse_bwt in kd_decode.hip; alone: the two test hooks at the end), and
// the libdivsufsort seam's inverse_bw_transform, which shares the inverse BWT's walk.
#include <stdio.h>

#include <vector>

#include "kd_decode.h"

namespace bce {

namespace {

// ---------------------------------------------------------------------------------------------------------
// After the last round: R -> plane bits -> rank granules.  Between two known boundaries a < b a plane is
// constant: all ones iff R[b] - R[a] == b - a, all zeros iff R[b] == R[a] (anything else: inconsistent archive).
// ---------------------------------------------------------------------------------------------------------
constexpr int FG_T = 256;
constexpr uint32_t FG_PER = 32;                        // positions per thread = one 32-bit word of the plane
constexpr uint32_t FG_CHUNK = FG_T * FG_PER;           // 8192 positions per block

struct FillArgs {
  const uint32_t *R;        // [8][n + 1]
  uint32_t *cmax;           // [8][chunks]: last known index + 1 inside the chunk (0 = none), then its exclusive prefix max
  uint8_t *type;            // [8][n + 1]: at a known index a: 1 if the gap that starts at a is all ones
  uint32_t *words;          // [8][nwords] plane bits, LSB first
  uint32_t *rankw;          // [8][nwords] rank1 at the first position of each word
  uint32_t n, chunks, nwords;
  uint32_t *err;
};

__global__ __launch_bounds__(FG_T) void fill_chunkmax_kernel(FillArgs a) {
  const uint32_t p = blockIdx.y, c = blockIdx.x;
  const uint32_t *R = a.R + (size_t)p * ((size_t)a.n + 1);
  uint32_t best = 0;
  const uint64_t base = (uint64_t)c * FG_CHUNK;
  for (uint32_t i = threadIdx.x; i < FG_CHUNK; i += FG_T) {
    const uint64_t q = base + i;
    if (q <= a.n && R[q] != kUnknown) best = (uint32_t)q + 1u;
  }
  uint32_t tot;
  (void)block_incl_scan_max<FG_T>(best, &tot);
  if (threadIdx.x == 0) a.cmax[(size_t)p * a.chunks + c] = tot;
}

// exclusive prefix max over the chunks of one plane (block = plane)
__global__ __launch_bounds__(1024) void fill_chunkscan_kernel(FillArgs a) {
  uint32_t *cm = a.cmax + (size_t)blockIdx.x * a.chunks;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < a.chunks; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < a.chunks ? cm[i] : 0u;
    uint32_t tot;
    const uint32_t inc = block_incl_scan_max<1024>(v, &tot);
    __shared__ uint32_t sh[1024];
    sh[threadIdx.x] = inc;
    __syncthreads();
    uint32_t ex = threadIdx.x ? sh[threadIdx.x - 1] : 0u;
    ex = ex > carry ? ex : carry;
    __syncthreads();
    if (i < a.chunks) cm[i] = ex;
    carry = carry > tot ? carry : tot;
  }
}

// PASS 0: gap types at the known indices.  PASS 1: plane words + word ranks.
template <int PASS>
__global__ __launch_bounds__(FG_T) void fill_kernel(FillArgs a) {
  __shared__ uint32_t sh[FG_T];
  const uint32_t p = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const uint32_t *R = a.R + (size_t)p * ((size_t)a.n + 1);
  uint8_t *type = a.type + (size_t)p * ((size_t)a.n + 1);
  const uint64_t q0 = (uint64_t)c * FG_CHUNK + (uint64_t)tid * FG_PER;
  // last known index + 1 among my positions, then the same for everything before me
  uint32_t r[FG_PER];
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t i = 0; i < FG_PER; ++i) {
    const uint64_t q = q0 + i;
    r[i] = q <= a.n ? R[q] : kUnknown;
    if (r[i] != kUnknown) mine = (uint32_t)q + 1u;
  }
  uint32_t tot;
  const uint32_t inc = block_incl_scan_max<FG_T>(mine, &tot);
  sh[tid] = inc;
  __syncthreads();
  uint32_t last = tid ? sh[tid - 1] : 0u;                     // known index + 1 before my range, inside the chunk
  const uint32_t carry = a.cmax[(size_t)p * a.chunks + c];
  last = last > carry ? last : carry;                         // ... or in an earlier chunk (index 0 is always known)
  if (PASS == 0) {
    uint32_t a_idx = last ? last - 1u : 0u;
    uint32_t ra = last ? R[a_idx] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < FG_PER; ++i) {
      const uint64_t q = q0 + i;
      if (q == 0 || q > a.n || r[i] == kUnknown) { if (q == 0 && r[i] != kUnknown) { a_idx = 0; ra = r[i]; } continue; }
      const uint32_t ones = r[i] - ra, wdt = (uint32_t)q - a_idx;
      if (r[i] < ra || (ones != 0 && ones != wdt)) *a.err = 1;   // a mixed gap that was never split
      type[a_idx] = ones == wdt ? 1 : 0;
      a_idx = (uint32_t)q; ra = r[i];
    }
  } else {
    uint32_t a_idx = last ? last - 1u : 0u;
    uint32_t ra = R[a_idx];
    uint32_t ty = type[a_idx];
    uint32_t word = 0;
    const uint32_t rank_first = ra + ty * ((uint32_t)q0 - a_idx);   // valid when q0 <= n (checked below)
    uint32_t rank0 = rank_first;
#pragma unroll
    for (uint32_t i = 0; i < FG_PER; ++i) {
      const uint64_t q = q0 + i;
      if (q >= a.n) break;
      if (r[i] != kUnknown) { a_idx = (uint32_t)q; ra = r[i]; ty = type[a_idx]; if (i == 0) rank0 = ra; }
      word |= ty << i;
    }
    const uint64_t w = q0 / 32;
    if (w < a.nwords) {
      a.words[(size_t)p * a.nwords + w] = word;
      a.rankw[(size_t)p * a.nwords + w] = q0 <= a.n ? rank0 : 0u;
    }
  }
}

__global__ void gran_from_words_kernel(FillArgs a, Granule *gran, uint32_t ngran) {
  const uint32_t p = blockIdx.y;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngran; g += gridDim.x * blockDim.x) {
    const uint32_t *W = a.words + (size_t)p * a.nwords, *RW = a.rankw + (size_t)p * a.nwords;
    const uint64_t w = (uint64_t)g * 3;
    Granule G;
    G.w0 = w < a.nwords ? W[w] : 0u;
    G.w1 = w + 1 < a.nwords ? W[w + 1] : 0u;
    G.w2 = w + 2 < a.nwords ? W[w + 2] : 0u;
    G.cum = w < a.nwords ? RW[w] : 0u;
    gran[(size_t)p * ngran + g] = G;
  }
}

// unbwt::bytewise (bce.cpp:1043-1085) as wavelet-matrix access: byte i = the bits met while following position
// i through the eight stable partitions (the reference's cursor heap D does the same walk for all i in order).
__global__ void access_kernel(const Granule *__restrict__ gran, uint32_t ngran, uint32_t n, const uint32_t *zeros8,
                              uint8_t *__restrict__ bwt) {
  uint32_t zeros[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) zeros[j] = zeros8[j];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t pos = i, chr = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t g = div96(pos), o = pos - g * 96u;
      const Granule G = gran[(size_t)j * ngran + g];
      const uint32_t r1 = granule_rank1(G, o);
      const uint32_t wsel = o >> 5, word = wsel == 0 ? G.w0 : (wsel == 1 ? G.w1 : G.w2);
      const uint32_t b = (word >> (o & 31u)) & 1u;
      chr |= b << j;
      pos = b ? zeros[j] + r1 : pos - r1;
    }
    bwt[i] = (uint8_t)chr;
  }
}

// ---- inverse BWT: LF by one stable radix pass on the byte, then concurrent walkers between marked rows ----
__global__ void lf_keys_kernel(const uint8_t *__restrict__ bwt, uint32_t n, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { keys[i] = bwt[i]; vals[i] = i; }
}
__global__ void lf_scatter_kernel(const uint32_t *__restrict__ sorted_rows, uint32_t n, uint32_t *__restrict__ lf) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) lf[sorted_rows[k]] = k;
}
// walker j starts at row j << sh and stops in front of the next row that is a multiple of 2^sh
__global__ void walk_len_kernel(const uint32_t *__restrict__ lf, uint32_t m, uint32_t sh, uint32_t *__restrict__ len,
                                uint32_t *__restrict__ endrow) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint32_t mask = (1u << sh) - 1u;
  uint32_t row = j << sh, l = 0;
  do { row = lf[row]; ++l; } while (row & mask);
  len[j] = l; endrow[j] = row;
}
// text[i] = bwt[row_i] along the walk; text position i lands at out[(i + off) % n]  (std::rotate, bce.cpp:1093)
__global__ void walk_write_kernel(const uint32_t *__restrict__ lf, const uint8_t *__restrict__ bwt, uint32_t m, uint32_t sh,
                                  const uint32_t *__restrict__ len, const uint32_t *__restrict__ dest_end, uint32_t n,
                                  uint32_t off, uint8_t *__restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  uint32_t row = j << sh;
  const uint32_t l = len[j];
  uint64_t i = dest_end[j];                                   // one past my last text position
  for (uint32_t t = 0; t < l; ++t) {
    --i;
    uint64_t o = i + off;
    if (o >= n) o -= n;
    out[o] = bwt[row];
    row = lf[row];
  }
}

// periodic inputs: the walk from row 0 goes round ONE cycle of the LF mapping (length lc) again and again; V holds that
// cycle as the last lc text positions would, and text[i] = V[lc - 1 - ((n - 1 - i) mod lc)]
__global__ void expand_cycle_kernel(const uint8_t *__restrict__ V, uint32_t lc, uint32_t n, uint32_t off, uint8_t *__restrict__ out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint64_t o = (uint64_t)i + off;
    if (o >= n) o -= n;
    out[o] = V[lc - 1u - ((n - 1u - i) % lc)];
  }
}

// ---- the libdivsufsort seam: inverse_bw_transform(T, U, A, n, idx) (include/divsufsort_hip.h; bce.cpp:1091) ----
// T = the BWT divbwt produces (n bytes, the suffix-0 row left out at 1-based position idx).  With the row put back as a
// sentinel the n + 1 rows are the BWT of the rotations of T$: LF by one stable radix pass on 9-bit symbols (0 = $), then
// the decoder's walk from row 0 -- the rotation that starts with $, preceded by the last text byte -- backwards through
// the text.  One cycle of n + 1 rows always (the sentinel is unique).
__global__ void seam_rows_kernel(const uint8_t *__restrict__ U, uint32_t n, uint32_t idx, uint8_t *__restrict__ rows,
                                 uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
    const uint32_t b = i == idx ? 0u : (uint32_t)U[i < idx ? i : i - 1u];
    rows[i] = (uint8_t)b;
    keys[i] = i == idx ? 0u : b + 1u;
    vals[i] = i;
  }
}

uint32_t grid256(uint64_t items) { return (uint32_t)((items + 255) / 256 < 8192 ? (items + 255) / 256 : 8192); }

// The inverse BWT's walk from row 0 through LF (`rows` rows; bwt[r]: the byte in front of row r) back to row 0, by walkers
// that start at every 2^sh-th row (walk_len_kernel), their segments chained here and then written in place
// (walk_write_kernel).  A cycle through all the rows lands at out[(i + off) % len]; a shorter one whose length divides `rows`
// (a periodic input) at cycle[i], if `cycle` is given; any other is not written.  *lc: the cycle's length, 0 if the walk came
// to a segment twice (LF is not a permutation); *walkers: how many walked.
int lf_walk(bce_hip_ctx *c, const uint32_t *lf, const uint8_t *bwt, uint32_t rows, uint8_t *out, uint32_t len, uint32_t off,
            uint8_t *cycle, uint64_t *lc, uint32_t *walkers) {
  uint32_t sh = 0;
  while (((uint64_t)rows >> sh) > (1u << 19)) ++sh;             // at most 2^19 walkers
  // ... and at least 256 rows per walker while that leaves a few thousand of them: the host chains the segments one after
  // the other (a random access each), which for one-row segments of a 1 MB input was 10 ms of a 36 ms decode
  while (sh < 8 && ((uint64_t)rows >> (sh + 1)) >= 4096) ++sh;
  const uint32_t m = (uint32_t)((((uint64_t)rows - 1) >> sh) + 1);
  *walkers = m;
  *lc = 0;
  BCE_TRY(ensure(c, c->key[0], (size_t)3 * m * 4 + 16));         // (the callers' sort is done with its key buffers)
  uint32_t *d_len = c->key[0].as<uint32_t>(), *d_end = d_len + m, *d_dest = d_len + 2 * (size_t)m;
  hipLaunchKernelGGL(walk_len_kernel, dim3((m + 63) / 64), dim3(64), 0, c->stream, lf, m, sh, d_len, d_end);
  std::vector<uint32_t> h_len(m), h_end(m), h_dest(m, 0);
  BCE_HIP_TRY(c, hipMemcpyAsync(h_len.data(), d_len, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  BCE_HIP_TRY(c, hipMemcpyAsync(h_end.data(), d_end, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  uint64_t l = 0;
  uint32_t cur = 0;
  std::vector<uint8_t> visited(m, 0);
  std::vector<uint32_t> order;
  do {
    const uint32_t j = cur >> sh;
    if (visited[j]) return BCE_HIP_OK;
    visited[j] = 1;
    order.push_back(j);
    l += h_len[j];
    cur = h_end[j];
  } while (cur != 0);
  *lc = l;
  uint64_t pos = l;
  for (uint32_t j : order) { h_dest[j] = (uint32_t)pos; pos -= h_len[j]; }
  for (uint32_t j = 0; j < m; ++j) if (!visited[j]) h_len[j] = 0;      // rows off the cycle are never written
  const bool whole = l == rows;
  if (!whole && !(cycle && rows % l == 0)) return BCE_HIP_OK;
  BCE_HIP_TRY(c, hipMemcpyAsync(d_dest, h_dest.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  BCE_HIP_TRY(c, hipMemcpyAsync(d_len, h_len.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  if (whole) hipLaunchKernelGGL(walk_write_kernel, dim3((m + 63) / 64), dim3(64), 0, c->stream, lf, bwt, m, sh, d_len, d_dest, len, off, out);
  else hipLaunchKernelGGL(walk_write_kernel, dim3((m + 63) / 64), dim3(64), 0, c->stream, lf, bwt, m, sh, d_len, d_dest, (uint32_t)l, 0u, cycle);
  return BCE_HIP_OK;
}

}  // namespace

// ---- R -> planes -> granules -> BWT bytes (Decode::planes; alone: kd_planes_from_ranks) ----
// R: the boundary ranks [8][n + 1] in device memory, zeros[p] = n - R[p][n].  The bytes land in c->bwt; the plane words and word
// ranks stay in c->key[0] / c->key[1] (*words, *rankw: [8][plane_words(n)]) until the inverse BWT sorts there.  own_text: the
// context's text buffer is made ready beside the BWT's.  peak_used: sampled after each allocation stage (dec_sample_mem).
int planes_stage(bce_hip_ctx *c, const uint32_t *R, uint32_t n, const uint32_t zeros[8], bool own_text, size_t *peak_used,
                 const uint32_t **words, const uint32_t **rankw) {
  const size_t rstride = (size_t)n + 1;
  FillArgs f;
  f.R = R; f.n = n;
  f.chunks = (uint32_t)(((uint64_t)n + 1 + FG_CHUNK - 1) / FG_CHUNK);
  f.nwords = plane_words(n);
  const uint32_t ngran = plane_granules(n);
  BCE_TRY(ensure(c, c->blk, (size_t)8 * f.chunks * 4 + 64));
  f.cmax = c->blk.as<uint32_t>();
  f.err = f.cmax + (size_t)8 * f.chunks;
  BCE_TRY(ensure(c, c->sa[0], 8 * rstride));                   // gap types
  f.type = c->sa[0].as<uint8_t>();
  BCE_TRY(ensure(c, c->key[0], (size_t)8 * f.nwords * 4));
  BCE_TRY(ensure(c, c->key[1], (size_t)8 * f.nwords * 4));
  f.words = c->key[0].as<uint32_t>();
  f.rankw = c->key[1].as<uint32_t>();
  if (words) *words = f.words;
  if (rankw) *rankw = f.rankw;
  BCE_TRY(ensure(c, c->gran, (size_t)8 * ngran * sizeof(Granule)));
  dec_sample_mem(peak_used);
  BCE_HIP_TRY(c, hipMemsetAsync(f.err, 0, 4, c->stream));
  BCE_HIP_TRY(c, hipMemsetAsync(f.words, 0, (size_t)8 * f.nwords * 4, c->stream));
  BCE_HIP_TRY(c, hipMemsetAsync(f.rankw, 0, (size_t)8 * f.nwords * 4, c->stream));
  hipLaunchKernelGGL(fill_chunkmax_kernel, dim3(f.chunks, 8), dim3(FG_T), 0, c->stream, f);
  hipLaunchKernelGGL(fill_chunkscan_kernel, dim3(8), dim3(1024), 0, c->stream, f);
  hipLaunchKernelGGL((fill_kernel<0>), dim3(f.chunks, 8), dim3(FG_T), 0, c->stream, f);
  hipLaunchKernelGGL((fill_kernel<1>), dim3(f.chunks, 8), dim3(FG_T), 0, c->stream, f);
  const uint32_t gb = (ngran + 255) / 256;
  hipLaunchKernelGGL(gran_from_words_kernel, dim3(gb < 4096 ? gb : 4096, 8), dim3(256), 0, c->stream, f, c->gran.as<Granule>(), ngran);
  uint32_t ferr = 0;
  BCE_TRY(read_back(c, &ferr, f.err, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  if (ferr) { snprintf(c->err, sizeof c->err, "decode: a mixed gap was never split"); return BCE_HIP_E_INTERNAL; }
  BCE_TRY(ensure(c, c->bwt, n));
  if (own_text) BCE_TRY(ensure(c, c->text, n));
  BCE_TRY(ensure(c, c->stat, 64));
  dec_sample_mem(peak_used);
  uint32_t *dz = c->stat.as<uint32_t>();
  BCE_HIP_TRY(c, hipMemcpyAsync(dz, zeros, 32, hipMemcpyHostToDevice, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  hipLaunchKernelGGL(access_kernel, dim3(grid256(n)), dim3(256), 0, c->stream, c->gran.as<Granule>(), ngran, n, dz, c->bwt.as<uint8_t>());
  return BCE_HIP_OK;
}

// ---- inverse BWT (Decode::inverse_bwt; alone: kd_unbwt) ----
// The n bytes of c->bwt -> the text, position i at text[(i + off) % n] (off < n; device memory, any alignment).  One cycle through
// all n rows for a primitive input; a shorter cycle (length lc, the input's period pattern in BWT terms) otherwise, written once
// into V (the sort's value buffers are free again) and then unrolled.  *lc, *walkers: as lf_walk reports them, set on the
// error return as well (no cycle through row 0 of a length that divides n: nothing is written to `text`).
int unbwt_stage(bce_hip_ctx *c, uint32_t n, uint32_t off, uint8_t *text, size_t *peak_used, uint64_t *lc, uint32_t *walkers) {
  const size_t b4 = (size_t)n * 4;
  const uint32_t gn = grid256(n);
  for (int i = 0; i < 2; ++i) { BCE_TRY(ensure(c, c->sa[i], b4)); BCE_TRY(ensure(c, c->key[i], b4)); }
  BCE_TRY(ensure(c, c->rank, b4));
  dec_sample_mem(peak_used);
  uint32_t *key[2] = {c->key[0].as<uint32_t>(), c->key[1].as<uint32_t>()};
  uint32_t *val[2] = {c->sa[0].as<uint32_t>(), c->sa[1].as<uint32_t>()};
  uint32_t *lf = c->rank.as<uint32_t>();
  hipLaunchKernelGGL(lf_keys_kernel, dim3(gn), dim3(256), 0, c->stream, c->bwt.as<uint8_t>(), n, key[0], val[0]);
  int res = 0;
  BCE_TRY(radix_sort_pairs(c, key, val, n, 0, 8, &res, 8));
  dec_sample_mem(peak_used);                                    // (the sort's histograms)
  hipLaunchKernelGGL(lf_scatter_kernel, dim3(gn), dim3(256), 0, c->stream, val[res], n, lf);
  uint8_t *V = reinterpret_cast<uint8_t *>(val[0]);
  *lc = 0; *walkers = 0;
  BCE_TRY(lf_walk(c, lf, c->bwt.as<uint8_t>(), n, text, n, off, V, lc, walkers));
  if (*lc == 0 || *lc > n || n % *lc) { snprintf(c->err, sizeof c->err, "decode: LF cycle of length %llu in %u rows", (unsigned long long)*lc, n); return BCE_HIP_E_INTERNAL; }
  // periodic input (the reference's decoder returns zeros here)
  if (*lc != n) hipLaunchKernelGGL(expand_cycle_kernel, dim3(gn), dim3(256), 0, c->stream, V, (uint32_t)*lc, n, off, text);
  return BCE_HIP_OK;
}

int kd_inverse_bw_transform(bce_hip_ctx *c, const uint8_t *T_host, uint8_t *U_host, uint32_t n, uint32_t idx) {
  if (n == 0 || n >= 0x7FFFFFFFu || idx == 0 || idx > n) return BCE_HIP_E_ARG;
  const uint32_t m_rows = n + 1u;
  const size_t b4 = (size_t)m_rows * 4;
  // the context's compression state is gone -- before the first allocation, which may give back its planes and node lists (ctx_trim,
  // phase 5: the caller's)
  dec_drop_state(c);
  BCE_TRY(ensure(c, c->text, m_rows));
  BCE_TRY(ensure(c, c->bwt, m_rows));
  BCE_TRY(ensure(c, c->ptmp[0], m_rows));
  for (int i = 0; i < 2; ++i) { BCE_TRY(ensure(c, c->sa[i], b4)); BCE_TRY(ensure(c, c->key[i], b4)); }
  BCE_TRY(ensure(c, c->rank, b4));
  uint8_t *d_in = c->ptmp[0].as<uint8_t>(), *rows = c->bwt.as<uint8_t>();
  BCE_HIP_TRY(c, hipMemcpyAsync(d_in, T_host, n, hipMemcpyHostToDevice, c->stream));
  uint32_t *key[2] = {c->key[0].as<uint32_t>(), c->key[1].as<uint32_t>()};
  uint32_t *val[2] = {c->sa[0].as<uint32_t>(), c->sa[1].as<uint32_t>()};
  uint32_t *lf = c->rank.as<uint32_t>();
  const uint32_t gn = grid256(m_rows);
  hipLaunchKernelGGL(seam_rows_kernel, dim3(gn), dim3(256), 0, c->stream, d_in, n, idx, rows, key[0], val[0]);
  int res = 0;
  BCE_TRY(radix_sort_pairs(c, key, val, m_rows, 0, 9, &res, 9));
  hipLaunchKernelGGL(lf_scatter_kernel, dim3(gn), dim3(256), 0, c->stream, val[res], m_rows, lf);
  // the walk's positions are those of $T: shifted by n (= -1 mod n + 1) the text lands at [0, n), the sentinel's slot at n.
  // (key[0] holds 4(n + 1) bytes already, which the walk's 3m + 4 words grow if they need more.)
  uint64_t lc = 0;
  uint32_t walkers = 0;
  BCE_TRY(lf_walk(c, lf, rows, m_rows, c->text.as<uint8_t>(), m_rows, n, nullptr, &lc, &walkers));
  if (lc != m_rows) return BCE_HIP_E_ARG;                        // not one LF cycle: T / idx inconsistent
  BCE_HIP_TRY(c, hipMemcpyAsync(U_host, c->text.p, n, hipMemcpyDeviceToHost, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// ---- test hooks: the back end alone (bce_hip_planes_from_ranks_device, bce_hip_unbwt_device) ----
// The stages above on arrays of the caller's, in a context whose compression state is dropped as a decode drops it; the context's
// buffers are the decoder's own, so a later encode or decode finds them as after a decode.
int kd_planes_from_ranks(bce_hip_ctx *c, const uint32_t *d_R, uint32_t n, uint8_t *d_bwt, uint32_t *d_words, uint32_t *d_rankw) {
  const size_t rstride = (size_t)n + 1;
  uint32_t zeros[8];
  for (int p = 0; p < 8; ++p) {                                  // the two ends of every plane are known: R[p][0] = 0, R[p][n] = its ones
    uint32_t r0 = 0, rn = 0;
    BCE_TRY(read_back(c, &r0, d_R + (size_t)p * rstride, 4));
    BCE_TRY(read_back(c, &rn, d_R + (size_t)p * rstride + n, 4));
    if (r0 != 0 || rn > n) { snprintf(c->err, sizeof c->err, "planes from ranks: R[%d][0] = %u, R[%d][n] = %u with n = %u", p, r0, p, rn, n); return BCE_HIP_E_ARG; }
    zeros[p] = n - rn;
  }
  dec_drop_state(c);
  PartEnd part_end{c};
  c->dec_part = 2;
  const uint32_t *words = nullptr, *rankw = nullptr;
  BCE_TRY(planes_stage(c, d_R, n, zeros, false, nullptr, &words, &rankw));
  const size_t wb = (size_t)8 * plane_words(n) * 4;
  if (d_words) BCE_HIP_TRY(c, hipMemcpyAsync(d_words, words, wb, hipMemcpyDeviceToDevice, c->stream));
  if (d_rankw) BCE_HIP_TRY(c, hipMemcpyAsync(d_rankw, rankw, wb, hipMemcpyDeviceToDevice, c->stream));
  BCE_HIP_TRY(c, hipMemcpyAsync(d_bwt, c->bwt.p, n, hipMemcpyDeviceToDevice, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

int kd_unbwt(bce_hip_ctx *c, const uint8_t *d_bwt, uint32_t n, uint32_t offset, uint8_t *d_out, uint64_t *cycle, uint32_t *walkers) {
  dec_drop_state(c);
  PartEnd part_end{c};
  c->dec_part = 3;
  BCE_TRY(ensure(c, c->bwt, n));
  BCE_HIP_TRY(c, hipMemcpyAsync(c->bwt.p, d_bwt, n, hipMemcpyDeviceToDevice, c->stream));
  uint64_t lc = 0;
  uint32_t m = 0;
  const int rc = unbwt_stage(c, n, offset % n, d_out, nullptr, &lc, &m);
  if (cycle) *cycle = lc;
  if (walkers) *walkers = m;
  if (rc != BCE_HIP_OK) { (void)hipStreamSynchronize(c->stream); return rc; }   // (nothing of the caller's is in flight on return)
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
