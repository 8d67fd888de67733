// kd_parse.hip -- a second buffer written as copies out of the indexed text plus the bytes that are new, and rebuilt from the text
// and that list (bce_hip_parse / _parse_device / _parse_of_lengths_device, bce_hip_patch / _patch_device, `bce -gr`, `bce -ga`).
//
// The parse.  len[i], pos[i]: the linear matching statistics of the query (kd_match.hip).  From e = q - 1 down: a copy of len[e]
// bytes where len[e] >= min_len, else the literal byte Q[e] (parse_step.h).  The chain is a dependent walk; it is cut into blocks
// of PAR_BLOCK = 2048 positions:
//   exit    one workgroup per block.  Every position's first hop goes into LDS; pointer doubling (11 rounds, two arrays in turn,
//           one barrier a round) finds for EVERY position the first chain node below the block's base, as node + 1 (0: the chain
//           is over).  A hop that has left the block is final and is carried.
//   walk    one lane: e = q - 1; entry[block(e)] = e; e = exit[e] - 1 ... : at most one dependent load per block, the only
//           sequential part.  Blocks the chain jumps over keep PARSE_NO_ENTRY.
//   mark    one workgroup per block: one lane walks the block's hops in LDS from the entry to the base (at most 2048 steps, the
//           blocks side by side) and sets a flag byte per node; the block's 2048 flag bytes leave as one row, zeros where no node is.
//   count   per block: the op heads and the literal nodes, packed into one u64 (heads in the high word: both stay below 2^31), and
//           the copy ends.  top: one workgroup scans the blocks' sums, 256 at a time (scan_util.h's carried pass).  emit: the
//           blocks again, every head writes its op at its scanned place and every literal node its byte.  A literal run may span
//           any number of blocks, so its length is not walked: every head leaves the literal count up to itself, and `runs` takes
//           the difference of two neighbouring heads.
// The patch.  check: per op the rules of parse_step.h, per block the sums of the lengths and of the literal lengths.  top: their
// scan, the flag bits together.  The host reads three words and refuses before anything is copied.  fill: every op's offset in
// the output and in the literal bytes.  copy: one lane per 16 bytes of OUTPUT (aligned as the output's address is), a workgroup
// per 16 KB: it finds the first and last op of its tile by binary search, each lane its own op between them; sixteen bytes that
// lie in one op move as one load of any alignment and one aligned store, the rest byte by byte.
// No atomics: every sum is taken in a fixed order.  Everything written is the feature's own (qb::par_* of c->qbuf) or the caller's outputs;
// the text, the lengths and the positions are only read.
#include "common.h"
#include "parse_step.h"
#include "scan_util.h"

namespace bce {

namespace {

constexpr int PAR_T = 256;                   // lanes per workgroup (4 waves)
constexpr int PAR_ITEMS = 8;                 // positions / ops per lane
constexpr uint32_t PAR_BLOCK = PAR_T * PAR_ITEMS;   // 2048
constexpr int PAR_ROUNDS = 11;               // 2^11 hops reach across a block
constexpr uint32_t PAT_CHUNK = 16;           // patch_copy: output bytes per lane and step
constexpr uint32_t PAT_STEPS = 4;
constexpr uint32_t PAT_TILE = PAR_T * PAT_CHUNK * PAT_STEPS;   // 16384 output bytes per workgroup
static_assert((1u << PAR_ROUNDS) == PAR_BLOCK, "the doubling rounds span one block");

__global__ __launch_bounds__(PAR_T) void parse_exit_kernel(const uint32_t *__restrict__ len, uint32_t q, uint32_t min_len,
                                                           uint32_t *__restrict__ exit1) {
  __shared__ uint32_t nxt[2][PAR_BLOCK];
  const uint32_t base = blockIdx.x * PAR_BLOCK;
#pragma unroll
  for (int k = 0; k < PAR_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * PAR_T + threadIdx.x, e = base + i;
    nxt[0][i] = e < q ? parse_next1(e, parse_jump(len[e], min_len)) : 0u;   // (past the end: final at once, never asked for)
  }
  __syncthreads();
  int cur = 0;
  for (int r = 0; r < PAR_ROUNDS; ++r) {                              // read one array, write the other, meet
#pragma unroll
    for (int k = 0; k < PAR_ITEMS; ++k) {
      const uint32_t i = (uint32_t)k * PAR_T + threadIdx.x;
      uint32_t v = nxt[cur][i];
      if (!parse_left_block(v, base)) v = nxt[cur][v - 1u - base];    // (v - 1 < base + i: a hop goes to the left)
      nxt[cur ^ 1][i] = v;
    }
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int k = 0; k < PAR_ITEMS; ++k) {
    const uint32_t i = (uint32_t)k * PAR_T + threadIdx.x, e = base + i;
    if (e < q) exit1[e] = nxt[cur][i];
  }
}

// one lane; entry[0, nb) prefilled with PARSE_NO_ENTRY
__global__ void parse_walk_kernel(const uint32_t *__restrict__ exit1, uint32_t q, uint32_t *__restrict__ entry) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t e = q - 1u;
  for (;;) {
    entry[e / PAR_BLOCK] = e;
    const uint32_t v = exit1[e];                                      // <= the base of e's block: every step leaves a block
    if (v == 0u) break;
    e = v - 1u;
  }
}

// flag: nb * PAR_BLOCK bytes, every block writes its whole row
__global__ __launch_bounds__(PAR_T) void parse_mark_kernel(const uint32_t *__restrict__ len, uint32_t q, uint32_t min_len,
                                                           const uint32_t *__restrict__ entry, uint8_t *__restrict__ flag) {
  __shared__ uint32_t hop[PAR_BLOCK];
  __shared__ uint2 row[PAR_T];                                        // the block's 2048 flag bytes
  const uint32_t base = blockIdx.x * PAR_BLOCK, ent = entry[blockIdx.x];
  row[threadIdx.x] = make_uint2(0u, 0u);
  if (ent != PARSE_NO_ENTRY) {
#pragma unroll
    for (int k = 0; k < PAR_ITEMS; ++k) {
      const uint32_t i = (uint32_t)k * PAR_T + threadIdx.x, e = base + i;
      hop[i] = e < q ? len[e] : 0u;
    }
  }
  __syncthreads();
  if (ent != PARSE_NO_ENTRY && threadIdx.x == 0) {
    uint8_t *f = reinterpret_cast<uint8_t *>(row);
    uint32_t i = ent - base;                                          // < PAR_BLOCK: the walk stored ent under its own block
    for (;;) {
      const uint32_t l = hop[i];
      f[i] = parse_kind(l, min_len);
      const uint32_t j = parse_jump(l, min_len);
      if (j > i) break;
      i -= j;
    }
  }
  __syncthreads();
  reinterpret_cast<uint2 *>(flag + base)[threadIdx.x] = row[threadIdx.x];
}

// the eight flags of a lane's positions base + 8 t .. + 7 in f[0 .. 7], the flag of the position behind them in f[8] (0 past the rows)
__device__ __forceinline__ void load_flags(const uint8_t *flag, uint32_t base, uint64_t rows_bytes, uint8_t f[PAR_ITEMS + 1]) {
  const uint64_t at = (uint64_t)base + threadIdx.x * PAR_ITEMS;
  const uint2 w = *reinterpret_cast<const uint2 *>(flag + at);
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[k] = (uint8_t)(w.x >> (8 * k)); f[4 + k] = (uint8_t)(w.y >> (8 * k)); }
  f[PAR_ITEMS] = at + PAR_ITEMS < rows_bytes ? flag[at + PAR_ITEMS] : PARSE_NONE;
}

// heads << 32 | literal nodes of a lane's eight positions; *copies = its copy ends
__device__ __forceinline__ uint64_t count_flags(const uint8_t f[PAR_ITEMS + 1], uint32_t *copies) {
  uint32_t heads = 0, lits = 0, cop = 0;
#pragma unroll
  for (int k = 0; k < PAR_ITEMS; ++k) {
    heads += parse_is_head(f[k], f[k + 1]);
    lits += f[k] == PARSE_LIT;
    cop += f[k] == PARSE_COPY;
  }
  *copies = cop;
  return (uint64_t)heads << 32 | lits;
}

__global__ __launch_bounds__(PAR_T) void parse_count_kernel(const uint8_t *__restrict__ flag, uint64_t rows_bytes, uint64_t *__restrict__ bsum,
                                                            uint32_t *__restrict__ bcop) {
  uint8_t f[PAR_ITEMS + 1];
  load_flags(flag, blockIdx.x * PAR_BLOCK, rows_bytes, f);
  uint32_t cop;
  const uint64_t s = count_flags(f, &cop);
  const uint64_t tot = block_reduce_sum64<PAR_T>(s);
  cop = block_reduce_sum<PAR_T>(cop);
  if (threadIdx.x == 0) { bsum[blockIdx.x] = tot; bcop[blockIdx.x] = cop; }
}

// one workgroup: bsum[0, nb) -> its exclusive scan, in place; res[0] = heads << 32 | literal nodes of the query, res[1] = its copies
__global__ __launch_bounds__(PAR_T) void parse_top_kernel(uint64_t *__restrict__ bsum, const uint32_t *__restrict__ bcop, uint32_t nb,
                                                          uint64_t *__restrict__ res) {
  const uint64_t sum = block_carried_scan_sum64<PAR_T>(bsum, nb);
  uint64_t cop = 0;
  for (uint32_t i = threadIdx.x; i < nb; i += PAR_T) cop += bcop[i];
  cop = block_reduce_sum64<PAR_T>(cop);
  if (threadIdx.x == 0) { res[0] = sum; res[1] = cop; }
}

// ops: nops pairs of words (len, src); a literal head leaves its length to parse_runs_kernel and its literal count in hpre
__global__ __launch_bounds__(PAR_T) void parse_emit_kernel(const uint8_t *__restrict__ flag, uint64_t rows_bytes, const uint64_t *__restrict__ bsum,
                                                           const uint32_t *__restrict__ len, const uint32_t *__restrict__ pos,
                                                           const uint8_t *__restrict__ query, uint32_t *__restrict__ ops,
                                                           uint8_t *__restrict__ lits, uint32_t *__restrict__ hpre) {
  const uint32_t base = blockIdx.x * PAR_BLOCK;
  uint8_t f[PAR_ITEMS + 1];
  load_flags(flag, base, rows_bytes, f);
  uint32_t cop;
  const uint64_t s = count_flags(f, &cop);
  uint64_t tot;
  const uint64_t ex = bsum[blockIdx.x] + block_excl_scan_sum64<PAR_T>(s, &tot);
  uint32_t k = (uint32_t)(ex >> 32), l = (uint32_t)ex;               // ops and literal bytes in front of this lane's positions
#pragma unroll
  for (int j = 0; j < PAR_ITEMS; ++j) {
    const uint32_t e = base + threadIdx.x * PAR_ITEMS + (uint32_t)j;  // (a flag other than 0 stands only at e < q)
    if (f[j] == PARSE_LIT) lits[l++] = query[e];
    if (parse_is_head(f[j], f[j + 1])) {
      if (f[j] == PARSE_COPY) { ops[2 * (size_t)k] = len[e]; ops[2 * (size_t)k + 1] = pos ? pos[e] : 0u; }
      else ops[2 * (size_t)k + 1] = PARSE_LITERAL;
      hpre[k++] = l;
    }
  }
}

__global__ __launch_bounds__(PAR_T) void parse_runs_kernel(uint32_t *__restrict__ ops, const uint32_t *__restrict__ hpre, uint32_t nops) {
  const uint32_t k = blockIdx.x * PAR_T + threadIdx.x;
  if (k >= nops || ops[2 * (size_t)k + 1] != PARSE_LITERAL) return;
  ops[2 * (size_t)k] = hpre[k] - (k ? hpre[k - 1] : 0u);
}

// ---- the patch ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_ops(const uint32_t *ops, uint32_t nops, uint32_t base, uint32_t olen[PAR_ITEMS], uint32_t osrc[PAR_ITEMS]) {
#pragma unroll
  for (int j = 0; j < PAR_ITEMS; ++j) {
    const uint32_t k = base + threadIdx.x * PAR_ITEMS + (uint32_t)j;
    olen[j] = k < nops ? ops[2 * (size_t)k] : 0u;
    osrc[j] = k < nops ? ops[2 * (size_t)k + 1] : 0u;
  }
}

// per block: blen[b], blit[b] = the sums of its ops' lengths and of its literal runs' lengths; bbad[b] = what is wrong with one of them
__global__ __launch_bounds__(PAR_T) void patch_check_kernel(const uint32_t *__restrict__ ops, uint32_t nops, uint32_t n, uint64_t *__restrict__ blen,
                                                            uint64_t *__restrict__ blit, uint32_t *__restrict__ bbad) {
  const uint32_t base = blockIdx.x * PAR_BLOCK;
  uint32_t olen[PAR_ITEMS], osrc[PAR_ITEMS];
  load_ops(ops, nops, base, olen, osrc);
  uint64_t sl = 0, st = 0;
  uint32_t bad = 0;                                                   // ops of length 0 in the low half, copies out of range in the high half
#pragma unroll
  for (int j = 0; j < PAR_ITEMS; ++j) {
    if (base + threadIdx.x * PAR_ITEMS + (uint32_t)j >= nops) continue;
    const uint32_t b = patch_op_bad(olen[j], osrc[j], n);
    bad += (b & PATCH_BAD_ZERO ? 1u : 0u) + (b & PATCH_BAD_RANGE ? 0x10000u : 0u);
    sl += olen[j];
    st += patch_lit_len(olen[j], osrc[j]);
  }
  const uint64_t tl = block_reduce_sum64<PAR_T>(sl), tt = block_reduce_sum64<PAR_T>(st);
  bad = block_reduce_sum<PAR_T>(bad);                                 // (at most 2048 in either half)
  if (threadIdx.x == 0) {
    blen[blockIdx.x] = tl;
    blit[blockIdx.x] = tt;
    bbad[blockIdx.x] = (bad & 0xFFFFu ? PATCH_BAD_ZERO : 0u) | (bad >> 16 ? PATCH_BAD_RANGE : 0u);
  }
}

// one workgroup: both sums -> their exclusive scans, in place; res[0] = the output's bytes, res[1] = the literal bytes, res[2] = the flag bits
__global__ __launch_bounds__(PAR_T) void patch_top_kernel(uint64_t *__restrict__ blen, uint64_t *__restrict__ blit, const uint32_t *__restrict__ bbad,
                                                          uint32_t nb, uint64_t *__restrict__ res) {
  const uint64_t cl = block_carried_scan_sum64<PAR_T>(blen, nb), ct = block_carried_scan_sum64<PAR_T>(blit, nb);
  uint32_t zero = 0, range = 0;
  for (uint32_t i = threadIdx.x; i < nb; i += PAR_T) {
    const uint32_t b = bbad[i];
    zero |= b & PATCH_BAD_ZERO;
    range |= b & PATCH_BAD_RANGE;
  }
  zero = block_reduce_max<PAR_T>(zero);
  range = block_reduce_max<PAR_T>(range);
  if (threadIdx.x == 0) { res[0] = cl; res[1] = ct; res[2] = zero | range; }
}

// after the list has passed: off[k], loff[k] = where op k begins in the output and in the literal bytes (both below 2^31), off[nops] = the total
__global__ __launch_bounds__(PAR_T) void patch_fill_kernel(const uint32_t *__restrict__ ops, uint32_t nops, const uint64_t *__restrict__ blen,
                                                           const uint64_t *__restrict__ blit, uint32_t *__restrict__ off, uint32_t *__restrict__ loff) {
  const uint32_t base = blockIdx.x * PAR_BLOCK;
  uint32_t olen[PAR_ITEMS], osrc[PAR_ITEMS];
  load_ops(ops, nops, base, olen, osrc);
  uint64_t sl = 0, st = 0;
#pragma unroll
  for (int j = 0; j < PAR_ITEMS; ++j) { sl += olen[j]; st += patch_lit_len(olen[j], osrc[j]); }
  uint64_t tl, tt;
  uint64_t rl = blen[blockIdx.x] + block_excl_scan_sum64<PAR_T>(sl, &tl), rt = blit[blockIdx.x] + block_excl_scan_sum64<PAR_T>(st, &tt);
#pragma unroll
  for (int j = 0; j < PAR_ITEMS; ++j) {
    const uint32_t k = base + threadIdx.x * PAR_ITEMS + (uint32_t)j;
    if (k < nops) { off[k] = (uint32_t)rl; loff[k] = (uint32_t)rt; }
    rl += olen[j];
    rt += patch_lit_len(olen[j], osrc[j]);
    if (k + 1u == nops) off[nops] = (uint32_t)rl;
  }
}

// where op k's bytes come from
__device__ __forceinline__ const uint8_t *patch_src(const uint32_t *ops, const uint32_t *loff, const uint8_t *text, const uint8_t *lits, uint32_t k) {
  const uint32_t src = ops[2 * (size_t)k + 1];
  return src == PARSE_LITERAL ? lits + loff[k] : text + src;
}

// Output byte o stands at out[o]; the lanes' chunks are the 16-byte words of the output's ADDRESS, `lead` = that address mod 16, so
// a whole chunk is stored as one aligned word.  Chunk c holds the output bytes [16 c - lead, 16 c + 16 - lead) cut to [0, total).
__global__ __launch_bounds__(PAR_T) void patch_copy_kernel(const uint32_t *__restrict__ ops, uint32_t nops, const uint32_t *__restrict__ off,
                                                           const uint32_t *__restrict__ loff, const uint8_t *__restrict__ text,
                                                           const uint8_t *__restrict__ lits, uint8_t *__restrict__ out, uint32_t total,
                                                           uint32_t lead) {
  const uint64_t span = (uint64_t)lead + total;                       // the chunks cover [0, span) of the address-aligned line
  const uint64_t t0 = (uint64_t)blockIdx.x * PAT_TILE, t1 = t0 + PAT_TILE < span ? t0 + PAT_TILE : span;
  // the tile's first and last output byte, and their ops: once per workgroup, the same in every lane
  const uint32_t first = (uint32_t)(t0 > lead ? t0 - lead : 0u), last = (uint32_t)(t1 - 1u - lead);
  const uint32_t k0 = patch_op_of(off, nops, first), k1 = patch_op_of(off, nops, last);
#pragma unroll 1
  for (uint32_t s = 0; s < PAT_STEPS; ++s) {
    const uint64_t c0 = t0 + ((uint64_t)s * PAR_T + threadIdx.x) * PAT_CHUNK;
    if (c0 >= t1) break;
    const uint32_t lo = (uint32_t)(c0 > lead ? c0 - lead : 0u);
    const uint32_t hi = (uint32_t)((c0 + PAT_CHUNK < span ? c0 + PAT_CHUNK : span) - lead);
    uint32_t k = k0 + patch_op_of(off + k0, k1 - k0 + 1u, lo);       // (off[k1 + 1] > last >= lo)
    uint32_t begin = off[k], end = off[k + 1];
    const uint8_t *src = patch_src(ops, loff, text, lits, k);
    if (hi - lo == PAT_CHUNK && end >= hi) {                          // sixteen bytes of one op: one load of any alignment, one aligned store
      uint4 v;
      __builtin_memcpy(&v, src + (lo - begin), PAT_CHUNK);
      *reinterpret_cast<uint4 *>(out + lo) = v;
      continue;
    }
    for (uint32_t o = lo; o < hi; ++o) {                              // the ragged ends: across ops, and the output's first and last bytes
      while (end <= o) { ++k; begin = end; end = off[k + 1]; src = patch_src(ops, loff, text, lits, k); }
      out[o] = src[o - begin];
    }
  }
}

int par_totals(bce_hip_ctx *c, const uint64_t *d_res, uint32_t q, bce_hip_parse_info *info) {
  uint64_t res[2];
  BCE_TRY(read_back(c, res, d_res, 16));                              // (the wait)
  BCE_HIP_TRY(c, hipGetLastError());
  info->nops = res[0] >> 32;
  info->nlits = res[0] & 0xFFFFFFFFull;
  info->ncopies = res[1];
  info->copied = q - info->nlits;
  return BCE_HIP_OK;
}

}  // namespace

// The parse of q >= 1 query bytes from their q lengths (d_len[i] <= i + 1; anything larger counts as i + 1) and positions (d_pos may
// be null: src = 0).  *info is exact whenever BCE_HIP_OK or BCE_HIP_E_OVERFLOW comes back.  sizing: nothing more; otherwise the ops
// (pairs of words, 4-byte aligned) and the literal bytes are written when both fit their caps, else BCE_HIP_E_OVERFLOW and neither
// is touched.  All arrays: device memory of the context's device.  Queued on the context's stream; complete on return.
int kd_parse(bce_hip_ctx *c, const uint32_t *d_len, const uint32_t *d_pos, const uint8_t *d_query, uint32_t q, uint32_t min_len, bool sizing,
             uint32_t *d_ops, uint64_t ops_cap, uint8_t *d_lits, uint64_t lits_cap, bce_hip_parse_info *info) {
  const uint32_t nb = (uint32_t)(((uint64_t)q + PAR_BLOCK - 1) / PAR_BLOCK);
  const uint64_t rows_bytes = (uint64_t)nb * PAR_BLOCK;
  BCE_TRY(ensure(c, c->qbuf[qb::par_res], 32));
  BCE_TRY(ensure(c, c->qbuf[qb::par_exit], (size_t)q * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::par_entry], (size_t)nb * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::par_flag], (size_t)rows_bytes));
  BCE_TRY(ensure(c, c->qbuf[qb::par_bsum], (size_t)nb * 8));
  BCE_TRY(ensure(c, c->qbuf[qb::par_bcnt], (size_t)nb * 4));
  uint32_t *exit1 = c->qbuf[qb::par_exit].as<uint32_t>(), *entry = c->qbuf[qb::par_entry].as<uint32_t>(), *bcop = c->qbuf[qb::par_bcnt].as<uint32_t>();
  uint8_t *flag = c->qbuf[qb::par_flag].as<uint8_t>();
  uint64_t *bsum = c->qbuf[qb::par_bsum].as<uint64_t>(), *d_res = c->qbuf[qb::par_res].as<uint64_t>();
  BCE_HIP_TRY(c, hipMemsetAsync(entry, 0xFF, (size_t)nb * 4, c->stream));
  hipLaunchKernelGGL(parse_exit_kernel, dim3(nb), dim3(PAR_T), 0, c->stream, d_len, q, min_len, exit1);
  hipLaunchKernelGGL(parse_walk_kernel, dim3(1), dim3(64), 0, c->stream, exit1, q, entry);
  hipLaunchKernelGGL(parse_mark_kernel, dim3(nb), dim3(PAR_T), 0, c->stream, d_len, q, min_len, entry, flag);
  hipLaunchKernelGGL(parse_count_kernel, dim3(nb), dim3(PAR_T), 0, c->stream, flag, rows_bytes, bsum, bcop);
  hipLaunchKernelGGL(parse_top_kernel, dim3(1), dim3(PAR_T), 0, c->stream, bsum, bcop, nb, d_res);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_TRY(par_totals(c, d_res, q, info));
  if (sizing) return BCE_HIP_OK;
  if (info->nops > ops_cap || info->nlits > lits_cap) {
    snprintf(c->err, sizeof c->err, "parse: %llu ops and %llu literal bytes, room for %llu and %llu", (unsigned long long)info->nops,
             (unsigned long long)info->nlits, (unsigned long long)ops_cap, (unsigned long long)lits_cap);
    return BCE_HIP_E_OVERFLOW;
  }
  const uint32_t nops = (uint32_t)info->nops;                         // >= 1: the last position is a head
  BCE_TRY(ensure(c, c->qbuf[qb::par_hpre], (size_t)nops * 4));
  uint32_t *hpre = c->qbuf[qb::par_hpre].as<uint32_t>();
  hipLaunchKernelGGL(parse_emit_kernel, dim3(nb), dim3(PAR_T), 0, c->stream, flag, rows_bytes, bsum, d_len, d_pos, d_query, d_ops, d_lits, hpre);
  hipLaunchKernelGGL(parse_runs_kernel, dim3((nops + PAR_T - 1) / PAR_T), dim3(PAR_T), 0, c->stream, d_ops, hpre, nops);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

// The bytes that nops >= 1 ops (pairs of words, 4-byte aligned, nops < 2^31) and nlits literal bytes describe over the context's
// text (c->text, c->n), into d_out (any alignment).  A list that is not well formed: BCE_HIP_E_ARG with the reason in c->err, before
// the copy is launched.  *out_len = the result's bytes once the list has passed; more than cap: BCE_HIP_E_OVERFLOW; sizing:
// nothing is copied.  Complete on return.
int kd_patch(bce_hip_ctx *c, const uint32_t *d_ops, uint32_t nops, const uint8_t *d_lits, uint64_t nlits, bool sizing, uint8_t *d_out,
             uint64_t cap, uint64_t *out_len) {
  const uint32_t nb = (nops + PAR_BLOCK - 1) / PAR_BLOCK;
  BCE_TRY(ensure(c, c->qbuf[qb::par_res], 32));
  BCE_TRY(ensure(c, c->qbuf[qb::par_bsum], (size_t)nb * 16));
  BCE_TRY(ensure(c, c->qbuf[qb::par_bcnt], (size_t)nb * 4));
  uint64_t *blen = c->qbuf[qb::par_bsum].as<uint64_t>(), *blit = blen + nb, *d_res = c->qbuf[qb::par_res].as<uint64_t>();
  uint32_t *bbad = c->qbuf[qb::par_bcnt].as<uint32_t>();
  hipLaunchKernelGGL(patch_check_kernel, dim3(nb), dim3(PAR_T), 0, c->stream, d_ops, nops, c->n, blen, blit, bbad);
  hipLaunchKernelGGL(patch_top_kernel, dim3(1), dim3(PAR_T), 0, c->stream, blen, blit, bbad, nb, d_res);
  BCE_HIP_TRY(c, hipGetLastError());
  uint64_t res[3];
  BCE_TRY(read_back(c, res, d_res, 24));
  BCE_HIP_TRY(c, hipGetLastError());
  if (const char *why = patch_list_bad((uint32_t)res[2], res[0], res[1], nlits)) { snprintf(c->err, sizeof c->err, "%s", why); return BCE_HIP_E_ARG; }
  *out_len = res[0];
  if (sizing) return BCE_HIP_OK;
  if (res[0] > cap) {
    snprintf(c->err, sizeof c->err, "patch: %llu bytes, room for %llu", (unsigned long long)res[0], (unsigned long long)cap);
    return BCE_HIP_E_OVERFLOW;
  }
  BCE_TRY(ensure(c, c->qbuf[qb::par_off], ((size_t)nops + 1) * 4));
  BCE_TRY(ensure(c, c->qbuf[qb::par_loff], (size_t)nops * 4));
  uint32_t *off = c->qbuf[qb::par_off].as<uint32_t>(), *loff = c->qbuf[qb::par_loff].as<uint32_t>();
  const uint32_t total = (uint32_t)res[0], lead = (uint32_t)(reinterpret_cast<uintptr_t>(d_out) & (PAT_CHUNK - 1u));
  const uint32_t tiles = (uint32_t)(((uint64_t)lead + total + PAT_TILE - 1) / PAT_TILE);
  hipLaunchKernelGGL(patch_fill_kernel, dim3(nb), dim3(PAR_T), 0, c->stream, d_ops, nops, blen, blit, off, loff);
  hipLaunchKernelGGL(patch_copy_kernel, dim3(tiles), dim3(PAR_T), 0, c->stream, d_ops, nops, off, loff, c->text.as<uint8_t>(), d_lits, d_out, total,
                     lead);
  BCE_HIP_TRY(c, hipGetLastError());
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));
  BCE_HIP_TRY(c, hipGetLastError());
  return BCE_HIP_OK;
}

}  // namespace bce
