// kd_crc32.hip -- CRC-32 (zlib's: reflected 0xEDB88320, init and final xor 0xFFFFFFFF) of a device buffer
// (bce_hip_crc32_device, bce_hip_input_crc32, bce_hip_decode_crc32; the blocks of a version-2 container).
//
// The text is in HBM already -- the decoder leaves it there, the loads put it there --, so its checksum is one more pass that
// never leaves the device: every byte is read once, nothing is written but one 32-bit word.  CRC is linear over GF(2)
// (crc32_gf2.h), so the pass needs no order: every piece's raw CRC (zero init) is multiplied by x^(8 * its distance to the end)
// mod P and everything is xored together; init and final xor are one host-side term that depends on n alone.
//   - Any alignment: the first (-d mod 16) bytes and the last (n - head) mod 16 bytes are taken bytewise by one lane of
//     workgroup 0, the 16-byte units in between by all lanes.
//   - Lanes take INTERLEAVED units (lane l of L = grid x 256 takes l, l + L, ...: every wave load is 1 KB contiguous).  The
//     units are numbered from the END: `pad` zero units are thought in front of the first (leading zeros leave a raw CRC as it
//     is), so that every lane takes exactly `rounds` units and its last one lies 16 (L - 1 - l) bytes before the end of the
//     units -- a distance that depends on the lane alone.
//   - A lane's running value Y is kept L - 1 units AHEAD of its position, so that one step -- "advance by L units and take the
//     next one in" -- is Y' = ((Y x^96 + U) x^32) x^(128 (L - 1)): Y xored into the unit's first word, then sixteen byte look-ups
//     in tables T[j][v] = v x^(8 (16 L - j)) mod P (16 KB of LDS, built by the host for the launch's L, kept by the context).
//     The last unit is only xored in; the lane's four words W are then reduced with the lane's distance in one go,
//     sum_k W_k x^(32 (4 - k) + 128 (255 - lane in workgroup)): four shift-and-xor multiplications with constants from a table
//     that depends on nothing.
//   - The workgroup xors its lanes' values (shuffles, then LDS), multiplies by x^(8 * distance of its last unit to the end) --
//     square and multiply over the host's x^(8 2^k), one factor per lane of wave 0, multiplied up by shuffles -- and issues ONE
//     atomicXor.
// gfx950 has no carry-less multiply, so the work per byte is one LDS look-up (random addresses: bank conflicts as the data
// has them; equal bytes broadcast) and about four VALU instructions.  Measured (profiles/r08_crc32.json): 10^9 B
// in 182 us on text, 206 us on random bytes (5.5 / 4.9 TB/s: close to HBM, the difference is the LDS), 10^8 B in 34 us.
#include "common.h"
#include "crc32_gf2.h"

namespace bce {

namespace {

constexpr int CRC_T = 256;                   // lanes per workgroup (4 waves)
constexpr uint32_t CRC_MAX_GRID = 1024;      // workgroups at most (4 per CU)
constexpr uint32_t CRC_ROUNDS = 16;          // units per lane at most while the grid can still double (8..16 below the largest grid)
constexpr uint32_t CRC_TAB_WORDS = 16 * 256; // the launch's step tables
constexpr uint32_t CRC_LANE_WORDS = 4 * CRC_T;   // the lanes' final constants

constexpr uint32_t CRC_POW_WORDS = 64;       // x^(8 2^k) mod P
constexpr uint32_t CRC_RES_WORDS = 4;        // the result word (and padding), behind the tables: memory only this file touches

__device__ inline uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  #pragma unroll 8
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}

// x^(8 bytes) mod P in every lane of a full wave: lane k holds the factor of bit k of `bytes`, the 64 are multiplied up
__device__ inline uint32_t wave_xpow8(uint64_t bytes, uint32_t lane, const uint32_t *__restrict__ pw) {
  uint32_t f = ((bytes >> lane) & 1u) ? pw[lane] : kCrcOne;
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) f = mulmod(f, (uint32_t)__shfl_xor((int)f, d, 64));
  return f;
}

// raw CRC of a few bytes, bit by bit (the ragged ends: at most 15 bytes each)
__device__ inline uint32_t raw_bytes(const uint8_t *p, uint32_t count) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < count; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  }
  return c;
}

// d + head is 16-byte aligned; `units` 16-byte units follow it, then tail < 16 bytes.  rounds * lanes = units + pad, lanes = gridDim.x * CRC_T.
// *result (zeroed by the host) ends as the raw CRC of the head + 16 units + tail bytes.
__global__ __launch_bounds__(CRC_T) void crc32_kernel(const uint8_t *__restrict__ d, uint32_t head, uint64_t units, uint32_t tail,
                                                      uint64_t rounds, uint64_t pad, const uint32_t *__restrict__ step_tab,
                                                      const uint32_t *__restrict__ lane_tab, const uint32_t *__restrict__ pw, uint32_t *result) {
  __shared__ uint32_t tab[CRC_TAB_WORDS];
  __shared__ uint32_t wave_val[CRC_T / 64];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < CRC_TAB_WORDS; i += CRC_T) tab[i] = step_tab[i];
  __syncthreads();
  const uint64_t lanes = (uint64_t)gridDim.x * CRC_T;
  const uint4 *body = reinterpret_cast<const uint4 *>(d + head);
  uint64_t v = (uint64_t)blockIdx.x * CRC_T + tid;                 // this lane's unit of round 0, counted with the pad
  const uint4 zero = make_uint4(0, 0, 0, 0);
  uint32_t y = 0;
  auto step = [&](uint4 u) {
    u.x ^= y;
    y = tab[0 * 256 + (u.x & 0xFFu)] ^ tab[1 * 256 + ((u.x >> 8) & 0xFFu)] ^ tab[2 * 256 + ((u.x >> 16) & 0xFFu)] ^ tab[3 * 256 + (u.x >> 24)] ^
        tab[4 * 256 + (u.y & 0xFFu)] ^ tab[5 * 256 + ((u.y >> 8) & 0xFFu)] ^ tab[6 * 256 + ((u.y >> 16) & 0xFFu)] ^ tab[7 * 256 + (u.y >> 24)] ^
        tab[8 * 256 + (u.z & 0xFFu)] ^ tab[9 * 256 + ((u.z >> 8) & 0xFFu)] ^ tab[10 * 256 + ((u.z >> 16) & 0xFFu)] ^ tab[11 * 256 + (u.z >> 24)] ^
        tab[12 * 256 + (u.w & 0xFFu)] ^ tab[13 * 256 + ((u.w >> 8) & 0xFFu)] ^ tab[14 * 256 + ((u.w >> 16) & 0xFFu)] ^ tab[15 * 256 + (u.w >> 24)];
  };
  uint64_t k = 0;
  if (rounds > 1) {                                                 // round 0: the only one that can fall into the pad
    step(v >= pad ? body[v - pad] : zero);
    v += lanes; k = 1;
  }
  for (; k + 4 < rounds; k += 4, v += 4 * lanes) {                  // four loads in flight per lane
    const uint4 u0 = body[v - pad], u1 = body[v + lanes - pad], u2 = body[v + 2 * lanes - pad], u3 = body[v + 3 * lanes - pad];
    step(u0); step(u1); step(u2); step(u3);
  }
  for (; k + 1 < rounds; ++k, v += lanes) step(body[v - pad]);
  uint4 w = v >= pad ? body[v - pad] : zero;                        // the last round (v - pad < units: rounds * lanes = units + pad)
  w.x ^= y;
  const uint4 kk = reinterpret_cast<const uint4 *>(lane_tab)[tid];
  uint32_t mine = mulmod(w.x, kk.x) ^ mulmod(w.y, kk.y) ^ mulmod(w.z, kk.z) ^ mulmod(w.w, kk.w);
  #pragma unroll
  for (int s = 32; s >= 1; s >>= 1) mine ^= (uint32_t)__shfl_xor((int)mine, s, 64);
  if ((tid & 63u) == 0) wave_val[tid >> 6] = mine;
  __syncthreads();
  if (tid < 64) {                                                   // wave 0: the workgroup's value to its place, one atomic
    uint32_t g = wave_val[0] ^ wave_val[1] ^ wave_val[2] ^ wave_val[3];
    const uint64_t after = ((uint64_t)(gridDim.x - 1u - blockIdx.x) * CRC_T) * 16u + tail;   // bytes behind this workgroup's last unit
    g = mulmod(g, wave_xpow8(after, tid, pw));
    if (blockIdx.x == 0) {                                          // the two ragged ends
      const uint32_t hx = wave_xpow8(units * 16u + tail, tid, pw);
      if (tid == 0) {
        g ^= mulmod(raw_bytes(d, head), hx);
        g ^= raw_bytes(d + head + units * 16u, tail);
      }
    }
    if (tid == 0 && g) atomicXor(result, g);
  }
}

// The launch's tables, kept by the context from one call to the next: crc_tab = [16][256] step tables for `grid` workgroups, then
// the lanes' [256][4] final constants and the 64 powers x^(8 2^k) (which depend on nothing), then the result word.
// What the buffer holds is said by two fields of the context that are set only once an upload has COMPLETED: crc_const_ready (the
// constants) and crc_tab_grid (the step tables; 0 = none) -- an upload that fails leaves both saying "not there".
int crc_tables(bce_hip_ctx *c, uint32_t grid) {
  if (!c->crc_tab.p) { c->crc_const_ready = false; c->crc_tab_grid = 0; }
  BCE_TRY(ensure(c, c->crc_tab, (size_t)(CRC_TAB_WORDS + CRC_LANE_WORDS + CRC_POW_WORDS + CRC_RES_WORDS) * 4));
  const bool fresh = !c->crc_const_ready;
  if (!fresh && c->crc_tab_grid == grid) return BCE_HIP_OK;
  c->crc_tab_grid = 0;
  std::vector<uint32_t> h(fresh ? CRC_TAB_WORDS + CRC_LANE_WORDS + CRC_POW_WORDS : CRC_TAB_WORDS);
  // T[j][v] = v x^(8 (16 L - j)): the factor of j = 15 by square and multiply, each earlier j one more byte
  const uint64_t L = (uint64_t)grid * CRC_T;
  const uint32_t x8 = kCrcOne >> 8;
  uint32_t e = crc_xpow8(16 * L - 15);
  for (int j = 15; j >= 0; --j, e = crc_mulmod(e, x8)) {
    uint32_t *t = h.data() + j * 256;
    t[0] = 0;
    for (uint32_t b = 0; b < 8; ++b) {
      const uint32_t one = crc_mulmod(1u << b, e);
      for (uint32_t v = 0; v < (1u << b); ++v) t[(1u << b) | v] = one ^ t[v];
    }
  }
  if (fresh) {
    // K[l][k] = x^(32 (4 - k) + 128 (255 - l)): word k of a unit to the end of the workgroup's last unit
    const uint32_t x128 = crc_xpow8(16);
    uint32_t base = kCrcOne;                                        // x^(128 (255 - l)), from l = 255 down
    for (int l = CRC_T - 1; l >= 0; --l, base = crc_mulmod(base, x128))
      for (int k = 0; k < 4; ++k) h[CRC_TAB_WORDS + l * 4 + k] = crc_mulmod(base, crc_xpow8(4 * (4 - k)));
    memcpy(h.data() + CRC_TAB_WORDS + CRC_LANE_WORDS, crc_pow2().v, CRC_POW_WORDS * 4);
  }
  BCE_HIP_TRY(c, hipMemcpyAsync(c->crc_tab.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->stream));
  BCE_HIP_TRY(c, hipStreamSynchronize(c->stream));                 // (h goes away)
  c->crc_const_ready = true;
  c->crc_tab_grid = grid;
  return BCE_HIP_OK;
}

}  // namespace

// *crc = the CRC-32 of d[0, n).  d: device memory of the context's device, any alignment.  Queued on the context's stream behind
// whatever wrote the buffer; returns when the word is on the host.
int kd_crc32(bce_hip_ctx *c, const uint8_t *d, uint64_t n, uint32_t *crc) {
  *crc = 0;
  if (n == 0) return BCE_HIP_OK;
  const uint32_t head = (uint32_t)std::min<uint64_t>(n, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);
  const uint64_t units = (n - head) / 16;
  const uint32_t tail = (uint32_t)(n - head - units * 16);
  // the smallest power of two of workgroups (few different step tables) that leaves every lane CRC_ROUNDS units at most: 8..16 per
  // lane below the largest grid, which 64 MB reach, and as many as it takes from there on
  uint32_t grid = 1;
  while (grid < CRC_MAX_GRID && (uint64_t)grid * CRC_T * CRC_ROUNDS < units) grid <<= 1;
  const uint64_t lanes = (uint64_t)grid * CRC_T;
  const uint64_t rounds = std::max<uint64_t>(1, (units + lanes - 1) / lanes), pad = rounds * lanes - units;
  BCE_TRY(crc_tables(c, grid));
  // (the result word lies in this file's own buffer: a call between two stages of a compression -- bce_hip_input_crc32 is valid
  //  there -- must not touch the scratch words other stages keep in c->stat, K4's model counters among them)
  uint32_t *d_res = c->crc_tab.as<uint32_t>() + CRC_TAB_WORDS + CRC_LANE_WORDS + CRC_POW_WORDS;
  BCE_HIP_TRY(c, hipMemsetAsync(d_res, 0, 4, c->stream));
  hipLaunchKernelGGL(crc32_kernel, dim3(grid), dim3(CRC_T), 0, c->stream, d, head, units, tail, rounds, pad, c->crc_tab.as<uint32_t>(),
                     c->crc_tab.as<uint32_t>() + CRC_TAB_WORDS, c->crc_tab.as<uint32_t>() + CRC_TAB_WORDS + CRC_LANE_WORDS, d_res);
  BCE_HIP_TRY(c, hipGetLastError());
  uint32_t raw = 0;
  BCE_TRY(read_back(c, &raw, d_res, 4));
  BCE_HIP_TRY(c, hipGetLastError());
  *crc = raw ^ crc_init_term(n);
  return BCE_HIP_OK;
}

}  // namespace bce
