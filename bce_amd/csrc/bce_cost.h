// bce_cost.h -- the ideal code length of one range-coder step, in integers, shared by the cost kernel (k4_cost.hip, device) and
// the host (bce_hip_cost_q24, the size formula of bce_hip_estimate, the CPU tests).
//
// A step encode(cum, freq, total) (bce.cpp:520-529) narrows the coder's range by freq / total: log2(total / freq) bits.
//   cost_q24(freq, total) = L(total) - L(freq),   L(x) = log2(x) of a uint32_t x >= 1 in unsigned Q24 fixed point (2^24 = one bit)
// L is integer arithmetic only -- no floating point anywhere, so g++ and hipcc, host and device, give the same word for the same
// x, and sums of costs are uint64_t sums: independent of the order of the additions, two runs agree bit for bit.
//   L(x) = (e << 24) + T(m),  e = floor(log2 x),  m = x / 2^e in [1, 2) with 31 fraction bits,
//   T    = log2 of the mantissa: a table of kLog2Steps + 1 = 1025 Q24 words at the mantissas 1 + i / 1024, linear in between.
// The table is made at compile time by squaring (one bit of log2 m per squaring of m: m^2 >= 2 <=> the bit is 1), to 30 bits, then
// rounded to Q24.  What follows from this: L(2^k) = k << 24 exactly (T(1) = 0); L is monotone non-decreasing (T is, and the
// interpolation never passes the next entry); the error against log2 is the chord's, h^2 / (8 ln 2) with h = 2^-10 = 1.7e-7 bit,
// plus a rounding of 2^-25 and one truncation of 2^-24: below 2^-21 bit.  x < 2048 falls on table entries.
// Magnitudes: L <= 32 << 24 = 2^29, so a cost is below 2^29 and 2^35 steps fit a uint64_t sum.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "bce_core.h"

namespace bce {

constexpr uint32_t kLog2StepBits = 10;
constexpr uint32_t kLog2Steps = 1u << kLog2StepBits;

struct Log2Table { uint32_t t[kLog2Steps + 1]; };

// log2(m / 2^31) for 2^31 <= m < 2^32 in Q30, by squaring (uint64_t products of Q31 words, truncated: each truncation is a
// relative 2^-31 whose share of the result halves with every later bit, below 2^-29 in all)
constexpr uint32_t log2_mantissa_q30(uint64_t m) {
  uint32_t r = 0;
  for (int b = 0; b < 30; ++b) {
    m = (m * m) >> 31;                                    // [2^31, 2^33)
    r <<= 1;
    if (m >> 32) { r |= 1u; m >>= 1; }
  }
  return r;
}
constexpr Log2Table make_log2_table() {
  Log2Table tab{};
  for (uint32_t i = 0; i < kLog2Steps; ++i)
    tab.t[i] = (log2_mantissa_q30(((uint64_t)1 << 31) + ((uint64_t)i << (31 - kLog2StepBits))) + 32u) >> 6;   // Q30 -> Q24, rounded
  tab.t[kLog2Steps] = 1u << 24;
  return tab;
}
#if defined(__HIPCC__)
__device__ __constant__ constexpr Log2Table kLog2TableDev = make_log2_table();
#endif
constexpr Log2Table kLog2Table = make_log2_table();

BCE_HD uint32_t clz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__clz((int)x);
#else
  return (uint32_t)__builtin_clz(x);
#endif
}

// L(x) with the table given (the kernel reads its copy in LDS); x >= 1
BCE_HD uint32_t log2_q24_with(const uint32_t *tab, uint32_t x) {
  const uint32_t lz = clz32(x), e = 31u - lz;
  const uint32_t m = x << lz;                             // the mantissa, Q31
  const uint32_t i = (m >> (31 - kLog2StepBits)) & (kLog2Steps - 1u);
  const uint32_t f = m & ((1u << (31 - kLog2StepBits)) - 1u);   // 21 bits between two entries
  const uint32_t t0 = tab[i], t1 = tab[i + 1];
  return (e << 24) + t0 + (uint32_t)(((uint64_t)(t1 - t0) * f) >> (31 - kLog2StepBits));
}
BCE_HD uint32_t log2_q24(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return log2_q24_with(kLog2TableDev.t, x);
#else
  return log2_q24_with(kLog2Table.t, x);
#endif
}
// 1 <= freq <= total
BCE_HD uint32_t cost_q24(uint32_t freq, uint32_t total) { return log2_q24(total) - log2_q24(freq); }

// What the range coder (host_coder.cpp, RangeCoder::encode_run) does with one model record (bce_core.h pack_model_out), as cost:
// one uniform bit -- set(s & 1, 2), bce.cpp:507-510 -- per bit below the escape field's sentinel, then set(cum, freq, total).
BCE_HD uint32_t record_cost_q24_with(const uint32_t *tab, uint64_t o) {
  const uint32_t nesc = 31u - clz32(out_esc_sentinel(o));  // (the sentinel is never 0: 1 = no escape bits)
  return (nesc << 24) + log2_q24_with(tab, out_total(o)) - log2_q24_with(tab, out_freq(o));
}

// ---- from per-plane sums to bytes --------------------------------------------------------------------------------------------
// A coder's stream.  encode() pushes a word whenever the top 16 bits of its range are settled (shift_out, bce.cpp:655-661), so
// after B bits it has pushed the whole words of B and still holds the rest, up to 16 bits, in its 64-bit state.  flush()
// (:610-615; its own shift_out is a no-op behind encode()) pushes exactly ONE more word, which carries that rest: it is the
// rounding up to whole words.  So a stream is floor(B / 16) + 1 words, and an empty one (no step at all) that one word.
// (Rounding up AND adding the flush word counts one word per plane too many: +16 to +22 B on every input measured)
constexpr uint32_t kFlushWords = 1;
BCE_HD uint64_t stream_words_q24(uint64_t cost_q24_sum) { return cost_q24_sum / ((uint64_t)16 << 24) + kFlushWords; }

}  // namespace bce
