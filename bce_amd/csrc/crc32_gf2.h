// crc32_gf2.h -- arithmetic in GF(2)[x] / P for CRC-32 as zlib, gzip and PNG compute it (P reflected = 0xEDB88320), shared by
// the host routines (decoder.cpp: bce_hip_crc32, bce_hip_crc32_combine) and the device pass's host side (kd_crc32.hip).
//
// A 32-bit value is a polynomial of degree < 32 in REFLECTED order: bit 31 is the coefficient of x^0, bit 0 that of x^31 -- the
// order in which a little-endian word holds four message bytes, so a word of the message is its own polynomial.
// The "raw" CRC (zero init, no final xor) of a message M is M(x) x^32 mod P, which is linear:
//   raw(A || B) = raw(A) x^(8 |B|) + raw(B)        and        crc(M) = raw(M) + 0xFFFFFFFF x^(8 |M|) + 0xFFFFFFFF.
#pragma once
#include <stdint.h>

namespace bce {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;          // the polynomial 1

// a b mod P
inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - (a >> 31));                     // a's coefficient of x^i, with b = b0 x^i
    a <<= 1;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}

// x^(8 * 2^k) mod P for k = 0..63: what square and multiply walks over (also handed to the device pass)
struct CrcPow2 {
  uint32_t v[64];
  CrcPow2() {
    uint32_t p = kCrcOne >> 8;                     // x^8
    for (int k = 0; k < 64; ++k) { v[k] = p; p = crc_mulmod(p, p); }
  }
};
inline const CrcPow2 &crc_pow2() { static const CrcPow2 t; return t; }

// x^(8 bytes) mod P
inline uint32_t crc_xpow8(uint64_t bytes) {
  const CrcPow2 &t = crc_pow2();
  uint32_t p = kCrcOne;
  for (int k = 0; bytes; ++k, bytes >>= 1)
    if (bytes & 1u) p = crc_mulmod(p, t.v[k]);
  return p;
}

// what the init and the final xor add to the raw CRC of n bytes
inline uint32_t crc_init_term(uint64_t n) { return crc_mulmod(0xFFFFFFFFu, crc_xpow8(n)) ^ 0xFFFFFFFFu; }

}  // namespace bce
