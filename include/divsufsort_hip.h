/*
 * divsufsort_hip.h -- libdivsufsort's 32-bit C ABI, first of all the two calls of akamiru/bce, served by the MI355X rotation
 * sorter (K1), the GPU inverse BWT and the GPU suffix-array checker of libbcehip.so.  Link libdivsufsort_hip.so (bce_amd/lib) in place of libdivsufsort and an UNMODIFIED
 * bce.cpp resolves its two calls here:
 *     bce.cpp:901    divbwt(file_.data(), file_.data(), 0, file_.size() - 1)
 *     bce.cpp:1091   inverse_bw_transform(out.data(), out.data(), nullptr, n, 1)
 * Types and signatures are libdivsufsort's (divsufsort.h: sauchar_t = uint8_t, saidx_t = saint_t = int32_t); install this
 * file as divsufsort.h, or keep libdivsufsort's own header -- the two declare the same functions.
 *
 * The functions use one process-wide GPU context (device $BCE_HIP_DEVICE, default 0), created on first use and guarded
 * by a mutex; buffers are host pointers, T and U may be the same buffer (bce calls them in place); the workspace A is
 * ignored (libdivsufsort allocates its own when it is NULL, which is what bce passes).
 */
#ifndef DIVSUFSORT_HIP_H
#define DIVSUFSORT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint8_t sauchar_t;
typedef int32_t saint_t;
typedef int32_t saidx_t;

/* Burrows-Wheeler transform of T[0, n) with an implicit smallest sentinel: U[0] = T[n-1], then T[SA[i] - 1] for the
 * suffixes in sorted order with the suffix 0 left out.  Returns its 1-based position (the primary index, 1..n), 0 for
 * n = 0, -1 on bad arguments, -2 when memory (host or device) runs out or no GPU is usable.  n < 2^31 - 1. */
saidx_t divbwt(const sauchar_t *T, sauchar_t *U, saidx_t *A, saidx_t n);

/* Inverse of divbwt: T = the transformed bytes, idx = the primary index it returned; U receives the text.
 * Returns 0, -1 on bad arguments (idx outside 1..n for n > 0, or bytes that are no BWT), -2 as above. */
saint_t inverse_bw_transform(const sauchar_t *T, sauchar_t *U, saidx_t *A, saidx_t n, saidx_t idx);

/* ---- the rest of libdivsufsort's 32-bit API -------------------------------------------------------------------------------
 * libdivsufsort's own header was not at hand when these were written: the names, signatures and return values below are
 * set down from knowledge of that library (divsufsort.h 2.0.x), and where this library adds a value it says so. */

/* The suffix array of T[0, n): SA[r] = the start of the r-th smallest suffix (a suffix that is a prefix of another sorts before
 * it).  The sort divbwt runs, with its order kept (bce_hip_suffix_array).  Returns 0, -1 on bad arguments (a null pointer,
 * n < 0), -2 when memory runs out or no GPU is usable.  n == 0 returns 0 and n == 1 gives SA[0] = 0, both without a GPU.
 * n < 2^31 - 1. */
saint_t divsufsort(const sauchar_t *T, saidx_t *SA, saidx_t n);

/* divbwt with the primary index stored in *idx: the same U, *idx = what divbwt returns, T == U allowed.  SA is workspace: it may
 * be NULL and is ignored.  n <= 1: U[0] = T[0] when n == 1, *idx = n.  Returns 0, -1 on bad arguments (a null T, U or idx,
 * n < 0), -2 as above. */
saint_t bw_transform(const sauchar_t *T, sauchar_t *U, saidx_t *SA, saidx_t n, saidx_t *idx);

/* Checks that SA[0, n) is the suffix array of T[0, n), on the GPU in linear time (bce_hip_sufcheck).  Callers test for 0:
 *    0  sorted (n == 0 included);          -1  bad arguments (a null pointer, n < 0);
 *   -2  an entry outside [0, n);           -3  two neighbouring rows whose first bytes are out of order;
 *   -4  any other fault: two neighbouring rows with equal first bytes in the wrong order, or an array that is no permutation;
 *   -5  THIS LIBRARY'S ADDITION: not checked, because memory ran out or no GPU is usable (libdivsufsort's own checker runs on
 *       the host and cannot fail that way).
 * With verbose != 0 one line goes to stderr that names the row or the text position. */
saint_t sufcheck(const sauchar_t *T, const saidx_t *SA, saidx_t n, saint_t verbose);

/* Binary searches over the caller's host arrays: plain host code, no context and no GPU (the batched GPU equivalent is
 * bce_hip_locate of bce_hip.h).  Returns the number of rows of SA[0, SAsize) whose suffix of T[0, Tsize) starts with
 * P[0, Psize) -- all Psize bytes present: a suffix shorter than P that is a prefix of P sorts before the matches and does not
 * count -- or with the byte c; *idx (idx may be NULL) = the first such row, or the row in front of which they would stand where
 * there is none.  SA must be sorted over the rows given; SAsize may be smaller than Tsize.  Bad arguments (a null T, P or SA, a
 * negative size): -1, *idx = -1.  Tsize == 0 or SAsize == 0: 0, *idx = -1.  Psize == 0: SAsize, *idx = 0. */
saidx_t sa_search(const sauchar_t *T, saidx_t Tsize, const sauchar_t *P, saidx_t Psize, const saidx_t *SA, saidx_t SAsize, saidx_t *idx);
saidx_t sa_simplesearch(const sauchar_t *T, saidx_t Tsize, const saidx_t *SA, saidx_t SAsize, saint_t c, saidx_t *idx);

/* The version of the API this library follows, with "-hip" appended. */
const char *divsufsort_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DIVSUFSORT_HIP_H */
