"""CPU: libdivsufsort_hip.so beyond the two calls of the reference -- the six further names of libdivsufsort's 32-bit API are declared
(include/divsufsort_hip.h) and exported; the two searches, plain host code, against tests/sa_ref.py; and everything divsufsort,
bw_transform and sufcheck answer without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import sa_ref
from conftest import ROOT

DECLARATIONS = [
    "saidx_t divbwt(const sauchar_t *T, sauchar_t *U, saidx_t *A, saidx_t n);",
    "saint_t inverse_bw_transform(const sauchar_t *T, sauchar_t *U, saidx_t *A, saidx_t n, saidx_t idx);",
    "saint_t divsufsort(const sauchar_t *T, saidx_t *SA, saidx_t n);",
    "saint_t bw_transform(const sauchar_t *T, sauchar_t *U, saidx_t *SA, saidx_t n, saidx_t *idx);",
    "saint_t sufcheck(const sauchar_t *T, const saidx_t *SA, saidx_t n, saint_t verbose);",
    "saidx_t sa_search(const sauchar_t *T, saidx_t Tsize, const sauchar_t *P, saidx_t Psize, const saidx_t *SA, saidx_t SAsize, saidx_t *idx);",
    "saidx_t sa_simplesearch(const sauchar_t *T, saidx_t Tsize, const saidx_t *SA, saidx_t SAsize, saint_t c, saidx_t *idx);",
    "const char *divsufsort_version(void);",
]
I32, VP = C.c_int32, C.c_void_p


@pytest.fixture(scope="module")
def seam():
    L = C.CDLL(os.path.join(ROOT, "bce_amd", "lib", "libdivsufsort_hip.so"))
    L.divsufsort.argtypes, L.divsufsort.restype = [VP, VP, I32], I32
    L.bw_transform.argtypes, L.bw_transform.restype = [VP, VP, VP, I32, VP], I32
    L.sufcheck.argtypes, L.sufcheck.restype = [VP, VP, I32, I32], I32
    L.sa_search.argtypes, L.sa_search.restype = [VP, I32, VP, I32, VP, I32, VP], I32
    L.sa_simplesearch.argtypes, L.sa_simplesearch.restype = [VP, I32, VP, I32, I32, VP], I32
    L.divsufsort_version.argtypes, L.divsufsort_version.restype = [], C.c_char_p
    return L


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def search(L, t, sa, p, rows=None, with_idx=True):
    """(count, idx) of sa_search over the first `rows` rows; idx None when NULL was passed"""
    T, P, S = u8(t), u8(p) if len(p) else np.zeros(1, dtype=np.uint8), np.ascontiguousarray(sa, dtype=np.int32)
    idx = I32(-77)
    got = L.sa_search(T.ctypes.data, len(t), P.ctypes.data, len(p), S.ctypes.data, len(S) if rows is None else rows, C.byref(idx) if with_idx else None)
    return got, idx.value if with_idx else None


def simple(L, t, sa, c, with_idx=True):
    T, S = u8(t), np.ascontiguousarray(sa, dtype=np.int32)
    idx = I32(-77)
    got = L.sa_simplesearch(T.ctypes.data, len(t), S.ctypes.data, len(S), c, C.byref(idx) if with_idx else None)
    return got, idx.value if with_idx else None


def test_the_header_declares_and_the_library_exports_all_eight():
    src = open(os.path.join(ROOT, "include", "divsufsort_hip.h")).read()
    L = C.CDLL(os.path.join(ROOT, "bce_amd", "lib", "libdivsufsort_hip.so"))
    for line in DECLARATIONS:
        assert line in src, line
        name = line.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(L, name), name
    assert "bce_hip_locate" in src                                         # the batched GPU equivalent of the searches is named


def test_version_string(seam):
    assert seam.divsufsort_version().decode().startswith("2.")


def test_sa_search_against_the_reference(seam):
    rs = np.random.RandomState(23)
    texts = [b"abracadabra", b"banana", b"aaaaaaa", b"\x00\x00\x01\x00", b"ab" * 20 + b"a", bytes(range(256))]
    for _ in range(60):
        texts.append(bytes(rs.choice([0, 97, 98, 99, 255], int(rs.randint(1, 70))).astype(np.uint8)))
    for t in texts:
        sa = sa_ref.suffix_array(t)
        n = len(t)
        pats = {t[i:i + m] for i in range(0, n, max(1, n // 7)) for m in (1, 2, 3, 5, n)}          # present, suffixes that end at n included
        pats |= {t + b"a", t[-2:] + b"\x00", b"zzz", b"\x00", b"\xff\xff", t[:3] + b"\x01\x02"}   # longer than the text, absent, past a short suffix
        for p in sorted(pats):
            if not p:
                continue
            want = sa_ref.search(t, sa, p)
            assert search(seam, t, sa, p) == want, (t, p)
            assert search(seam, t, sa, p, with_idx=False) == (want[0], None)
            if want[0]:
                assert sorted(int(s) for s in sa[want[1]:want[1] + want[0]]) == [i for i in range(n) if t.startswith(p, i)]
        for rows in (1, n // 2, n - 1):                                    # SAsize < Tsize: the first rows alone
            if rows >= 1:
                p = t[int(sa[0]):int(sa[0]) + 2]
                assert search(seam, t, sa, p, rows=rows) == sa_ref.search(t, sa[:rows], p), (t, rows)
        assert search(seam, t, sa, b"") == (n, 0)                          # the empty pattern: every row
        for c in sorted(set(t)) + [1, 254]:
            assert simple(seam, t, sa, c) == sa_ref.search(t, sa, bytes([c])), (t, c)
            assert simple(seam, t, sa, c, with_idx=False)[0] == sa_ref.search(t, sa, bytes([c]))[0]


def test_searches_refuse_bad_arguments(seam):
    t, sa, p = u8(b"banana"), np.array([5, 3, 1, 0, 4, 2], dtype=np.int32), u8(b"an")
    T, S, P = t.ctypes.data, sa.ctypes.data, p.ctypes.data
    idx = I32(5)
    assert seam.sa_search(T, 6, P, 2, S, 6, C.byref(idx)) == 2 and idx.value == 1
    assert seam.sa_search(None, 6, P, 2, S, 6, None) == -1 and seam.sa_search(T, 6, None, 2, S, 6, None) == -1
    assert seam.sa_search(T, 6, P, 2, None, 6, None) == -1
    assert seam.sa_search(T, -1, P, 2, S, 6, None) == -1 and seam.sa_search(T, 6, P, -1, S, 6, None) == -1 and seam.sa_search(T, 6, P, 2, S, -1, None) == -1
    assert seam.sa_search(T, 0, P, 2, S, 6, None) == 0 and seam.sa_search(T, 6, P, 2, S, 0, None) == 0
    assert seam.sa_search(T, 6, P, 0, S, 4, C.byref(idx)) == 4 and idx.value == 0
    assert seam.sa_simplesearch(None, 6, S, 6, 97, None) == -1 and seam.sa_simplesearch(T, 6, None, 6, 97, None) == -1
    assert seam.sa_simplesearch(T, -1, S, 6, 97, None) == -1 and seam.sa_simplesearch(T, 6, S, -1, 97, None) == -1
    assert seam.sa_simplesearch(T, 0, S, 6, 97, None) == 0 and seam.sa_simplesearch(T, 6, S, 0, 97, None) == 0
    assert seam.sa_simplesearch(T, 6, S, 6, 97, C.byref(idx)) == 3 and idx.value == 0


def test_what_the_sorting_calls_answer_without_a_gpu(seam):
    a, sa, idx = u8(b"banana"), np.full(6, -9, dtype=np.int32), I32(-9)
    A, S = a.ctypes.data, sa.ctypes.data
    assert seam.divsufsort(None, S, 6) == -1 and seam.divsufsort(A, None, 6) == -1 and seam.divsufsort(A, S, -1) == -1
    assert seam.divsufsort(A, S, 0) == 0
    assert seam.bw_transform(None, A, None, 6, C.byref(idx)) == -1 and seam.bw_transform(A, None, None, 6, C.byref(idx)) == -1
    assert seam.bw_transform(A, A, None, 6, None) == -1 and seam.bw_transform(A, A, None, -1, C.byref(idx)) == -1
    assert seam.sufcheck(None, S, 6, 0) == -1 and seam.sufcheck(A, None, 6, 0) == -1 and seam.sufcheck(A, S, -1, 0) == -1
    assert seam.sufcheck(A, S, 0, 0) == 0
    assert (sa == -9).all() and idx.value == -9 and a.tobytes() == b"banana"          # nothing was written


def test_texts_of_one_byte_and_none(seam):
    a, u, sa, idx = u8(b"x"), u8(b"?"), np.full(2, -9, dtype=np.int32), I32(-9)
    assert seam.divsufsort(a.ctypes.data, sa.ctypes.data, 1) == 0 and list(sa) == [0, -9]
    assert seam.bw_transform(a.ctypes.data, u.ctypes.data, None, 1, C.byref(idx)) == 0 and u.tobytes() == b"x" and idx.value == 1
    assert seam.bw_transform(a.ctypes.data, a.ctypes.data, sa.ctypes.data, 1, C.byref(idx)) == 0 and a.tobytes() == b"x"   # in place, with a workspace
    u[0] = 63
    assert seam.bw_transform(a.ctypes.data, u.ctypes.data, None, 0, C.byref(idx)) == 0 and idx.value == 0 and u.tobytes() == b"?"
