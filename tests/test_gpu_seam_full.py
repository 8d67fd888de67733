"""GPU: the rest of the libdivsufsort seam (libdivsufsort_hip.so through ctypes, as tests/test_gpu_seam.py): divsufsort against
tests/sa_ref.py, bw_transform against divbwt, sufcheck's return values on divsufsort's output and on planted defects, its verbose
line, and sa_search on a GPU-made array against the index's own locate."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bce_amd
import oracle
import sa_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
I32, VP = C.c_int32, C.c_void_p
LIB = os.path.join(ROOT, "bce_amd", "lib", "libdivsufsort_hip.so")


@pytest.fixture(scope="module")
def seam():
    L = C.CDLL(LIB)
    L.divbwt.argtypes, L.divbwt.restype = [VP, VP, VP, I32], I32
    L.divsufsort.argtypes, L.divsufsort.restype = [VP, VP, I32], I32
    L.bw_transform.argtypes, L.bw_transform.restype = [VP, VP, VP, I32, VP], I32
    L.sufcheck.argtypes, L.sufcheck.restype = [VP, VP, I32, I32], I32
    L.sa_search.argtypes, L.sa_search.restype = [VP, I32, VP, I32, VP, I32, VP], I32
    return L


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def sort(L, t):
    a, sa = u8(t), np.full(len(t), -9, dtype=np.int32)
    assert L.divsufsort(a.ctypes.data, sa.ctypes.data, len(a)) == 0
    assert a.tobytes() == bytes(t)
    return sa


def check(L, t, sa, verbose=0):
    a, s = u8(t), np.ascontiguousarray(sa).view(np.int32)
    return L.sufcheck(a.ctypes.data, s.ctypes.data, len(a), verbose)


@pytest.fixture(scope="module")
def big(seam):
    t = oracle.synth_text(3, 1 << 20)
    return t, sort(seam, t)


def test_divsufsort_on_small_texts(seam):
    rs = np.random.RandomState(5)
    cases = [b"ab", b"ba", b"aa", b"abracadabra", b"banana", b"\x00\x00\x01\x00", b"\xff" * 7, b"ab" * 9, bytes(range(256)), b"a" * 5000, b"ab" * 4000,
             b"abc" * 3333 + b"ab", oracle.synth_text(1, 2049), oracle.synth_rand(2, 2047)]
    for _ in range(60):
        cases.append(bytes(rs.choice([0, 1, 97, 98, 255], int(rs.randint(2, 60))).astype(np.uint8)))
    for t in cases:
        sa = sort(seam, t)
        assert np.array_equal(sa, sa_ref.suffix_array(t)), t[:40]
        assert check(seam, t, sa) == 0


def test_divsufsort_at_a_megabyte(seam, big):
    t, sa = big
    assert sa_ref.check(t, sa) == (sa_ref.OK, sa_ref.NONE)
    assert sa_ref.bwt_of(t, sa) == oracle.divbwt(t)
    assert check(seam, t, sa) == 0


@pytest.mark.parametrize("t", [b"banana", b"ab" * 4000, oracle.synth_text(9, 300001), oracle.synth_rand(4, 65537)], ids=["banana", "ab4000", "text", "rand"])
def test_bw_transform_is_divbwt(seam, t):
    a, want = u8(t), np.empty(len(t), dtype=np.uint8)
    p = seam.divbwt(a.ctypes.data, want.ctypes.data, None, len(a))
    assert (want.tobytes(), p) == oracle.divbwt(t)
    u, idx = np.empty_like(a), I32(-9)
    assert seam.bw_transform(a.ctypes.data, u.ctypes.data, None, len(a), C.byref(idx)) == 0
    assert idx.value == p and np.array_equal(u, want) and a.tobytes() == bytes(t)
    work = np.full(len(a) + 1, -9, dtype=np.int32)                          # a workspace is accepted, and T == U
    idx = I32(-9)
    assert seam.bw_transform(a.ctypes.data, a.ctypes.data, work.ctypes.data, len(a), C.byref(idx)) == 0
    assert idx.value == p and np.array_equal(a, want)


def test_sufcheck_return_values(seam, big):
    t, sa = big
    n = len(t)
    tb = np.frombuffer(t, dtype=np.uint8)
    m = sa.copy(); m[n - 1] = n
    assert check(seam, t, m) == -2
    m = sa.copy(); m[0] = -1
    assert check(seam, t, m) == -2
    first = int(np.flatnonzero(tb[sa[:-1]] != tb[sa[1:]])[0]) + 1           # rows first - 1 and first differ in their first byte
    m = sa.copy(); m[[first - 1, first]] = m[[first, first - 1]]
    assert sa_ref.check(t, m) == (sa_ref.ORDER, first) and check(seam, t, m) == -3
    same = int(np.flatnonzero(tb[sa[:-1]] == tb[sa[1:]])[1000]) + 1          # ... and these share it
    m = sa.copy(); m[[same - 1, same]] = m[[same, same - 1]]
    got = sa_ref.check(t, m)
    assert got[0] == sa_ref.ORDER and tb[m[got[1] - 1]] == tb[m[got[1]]] and check(seam, t, m) == -4
    m = sa.copy(); m[7] = m[8]
    assert sa_ref.check(t, m)[0] == sa_ref.MISSING and check(seam, t, m) == -4


SCRIPT = """
import ctypes as C, sys
import numpy as np
L = C.CDLL(sys.argv[1])
L.sufcheck.argtypes, L.sufcheck.restype = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32], C.c_int32
t = np.frombuffer(b"banana", dtype=np.uint8).copy()
for sa in ([5, 3, 1, 0, 4, 2], [5, 3, 1, 4, 0, 2], [5, 3, 1, 0, 4, 6]):
    s = np.array(sa, dtype=np.int32)
    print("rc", L.sufcheck(t.ctypes.data, s.ctypes.data, 6, 1), flush=True)
s = np.array([5, 3, 1, 4, 0, 2], dtype=np.int32)
print("quiet", L.sufcheck(t.ctypes.data, s.ctypes.data, 6, 0), flush=True)
"""


def test_the_verbose_line_goes_to_stderr(tmp_path):
    """A process of its own: the line is written by C code, past Python's sys.stderr."""
    script = tmp_path / "verbose.py"
    script.write_text(SCRIPT)
    r = subprocess.run([sys.executable, str(script), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:4] == ["rc 0", "rc -3", "rc -2", "quiet -3"]
    lines = [x for x in r.stderr.split("\n") if x.startswith("sufcheck: ")]
    assert len(lines) == 3, r.stderr
    assert "6 suffixes in order" in lines[0] and "row 4" in lines[1] and "SA[5]=6" in lines[2]
    assert "sufcheck" not in r.stdout


def test_sa_search_agrees_with_the_index(seam):
    t = oracle.synth_text(21, 200000)
    sa = sort(seam, t)
    pats = [b"the", b"and ", b"e", t[1000:1012], t[-5:], t[-1:], b"qzqzq", t[:40], t[150000:150003]]
    hits = bce_amd.locate(t, pats, cyclic=False)
    T, S = u8(t), sa
    for p, where in zip(pats, hits):
        P, idx = u8(p), I32(-9)
        count = seam.sa_search(T.ctypes.data, len(T), P.ctypes.data, len(P), S.ctypes.data, len(S), C.byref(idx))
        assert count == len(where), p
        assert np.array_equal(np.sort(sa[idx.value:idx.value + count]).astype(np.uint32), np.asarray(where, dtype=np.uint32)), p
