"""CPU: the reference of `bce -s`'s records (tests/scanrec_ref.py) before the kernels are held against it
(tests/test_gpu_scan_routes.py): the numpy scan_pack against bce_core.h's own, the host ScanCoder against the oracle on every
input family of the scan-mode tests, and that the families hold the rows they are there for."""
import ctypes as C

import numpy as np
import pytest

import scanrec_ref as ref
from model_cases import load_emul

ALL = list(ref.FAMILIES)


@pytest.fixture(scope="module")
def emul():
    L = load_emul()
    L.emul_scan.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    L.emul_scan_pack.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.emul_scan_pack.restype = None
    return L


def core_scan_pack(L, syms6):
    syms6 = np.ascontiguousarray(syms6, dtype=np.uint32)
    out = np.empty(len(syms6), dtype=np.uint32)
    L.emul_scan_pack(syms6.ctypes.data, len(syms6), out.ctypes.data)
    return out


def numpy_scan_pack(syms6):
    return ref.scan_pack(syms6[:, 1], syms6[:, 2], syms6[:, 3], syms6[:, 4], syms6[:, 5])


_traces = {}


def trace(name):
    if name not in _traces:
        _traces[name] = ref.trace_syms(ref.family_input(name))
    return _traces[name]


@pytest.mark.parametrize("name", ALL)
def test_numpy_scan_pack_equals_the_headers_on_every_trace_row(emul, name):
    syms = trace(name)
    if len(syms) == 0:
        return
    assert (numpy_scan_pack(syms) == core_scan_pack(emul, syms)).all()


def test_numpy_scan_pack_equals_the_headers_at_the_edges(emul):
    """k at both sides of the escape (31, 32, 33), of a second halving (63, 64) and far above; sym at both ends; c1 and c2 at both
    sides of 2^24, where c << 8 wraps in uint32; cs up to 2^31 - 1, always with c < cs."""
    rows = []
    W = 1 << 24
    for k in (2, 31, 32, 33, 63, 64, 1 << 20, (1 << 31) - 1):
        for sym in (0, k - 1, k // 2, 1):
            for cs in (W - 1, W, W + 1, W + 2, 3 * W + 5, (1 << 30) + 1, (1 << 31) - 1, 2, 255, 256, 257):
                for c1 in (0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, cs - 1, cs // 2):
                    for c2 in (0, W - 1, W, W + 1, cs - 1, cs // 3):
                        if c1 < cs and c2 < cs:
                            rows.append((0, sym, k, c1, c2, cs))
    rs = np.random.RandomState(9)
    for _ in range(20000):
        k = int(rs.randint(2, 1 << int(rs.randint(2, 32))))
        cs = int(rs.randint(2, 1 << int(rs.randint(2, 32))))
        rows.append((0, int(rs.randint(0, max(k, 1))) % k if k > 1 else 0, max(k, 2), int(rs.randint(0, cs)), int(rs.randint(0, cs)), cs))
    rows = np.array(rows, dtype=np.uint32)
    wrapped = (rows[:, 3].astype(np.uint64) << np.uint64(8)) >= (1 << 32)
    assert wrapped.sum() > 1000 and (~wrapped).sum() > 1000
    got, want = numpy_scan_pack(rows), core_scan_pack(emul, rows)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (rows[bad[0]].tolist(), ref.unpack(got[bad[0]]), ref.unpack(want[bad[0]]))
    # every field stays inside its bits: sym < k <= 31, both quotients below 256
    assert (((got >> 5) & 31) >= 2).all() and ((got & 31) < ((got >> 5) & 31)).all() and (got >> 31 == 0).all()
    # and a few words worked out by hand from bce_core.h's text
    assert int(ref.scan_pack(0, 2, 0, 0, 1)[0]) == 2 << 5
    assert int(ref.scan_pack(30, 31, 1, 2, 4)[0]) == 30 | (31 << 5) | (64 << 10) | (128 << 18)
    # k = 33, s = 5: one escape, s -> 2, k -> 16 + (~5 & 1) = 16;  c1 = 2^24 wraps to 0, c2 = 2^24 - 1 -> 0xFFFFFF00 / (2^24 + 1) = 255
    assert int(ref.scan_pack(5, 33, W, W - 1, W + 1)[0]) == 2 | (16 << 5) | (0 << 10) | (255 << 18) | (1 << 26)
    # k = 64, s = 62: 64 -> 32 + 1 = 33 (s 31) -> 16 + 0 = 16 (s 15): two escapes; AdaptiveCoder's halving would give 32 -> 16
    assert int(ref.scan_pack(62, 64, 0, 0, 9)[0]) == 15 | (16 << 5) | (2 << 26)


@pytest.mark.parametrize("name", ALL)
def test_host_scan_coder_equals_the_oracle_on_every_family(emul, name):
    """emul_scan (scan_coder.cpp behind bce_core.h's scan_pack) on the trace rows == oracle.scan, table and doubles: the host
    half of `bce -s` is right on these inputs, so a failure of the GPU tests points at the kernels."""
    syms = trace(name)
    _, cfg, res = ref.family_reference(name)
    for threads, chunks in ((0, 1), (5, 3)):
        out = np.zeros(288, dtype=np.uint8)
        r9 = np.zeros(9, dtype=np.float64)
        emul.emul_scan(syms.ctypes.data, len(syms), threads, chunks, out.ctypes.data, r9.ctypes.data)
        assert out.tobytes() == cfg, (threads, chunks)
        assert tuple(r9) == res, (threads, chunks)


@pytest.mark.parametrize("name", ALL)
def test_expected_streams_hold_every_trace_row_once(name):
    syms = trace(name)
    streams, _, _ = ref.family_reference(name)
    assert [len(s) for s in streams] == [int((syms[:, 0] == p).sum()) for p in range(8)]
    assert sum(len(s) for s in streams) == len(syms)


# What the oracle's trace of each family holds: (rows, rows with k > 31 -- the escape loop --, rows with k == 2).  The figures
# are the reference's own (they do not come from the code under test); they say that the family still holds what it is there
# for: thousands of escapes and binary symbols in the text and table inputs, no row at all where every plane is constant,
# no binary symbol where every rotation has a twin (periodic-halves), exactly one row per period in the pure "ab" run.
ROWS = {
    "nonode-a": (0, 0, 0), "nonode-d2x14": (0, 0, 0), "nonode-zeros-1000": (0, 0, 0), "nonode-ab-x7": (2, 0, 0),
    "edge-one-byte": (0, 0, 0), "edge-two-equal": (0, 0, 0), "edge-constant-100": (0, 0, 0),
    "edge-period2-100": (2, 2, 0), "edge-period3-99": (4, 4, 0), "edge-all-bytes": (2040, 120, 0),
    "text-64k": (125416, 4551, 65741), "rand-64k": (396093, 10195, 238638),
    "repeat": (458370, 19045, 261590), "copies": (103081, 4422, 55895),
    "stair-zeros": (124160, 4202, 68908), "stair-ff": (122185, 4201, 66828), "stair-period2": (121171, 4209, 65914),
    "stair-period3": (296760, 8508, 178068), "stair-period7-in-random": (364063, 9016, 220130),
    "stair-two-regions": (125485, 4202, 70234), "stair-at-start": (121685, 4213, 66422), "stair-at-end": (119142, 4195, 63895),
    "stair-record-table": (118233, 4331, 61530), "stair-period2-twice": (123194, 4209, 67933),
    "stair-three-regions-phases": (245968, 5814, 151358), "stair-many-zero-runs": (147821, 4198, 77566),
    "stair-same-length-twice": (120198, 4203, 59934), "stair-whole-text-periodic": (30003, 2, 30001),
    "stair-two-tables-first-at-start": (135867, 4210, 80608),
    "periodic-ab-c": (30003, 2, 30001), "periodic-halves": (221158, 16223, 0), "periodic-halves-hash": (221192, 16223, 47),
    "spine": (107203, 2822, 54206),
}


@pytest.mark.parametrize("name", ALL)
def test_families_hold_escapes_and_binary_symbols(name):
    syms = trace(name)
    rows, big, two = len(syms), int((syms[:, 2] > 31).sum()), int((syms[:, 2] == 2).sum())
    print("%s: n = %d, %d rows, %d with k > 31, %d with k == 2" % (name, len(ref.family_input(name)), rows, big, two))
    if name in ROWS:
        assert (rows, big, two) == ROWS[name]
    else:                                      # the other edge inputs: some rows, and both kinds from a few thousand bytes on
        assert rows > 0 and two > 0
        assert big > 0 or len(ref.family_input(name)) < 95
