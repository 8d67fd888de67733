"""The inputs of tests/test_gpu_unbwt.py for the fill and access kernels: byte arrays, their planes by tests/unbwt_ref.py and sparse
boundary-rank arrays made from them.  tests/test_unbwt_ref_cpu.py checks every one of them against the kernels' precondition on
the CPU, so the builders are deterministic and shared."""
import numpy as np

import unbwt_ref as ref

# around a 32-position word, a 96-position granule, and one, two and three 8192-position chunks of the fill kernels
FILL_SIZES = [1, 2, 3, 31, 32, 33, 95, 96, 97, 8191, 8192, 8193, 16383, 16384, 16385, 24575, 24576, 24577]


class Case:
    def __init__(self, name, data, keep=None, planes=None):
        self.name = name
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.n = len(self.data)
        self.bits, self.zeros, self.R_full, self.words, self.rankw = planes if planes is not None else ref.planes_of(self.data)
        if isinstance(keep, str) and keep == "all":
            self.R = self.R_full.copy()
        else:
            self.R = ref.sparse_ranks(self.R_full, self.bits, keep)

    def planes(self):
        return self.bits, self.zeros, self.R_full, self.words, self.rankw


def runs_of(rs, n, longest, symbols=256):
    """Runs of random lengths 1 .. longest of random bytes: long constant gaps on every level."""
    out = np.empty(n, dtype=np.uint8)
    i = 0
    while i < n:
        l = int(rs.randint(1, longest + 1))
        out[i:i + l] = rs.randint(0, symbols)
        i += l
    return out


def edge_indices(n):
    """Boundaries on both sides of every chunk edge, and at the first position of words and granules."""
    k = np.arange(0, n // ref.FG_CHUNK + 2) * ref.FG_CHUNK
    idx = np.concatenate([k - 1, k, k + 1, np.arange(0, n + 1, 32), np.arange(0, n + 1, 96), np.arange(31, n + 1, 32), np.arange(95, n + 1, 96)])
    return idx[(idx >= 0) & (idx <= n)]


def fill_cases(n):
    """Four kinds of bytes x four sets of known boundaries, and the forced edges."""
    rs = np.random.RandomState(1000 + n)
    kinds = [("random", rs.randint(0, 256, n).astype(np.uint8)),
             ("two-symbols", rs.choice([0x41, 0x43], n).astype(np.uint8)),              # six constant levels
             ("three-symbols", rs.choice([0x00, 0x10, 0xFF], n).astype(np.uint8)),
             ("runs", runs_of(rs, n, 20000))]
    for kind, data in kinds:
        planes = ref.planes_of(data)
        for label, keep in (("minimal", None), ("all", "all"), ("plus-1%", rs.rand(8, n + 1) < 0.01), ("plus-50%", rs.rand(8, n + 1) < 0.5),
                            ("edges", edge_indices(n))):
            yield Case("%s/%s/n=%d" % (kind, label, n), data, keep, planes)


def only_boundary_case(at, n=20000):
    """Level 0 with one bit change, at index `at`: its only known interior boundary.  The other levels are random."""
    rs = np.random.RandomState(at)
    data = (rs.randint(0, 128, n) * 2).astype(np.uint8)
    data[at:] |= 1
    return Case("only-boundary-at-%d" % at, data)


def edge_fill_cases():
    rs = np.random.RandomState(77)
    yield only_boundary_case(8191)                                # a chunk's last position
    yield only_boundary_case(8192)                                # the next chunk's first
    yield only_boundary_case(16383, 16385)
    yield only_boundary_case(16384, 16385)
    n = 20011
    data = (rs.randint(0, 64, n) * 4 + 1).astype(np.uint8)        # level 0 all ones, level 1 (same order: nothing moved) all zeros
    c = Case("ones-zeros-mixed", data)
    assert c.zeros[0] == 0 and c.zeros[1] == n and all(0 < z < n for z in c.zeros[2:])
    yield c
    yield Case("ones-zeros-mixed/edges", data, edge_indices(n), c.planes())
    yield Case("long-runs/edges", runs_of(rs, 3 * ref.FG_CHUNK + 17, 20000, 4), edge_indices(3 * ref.FG_CHUNK + 17))


def level0_steps(n, changes, seed):
    """Bytes whose bit 0 starts at 0 and flips at every index of `changes`; the other bits are random."""
    rs = np.random.RandomState(seed)
    bit = np.zeros(n, dtype=np.uint8)
    for c in changes:
        bit[c:] ^= 1
    return ((rs.randint(0, 128, n) * 2).astype(np.uint8)) | bit


def refused_fill_cases():
    """Rank arrays the fill kernels must refuse: a bit change of level 0 that is not known between two that are (a mixed gap), in
    the first chunk, across a chunk edge and in the last word; a rank that decreases."""
    n = 20000
    for name, changes, drop in (("mixed-first-chunk", [100, 200, 300], 200), ("mixed-across-chunks", [8000, 8190, 8300], 8190),
                                ("mixed-last-word", [19970, 19980], 19980)):
        c = Case(name, level0_steps(n, changes, len(name)))
        assert c.R[0, drop] != ref.K_UNKNOWN
        c.R[0, drop] = ref.K_UNKNOWN
        yield c
    c = Case("decreasing", level0_steps(n, [100, 200, 300], 5))
    assert c.R[0, 200] == 100 and c.R[0, 300] == 100
    c.R[0, 300] = 99
    yield c
    c = Case("decreasing-level-5", level0_steps(n, [100, 200, 300], 6))
    known = np.flatnonzero(c.R[5] != ref.K_UNKNOWN)
    k = known[len(known) // 2]
    assert c.R[5, k] > 0
    c.R[5, k] = 0 if c.R[5, known[len(known) // 2 - 1]] > 0 else ref.K_UNKNOWN - 1
    yield c


BIG_N = 1024 * ref.FG_CHUNK + ref.FG_CHUNK + 5                  # 1026 chunks: fill_chunkscan_kernel's loop runs twice


def big_cases():
    """A few runs millions long (the last known boundary is carried over hundreds of chunks, and over the 1024th), and one
    boundary in the last chunk only, on every level."""
    n = BIG_N
    data = np.empty(n, dtype=np.uint8)
    at = 0
    for value, length in ((0x5A, 3_000_001), (0xA5, 2_500_000), (0x5B, 1_999_999), (0xFF, n)):
        data[at:at + length] = value
        at += length
    yield Case("big/runs", data)
    data = np.zeros(n, dtype=np.uint8)
    data[n - 3:] = 0xFF                                           # all ones: they stay last on every level
    c = Case("big/last-chunk-only", data)
    for p in range(8):
        assert list(np.flatnonzero(c.R[p] != ref.K_UNKNOWN)) == [0, n - 3, n] and (n - 3) // ref.FG_CHUNK == ref.fill_chunks(n) - 1
    yield c
