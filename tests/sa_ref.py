"""Host references for the suffix-array feature (not a test module): the suffix array by prefix doubling in numpy, its inverse,
the checker's verdict exactly as include/bce_hip.h defines it for bce_hip_sufcheck, the search of the libdivsufsort seam's
sa_search, and the defects the checker's tests plant."""
import numpy as np

OK, RANGE, MISSING, ORDER = 0, 1, 2, 3
NONE = (1 << 64) - 1
NAMES = {RANGE: "range", MISSING: "missing", ORDER: "order"}
BLOCK = 2048                                    # rows of one block of the checker's reductions
PASS = 256 * BLOCK                              # rows whose block results one pass of its top-level walk takes


def _bytes(t):
    return np.frombuffer(bytes(t), dtype=np.uint8) if not isinstance(t, np.ndarray) else np.ascontiguousarray(t, dtype=np.uint8)


def suffix_array(t):
    """The suffix array of t as int32: a suffix that is a prefix of another sorts before it."""
    a = _bytes(t)
    n = len(a)
    if n < 300:
        b = a.tobytes()
        return np.array(sorted(range(n), key=lambda i: b[i:]), dtype=np.int32)
    rank = a.astype(np.int64) + 1                # 0: behind the text's end
    mult = max(n, 256) + 2
    k = 1
    while True:
        second = np.zeros(n, dtype=np.int64)
        if k < n:
            second[:n - k] = rank[k:]
        key = rank * mult + second
        order = np.argsort(key, kind="stable")
        ks = key[order]
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.cumsum(np.concatenate(([1], (ks[1:] != ks[:-1]).astype(np.int64))))
        if rank.max() == n:
            return order.astype(np.int32)
        k *= 2


def inverse(sa):
    sa = np.asarray(sa).astype(np.int64)
    isa = np.empty(len(sa), dtype=np.int32)
    isa[sa] = np.arange(len(sa), dtype=np.int32)
    return isa


def _unsigned(sa):
    s = np.ascontiguousarray(sa)
    assert s.dtype.itemsize == 4 and s.dtype.kind in "iu"
    return s.view(np.uint32).astype(np.int64)


def check(t, sa):
    """(reason, index) of bce_hip_sufcheck for the words sa against the bytes t: the three stages in their order, the smallest index
    of the first stage that finds something; (OK, NONE) for a sound array."""
    a = _bytes(t)
    n = len(a)
    s = _unsigned(sa)
    assert len(s) == n and n >= 1
    bad = np.flatnonzero(s >= n)
    if len(bad):
        return RANGE, int(bad[0])
    inv = np.full(n + 1, -1, dtype=np.int64)      # (inv[n]: never compared)
    inv[s] = np.arange(n, dtype=np.int64)         # an entry that stands twice: one writer wins, and a hole is left elsewhere
    holes = np.flatnonzero(inv[:n] < 0)
    if len(holes):
        return MISSING, int(holes[0])
    x, y = s[:-1], s[1:]
    tx, ty = a[x], a[y]
    deeper = (y + 1 < n) & (inv[np.minimum(x + 1, n)] < inv[np.minimum(y + 1, n)])
    ok = (tx < ty) | ((tx == ty) & ((x + 1 == n) | deeper))
    bad = np.flatnonzero(~ok)
    if len(bad):
        return ORDER, int(bad[0]) + 1
    return OK, NONE


def verdict(t, sa):
    """check() as bce_amd.sufcheck reports it: None, or (name, index)."""
    reason, at = check(t, sa)
    return None if reason == OK else (NAMES[reason], at)


def search(t, sa, p):
    """(count, left): the rows of sa (a sorted run of suffixes of t, not necessarily all) whose suffix starts with all of p, and the
    first of them -- where there is none, the row in front of which they would stand."""
    t, p = bytes(t), bytes(p)
    m = len(p)
    if m == 0:
        return len(sa), 0
    heads = [t[int(s):int(s) + m] for s in sa]    # (a suffix shorter than p that is a prefix of p compares below p)
    return sum(1 for h in heads if h == p), sum(1 for h in heads if h < p)


def bwt_of(t, sa):
    """divbwt's answer read off a suffix array: (U, primary index)."""
    a = _bytes(t)
    s = np.asarray(sa).astype(np.int64)
    row0 = int(np.flatnonzero(s == 0)[0])
    rest = s[s != 0]
    return bytes([int(a[-1])]) + a[rest - 1].tobytes(), row0 + 1


def mutations(t, sa):
    """(name, array) for every defect the checker's tests plant into the sound array sa of t (uint32 copies), as far as the text's
    length and content give room for it."""
    a = _bytes(t)
    n = len(a)
    sound = np.ascontiguousarray(sa).view(np.uint32)
    isa = inverse(sound)
    rows = sorted({r for r in (0, n - 1, BLOCK - 1, BLOCK, PASS - 1, PASS) if 0 <= r < n})

    def planted(edit):
        m = sound.copy()
        edit(m)
        return m

    def put(r, v):
        return planted(lambda m: m.__setitem__(r, v))

    def swap(i, j):
        def edit(m):
            m[i], m[j] = m[j], m[i]
        return planted(edit)

    for r in rows:
        yield "entry n at row %d" % r, put(r, n)
        yield "entry with bit 31 at row %d" % r, put(r, 0x80000000 | int(sound[r]))
    yield "entry 0xFFFFFFFF at row %d" % (n // 2), put(n // 2, 0xFFFFFFFF)
    if n >= 2:
        yield "row 0 twice", put(1, int(sound[0]))
        yield "last row twice", put(0, int(sound[n - 1]))
        yield "a middle row twice", put(n // 2, int(sound[(n // 2 + 1) % n]))
        for r in sorted({1, n - 1, BLOCK, PASS, n // 2}):
            if 1 <= r < n:
                yield "rows %d and %d swapped" % (r - 1, r), swap(r - 1, r)
        same = np.flatnonzero(a[sound[:-1]] == a[sound[1:]])
        for r in same[[0, len(same) // 2, -1]] if len(same) else []:
            yield "rows %d and %d, which share a first byte, swapped" % (r, r + 1), swap(int(r), int(r) + 1)
        last = int(isa[n - 1])                     # the suffix of one byte: a prefix of its lower neighbour where that shares the byte
        if last + 1 < n:
            yield "suffix n - 1 swapped with the row below", swap(last, last + 1)
        if last >= 1:
            yield "suffix n - 1 swapped with the row above", swap(last - 1, last)
    if n >= 8:
        def two_stages(m):
            m[1], m[2] = m[2], m[1]
            m[n - 1] = n
        yield "order at row 2 and range at the last row", planted(two_stages)

        def two_rows(m):
            m[n - 2] = n + 7
            m[3] = 0xFFFFFFF0
        yield "range at rows 3 and n - 2", planted(two_rows)

        def hole_and_order(m):
            m[1], m[2] = m[2], m[1]
            m[n - 1] = m[n - 2]
        yield "order at row 2 and a missing position", planted(hole_and_order)
