"""CPU: the early rounds of the enumeration do not need the finished rotation order.

K1's first sort orders the rotations by their first h bytes.  A BWT gathered from that order (`bwt'`) differs from the true
one only inside groups of rows that share their first h bytes.  The claim under test: every round r <= r_cap(h) = 8h - 1 of
the enumeration -- its node triples, its symbol records and therefore the range-coder operations of every plane up to the
end of that round -- and the planes' zero counts are the same on `bwt'` as on the true BWT.  The argument is in DESIGN.md;
this file is what decides.  It also reports the first round at which the two traces really differ (`FIRST_DIFF`, printed
with -s), so the margin is visible: the argument says round 8h + 1 at the earliest (the triples of round 8h are still
children of round 8h - 1).
"""
import numpy as np
import pytest

import oracle


def r_cap(h):
    """Last round whose nodes read ranks only at boundaries of classes of rows sharing <= h leading bytes."""
    return 8 * h - 1


def partial_bwt(data, h):
    """BWT from the rotations sorted by their first h bytes only (cyclic), ties by position."""
    t = np.frombuffer(data, dtype=np.uint8)
    n = len(t)
    pos = np.arange(n, dtype=np.int64)
    keys = []
    for lo in range(0, h, 8):                       # eight bytes per 64-bit key word, most significant word first
        k = np.zeros(n, dtype=np.uint64)
        for j in range(lo, min(lo + 8, h)):
            k = (k << np.uint64(8)) | t[(pos + j) % n].astype(np.uint64)
        keys.append(k)
    sa = np.lexsort(tuple(reversed(keys)))          # stable: equal keys stay in position order
    return t[(sa - 1) % n].copy()


def _rank1_tables(bwt):
    bits = oracle.plane_bits(bwt)                   # [8, n] in each plane's own order
    r1 = np.zeros((8, bits.shape[1] + 1), dtype=np.int64)
    np.cumsum(bits, axis=1, out=r1[:, 1:])
    return r1


def _symbol_rounds(tr, r1):
    """Round of every symbol record of the trace: which nodes code a symbol follows from the node rule and the ranks."""
    nd = tr["nodes"].astype(np.int64)
    rnd, pl, s, x0, x1 = nd.T
    x = x0 + x1
    n1 = r1[pl, s + x] - r1[pl, s]                  # ones among the node's rows
    n0 = x - n1
    mn = np.maximum(x0 - n1, 0)
    mx = x0 - np.maximum(n1 - x1, 0)
    emits = (n1 > 0) & (n0 > 0) & (mx != mn)
    assert int(emits.sum()) == len(tr["syms"])
    assert np.array_equal(pl[emits], tr["syms"][:, 0])
    assert np.array_equal((mx - mn + 1)[emits], tr["syms"][:, 2])
    return rnd[emits]


def _ops_per_symbol(syms):
    """Range-coder operations of one symbol record: one, plus one per halving of a k > 31 escape."""
    s = syms[:, 1].astype(np.int64)
    k = syms[:, 2].astype(np.int64)
    ops = np.ones(len(k), dtype=np.int64)
    while True:
        big = k > 31
        if not big.any():
            return ops
        ops += big
        k = np.where(big, (k + (~s & 1)) >> 1, k)
        s = np.where(big, s >> 1, s)


_TRUE = {}
FIRST_DIFF = {}


def _true_trace(name, data):
    if name not in _TRUE:
        bwt, off = oracle.bwt_stage(data)
        tr = oracle.trace_encode_from_bwt(bwt, off)
        sym_round = _symbol_rounds(tr, _rank1_tables(bwt))
        _TRUE[name] = (bwt, off, tr, sym_round, _ops_per_symbol(tr["syms"]))
    return _TRUE[name]


def _first_difference(a, b):
    """Round of the first node at which two traces differ, None if they are the same."""
    m = min(len(a), len(b))
    ne = np.flatnonzero((a[:m] != b[:m]).any(axis=1))
    if len(ne):
        return int(min(a[ne[0], 0], b[ne[0], 0]))
    if len(a) != len(b):
        return int((a if len(a) > m else b)[m, 0])
    return None


def _inputs():
    k64, m1 = 64 << 10, 1 << 20
    yield "text-64K", lambda: oracle.synth_text(11, k64), (4, 8, 12)
    yield "text-1M", lambda: oracle.synth_text(12, m1), (4, 8, 12)
    yield "rand-64K", lambda: oracle.synth_rand(13, k64), (2, 3, 4)
    yield "ab", lambda: b"ab" * 4096, (1, 2, 8, 12)
    yield "abcabd", lambda: b"abcabd" * 1500 + b"x", (1, 3, 6, 8, 12)
    yield "one-byte", lambda: b"q" * 5000, (1, 8, 12)
    yield "300B", lambda: bytes((i * 37 + (i >> 3)) & 0xFF for i in range(300)), (1, 2, 8)
    yield "300B-text", lambda: oracle.synth_text(14, 300), (1, 2, 8, 12)
    yield "shorter-than-h", lambda: b"banana", (8, 12)
    yield "shorter-than-h-5", lambda: b"abcab", (8, 12)


CASES = [(name, make, h) for name, make, hs in _inputs() for h in hs]


@pytest.mark.parametrize("name,make,h", CASES, ids=["%s-h%d" % (c[0], c[2]) for c in CASES])
def test_early_rounds_do_not_need_the_finished_order(name, make, h):
    data = make()
    bwt, off, tr, sym_round, sym_ops = _true_trace(name, data)
    bwt_p = partial_bwt(data, h)
    assert np.array_equal(np.sort(bwt_p), np.sort(bwt))
    tp = oracle.trace_encode_from_bwt(bwt_p, off)
    cap = r_cap(h)

    first = _first_difference(tr["nodes"], tp["nodes"])
    FIRST_DIFF[(name, h)] = first
    print("%s h=%d: r_cap %d, rounds %d, traces first differ in round %s" % (name, h, cap, tr["rounds"], first))

    # the planes' zero counts
    assert tp["C"] == tr["C"]

    # node triples of every round <= r_cap, in order (the trace is round-major)
    na = tr["nodes"][: np.searchsorted(tr["nodes"][:, 0], cap, side="right")]
    nb = tp["nodes"][: np.searchsorted(tp["nodes"][:, 0], cap, side="right")]
    assert na.shape == nb.shape and np.array_equal(na, nb)
    assert first is None or first > cap

    # symbol records of those rounds, and with them every plane's coder operations up to the end of round r_cap
    sr_p = _symbol_rounds(tp, _rank1_tables(bwt_p))
    ops_p = _ops_per_symbol(tp["syms"])
    ka, kb = np.searchsorted(sym_round, cap, side="right"), np.searchsorted(sr_p, cap, side="right")
    assert ka == kb and np.array_equal(tr["syms"][:ka], tp["syms"][:kb])
    for plane in range(8):
        oa = tr["ops"][tr["ops"][:, 0] == plane]
        ob = tp["ops"][tp["ops"][:, 0] == plane]
        late_a = sym_ops[(tr["syms"][:, 0] == plane) & (sym_round > cap)].sum()
        late_b = ops_p[(tp["syms"][:, 0] == plane) & (sr_p > cap)].sum()
        ca, cb = len(oa) - late_a, len(ob) - late_b
        assert ca == cb and ca > 0
        assert np.array_equal(oa[:ca], ob[:cb])


def test_full_depth_order_is_the_bwt():
    """h >= n sorts the rotations completely (tied rotations have equal preceding bytes): the provisional BWT is the BWT."""
    for data in (b"banana", b"abcab", b"ab" * 7, oracle.synth_text(15, 300)):
        bwt, _ = oracle.bwt_stage(data)
        assert np.array_equal(partial_bwt(data, len(data)), bwt)


def test_the_cap_is_tight_somewhere():
    """One byte deeper than h is really needed right behind the cap: on random bytes the traces differ in round 8h + 1, the first
    whose node triples come from ranks that the order sorted to depth h no longer gives."""
    data = oracle.synth_rand(13, 64 << 10)
    bwt, off, tr, _, _ = _true_trace("rand-64K", data)
    for h in (1, 2):
        tp = oracle.trace_encode_from_bwt(partial_bwt(data, h), off)
        assert _first_difference(tr["nodes"], tp["nodes"]) == r_cap(h) + 2
