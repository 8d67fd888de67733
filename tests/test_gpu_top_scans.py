"""GPU: the selection behind bce_hip_top_kgrams alone, through the hook bce_hip_top_classes_of_lcp_device, on synthetic LCP arrays
that put classes and ties across any block (B = 2048 rows) and any pass (P = 256 blocks) of the carried scans: the class-start
carry, the histogram, the candidates' offsets and the stable sort, with the launches and geometry of the real call.  Against the
numpy reference tests/top_ref.py: top_of_lcp, which tests/test_top_cpu.py checks against the counted k-grams."""
import ctypes as C

import numpy as np
import pytest
import torch

from bce_amd import api

import top_ref as ref

pytestmark = pytest.mark.gpu
E_ARG = -1
B = 2048                                       # rows of a scan block
P = 256 * B                                    # rows of one pass of a carried scan: 524 288
GRID = (1, 2047, 2048, 2049, 4097, P - 1, P, P + 1, P + 2049, 2 * P + 1)
GUARD = -0x21524111                            # 0xDEADBEEF as an int32
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


def _guarded(words):
    """The words as int32 at element 1 of a device tensor -- 4-byte aligned and no more -- with guard words around them."""
    buf = torch.full((len(words) + 4,), GUARD, dtype=torch.int32, device=DEV)
    buf[1:1 + len(words)] = torch.from_numpy(np.asarray(words).astype(np.uint32).view(np.int32)).to(DEV)
    return buf, buf[1:1 + len(words)]


def _untouched(buf, words):
    got = buf.cpu().numpy()
    return got[0] == GUARD and (got[1 + len(words):] == GUARD).all() and np.array_equal(got[1:1 + len(words)].view(np.uint32), words)


def _from_sizes(sizes, n, k=9):
    """The LCP array of n rows whose classes for k have these sizes, in row order, as far as they fit; singletons behind them."""
    a = np.full(n, k, dtype=np.uint32)
    total = int(np.sum(sizes))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    a[starts[starts < n]] = 0
    if total < n:
        a[total:] = 0
    return a


def _lcp_arrays(n):
    """(name, LCP array of n words with word 0 == 0, the k values to ask with)."""
    rs = np.random.RandomState(n)
    small = rs.randint(0, 6, n).astype(np.uint32)
    small[0] = 0
    out = [("small values: very many small classes, ties everywhere", small, (1, 3, 5))]
    out.append(("all singletons: every class a candidate, nothing to sort", np.zeros(n, dtype=np.uint32), (1, 9)))
    a = np.full(n, 4096, dtype=np.uint32)
    a[0] = 0
    out.append(("one class over everything", a, (0, 9, 4096)))
    if n > 2001:
        a = small.copy()
        a[1001:n - 1000 + 1] = 9                                         # rows 1000 .. n - 1000: across every block and pass edge there is
        out.append(("a large class from row 1000 to row n - 1000", a, (9, 3)))
        a = small.copy()
        a[1001:] = 9
        out.append(("a large class from row 1000 to the last row", a, (9,)))
    if n > B:
        # equal sizes on both sides of every block edge (and so of every pass edge): runs of 300, then of 7, cut so that one class
        # ends on the edge's last row, the next starts on its first; the ties must come out in row order
        for size in (300, 7):
            per = B // size
            sizes = np.tile(np.concatenate([np.full(per, size), [B - per * size]]), n // B + 1)
            sizes = sizes[sizes > 0]
            out.append(("classes of %d up to every block edge, a rest class before it" % size, _from_sizes(sizes, n), (9,)))
        sizes = np.tile([300, 300, 5, 300, 1, 2, 300, 300, 300, 1000], n // 2808 + 1)   # (a period of 2808 rows) classes of 300 and 1000 that straddle the edges
        out.append(("equal classes straddling block and pass edges", _from_sizes(sizes, n), (9,)))
    if n >= 2047:
        sizes = rs.randint(4, 8, n // 4 + 1)                              # every class in the bin [4, 8): every class a candidate, two key bits
        out.append(("a candidate set in one bin", _from_sizes(sizes, n), (9,)))
        sizes = np.where(rs.randint(0, 50, n // 3 + 1) == 0, rs.randint(64, 128, n // 3 + 1), rs.randint(1, 4, n // 3 + 1))
        out.append(("few classes of 64 .. 127 among very many of 1 .. 3", _from_sizes(sizes, n), (9,)))
    return out


def _select_and_check(ctx, name, lcp, k, limits):
    n = len(lcp)
    sa = np.random.RandomState(n + 1).permutation(n).astype(np.uint32)      # a position names its row
    lbuf, d_lcp = _guarded(lcp)
    sbuf, d_sa = _guarded(sa)
    torch.cuda.synchronize()
    counts, rows, distinct, hist = ref.top_of_lcp(lcp, k, 1 << 30)          # the whole order, once: every limit's answer is its prefix
    for limit in limits:
        got, d, h = api.top_classes_of_lcp_device(d_lcp.data_ptr(), n, d_sa.data_ptr(), k, limit, ctx)
        want = min(limit, distinct)
        assert (d, h, len(got)) == (distinct, hist, want), (name, n, k, limit, d, len(got))
        ok = np.array_equal(got["count"], counts[:want]) and np.array_equal(got["row"], rows[:want])
        if not ok:
            e = int(np.flatnonzero((got["count"] != counts[:want]) | (got["row"] != rows[:want]))[0])
            raise AssertionError((name, n, k, limit, e, got[e], int(counts[e]), int(rows[e])))
        assert np.array_equal(got["pos"], sa[rows[:want]]), (name, n, k, limit)
    assert _untouched(lbuf, lcp) and _untouched(sbuf, sa), (name, n)


@pytest.mark.parametrize("n", GRID)
def test_the_selection_on_synthetic_lcp_arrays(ctx, n):
    for name, lcp, ks in _lcp_arrays(n):
        for k in ks:
            distinct = len(ref.classes_of_lcp(lcp, k)[0])
            limits = sorted(set(v for v in (1, 2, 1000, distinct - 1, distinct, distinct + 1) if 1 <= v <= api.TOP_MAX))
            _select_and_check(ctx, name, lcp, k, limits)


def test_the_arrays_hold_what_their_names_say():
    n = P + 2049
    arrays = {name.split(":")[0]: (lcp, ks) for name, lcp, ks in _lcp_arrays(n)}
    starts, sizes = ref.classes_of_lcp(arrays["classes of 300 up to every block edge, a rest class before it"][0], 9)
    assert set(sizes.tolist()) >= {300, B - 6 * 300} and np.isin(np.arange(B, n, B), starts).all()   # a class starts on every block's first row
    starts, sizes = ref.classes_of_lcp(arrays["equal classes straddling block and pass edges"][0], 9)
    ends = starts + sizes
    assert ((starts < P) & (ends > P)).any()                                 # a class lies across the pass edge
    assert ((sizes == 300) & (starts // B != (ends - 1) // B)).sum() > 10    # classes of 300 across block edges, and many more inside blocks
    starts, sizes = ref.classes_of_lcp(arrays["a candidate set in one bin"][0], 9)
    assert sizes[:-1].min() >= 4 and sizes.max() <= 7
    starts, sizes = ref.classes_of_lcp(arrays["a large class from row 1000 to row n - 1000"][0], 9)
    assert sizes.max() == n - 1999 and starts[sizes.argmax()] == 1000
    assert [v.tolist() for v in ref.top_of_lcp(np.zeros(5, dtype=np.uint32), 1, 3)[:2]] == [[1, 1, 1], [0, 1, 2]]


def test_the_hook_refuses_bad_arguments_before_any_device_call(ctx):
    words = torch.zeros(8, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    lib, p = ctx.lib, words.data_ptr()
    out = np.full(4, 7, dtype=api.TOP_DTYPE)
    found, distinct, hist = C.c_uint32(5), C.c_uint64(6), (C.c_uint64 * 32)(*([7] * 32))
    tail = (C.byref(found), C.byref(distinct), C.addressof(hist))
    for args in ((None, 8, p, 1, 4, out.ctypes.data) + tail, (p, 8, None, 1, 4, out.ctypes.data) + tail, (p, 0, p, 1, 4, out.ctypes.data) + tail,
                 (p, 1 << 31, p, 1, 4, out.ctypes.data) + tail, (p, 8, p, 4097, 4, out.ctypes.data) + tail, (p, 8, p, 1, 0, out.ctypes.data) + tail,
                 (p, 8, p, 1, (1 << 20) + 1, out.ctypes.data) + tail, (p, 8, p, 1, 4, None) + tail,
                 (p, 8, p, 1, 4, out.ctypes.data, None, C.byref(distinct), C.addressof(hist))):
        assert lib.bce_hip_top_classes_of_lcp_device(ctx.h, *args) == E_ARG, args
    assert (out["count"] == 7).all() and (found.value, distinct.value, list(hist)) == (5, 6, [7] * 32)
    got, d, h = api.top_classes_of_lcp_device(p, 8, p, 1, 4, ctx)           # eight singletons: the four lowest rows
    assert got["row"].tolist() == [0, 1, 2, 3] and got["count"].tolist() == [1] * 4 and d == 8 and h == [8] + [0] * 31
