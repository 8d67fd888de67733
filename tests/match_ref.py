"""Brute-force references for the matching statistics of a query against a text (tests/test_match_cpu.py, tests/test_gpu_match.py):
pure Python / numpy on the text itself, nothing of the index."""
import numpy as np

NONE = 0xFFFFFFFF


def match_lens(text, query, max_len, cyclic=False):
    """len[i] = the largest l <= min(max_len, i + 1) such that query[i - l + 1 .. i] occurs in the text -- the circular text with
    cyclic (searched in text * k, as locate_ref.cyclic_hits does, at starts below n), else the text as it lies.  Every test is one
    bytes.find.  The strings that end at i are suffixes of one another, so "occurs" is monotone in l: bisected, not walked."""
    text, query = bytes(text), bytes(query)
    n = len(text)
    ext = text * ((min(max_len, len(query)) + n - 1) // n + 1) if cyclic else text
    out = np.zeros(len(query), dtype=np.uint32)
    for i in range(len(query)):
        lo, hi = 0, min(max_len, i + 1)                               # the match of lo bytes occurs; none longer than hi does
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if 0 <= ext.find(query[i - mid + 1:i + 1]) < n:
                lo = mid
            else:
                hi = mid - 1
        out[i] = lo
    return out


def check_positions(text, query, lens, pos, cyclic):
    """Every pos[i] is valid: 0xFFFFFFFF exactly where len[i] == 0, else a start below n at which the match of len[i] bytes stands
    -- around the end of the text too with cyclic, else with pos[i] + len[i] <= n."""
    text, query = bytes(text), bytes(query)
    n = len(text)
    assert len(lens) == len(pos) == len(query)
    ext = text * (int(max(lens.tolist() + [0])) // n + 2) if cyclic else text
    for i, (l, p) in enumerate(zip(lens.tolist(), pos.tolist())):
        if l == 0:
            assert p == NONE, (i, p)
        else:
            assert p < n and (cyclic or p + l <= n) and ext[p:p + l] == query[i - l + 1:i + 1], (i, l, p)


def covered(lens, min_len):
    """The j for which some i >= j has lens[i] >= min_len and i - lens[i] + 1 <= j: from the definition, a difference array over
    the matches' extents."""
    lens = np.asarray(lens, dtype=np.int64)
    q = len(lens)
    mark = np.zeros(q + 1, dtype=np.int64)
    ends = np.flatnonzero(lens >= min_len)
    np.add.at(mark, ends - lens[ends] + 1, 1)
    np.add.at(mark, ends + 1, -1)
    return int(np.count_nonzero(np.cumsum(mark[:q]) > 0))


def coverage(text, query, min_len, cyclic=False):
    return covered(match_lens(text, query, min_len, cyclic), min_len)
