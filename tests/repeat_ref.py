"""References for the LCP array of the sorted rotations and what is reduced from it (tests/test_repeat_cpu.py,
tests/test_gpu_repeat.py): numpy / pure Python on the text itself, nothing of the index."""
import math
from collections import Counter

import numpy as np

NONE = 0xFFFFFFFF


def _windows(text, L):
    """The n windows of L cyclic bytes, window i = text[(i + j) mod n], j < L: a sliding-window view of the extended text, (n, L)."""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(a)
    ext = np.tile(a, (L - 1) // n + 2)[:n + L - 1]
    return np.lib.stride_tricks.sliding_window_view(ext, L)


def capped_lcp(text, L):
    """lcp[0] = 0, lcp[r] = min(L, the common prefix of the rotations in rows r - 1 and r of the sorted rotations), no cap at n.
    The n windows of L cyclic bytes are sorted as byte strings (a void view), neighbours are compared: rotations that differ within
    L bytes stand in the order of the full sort, and those tied to L bytes carry L whatever their order, so the capped array is a
    function of the text alone."""
    n = len(text)
    assert n >= 1 and L >= 1
    w = np.ascontiguousarray(_windows(text, L))
    order = np.argsort(w.view(np.dtype((np.void, L))).ravel(), kind="stable")
    s = w[order]
    out = np.zeros(n, dtype=np.uint32)
    if n > 1:
        ne = s[1:] != s[:-1]
        out[1:] = np.where(ne.any(axis=1), ne.argmax(axis=1), L)
    return out


def classes_of_lcp(lcp, k):
    """The sorted sizes of the maximal runs of rows [s, e) with lcp[r] >= k for s < r < e."""
    lcp = np.asarray(lcp, dtype=np.int64)
    starts = np.flatnonzero(np.concatenate([[True], lcp[1:] < k]))
    return sorted(np.diff(np.concatenate([starts, [len(lcp)]])).tolist())


def kgram_classes(text, k):
    """The sorted occurrence counts of the distinct cyclic k-grams, counted as byte strings: independent of any sort of rotations."""
    text = bytes(text)
    n = len(text)
    if k == 0:
        return [n]
    if n * k <= 1 << 22:
        ext = text * (k // n + 2)
        return sorted(Counter(ext[i:i + k] for i in range(n)).values())
    w = np.ascontiguousarray(_windows(text, k))
    _, counts = np.unique(w.view(np.dtype((np.void, k))).ravel(), return_counts=True)
    return sorted(counts.tolist())


def kgram_record(text, k, log2q):
    """(distinct, once, nlogn_q24, max_count) of the cyclic k-grams; log2q(c) = the library's Q24 integer log2 of c."""
    sizes = kgram_classes(text, k)
    cnt = Counter(sizes)
    return len(sizes), cnt.get(1, 0), sum(m * c * log2q(c) for c, m in cnt.items()), sizes[-1]


def entropy_q24(n, s_k, s_k1):
    """H_k from the integer sums, the expression the library's callers and the CLI use."""
    return max(0, s_k - s_k1) / (n * 16777216.0)


def entropy_float(text, k):
    """The order-k empirical entropy of the circular text from the definition, in floats:
    H_k = (1 / n) * sum over k-grams w, bytes c of N(wc) * log2(N(w) / N(wc))."""
    n = len(text)
    f = lambda sizes: math.fsum(c * math.log2(c) for c in sizes)
    return max(0.0, (f(kgram_classes(text, k)) - f(kgram_classes(text, k + 1))) / n)


def rot_lcp(text, a, b, L):
    """The common prefix of rotations a and b, at most L, byte by byte."""
    n = len(text)
    l = 0
    while l < L and text[(a + l) % n] == text[(b + l) % n]:
        l += 1
    return l


def lcp_of_order(text, sa, L):
    return np.array([0] + [rot_lcp(text, sa[r - 1], sa[r], L) for r in range(1, len(sa))], dtype=np.uint32)
