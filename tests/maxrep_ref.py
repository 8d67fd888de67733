"""Host references for the maximal repeats (not a test module): the list of bce_hip_maximal_repeats from the capped LCP array of
repeat_ref and a stack over it, the same on arrays a test supplies (the hook bce_hip_maxrep_of_arrays_device), the brute force from
the definition, and the selection as the device runs it."""
from collections import Counter, defaultdict

import numpy as np

import repeat_ref

ORDERS = {"len": 0, "count": 1, "gain": 2}
BLOCK = 2048                                    # rows of one block of the trees, the prefix count and the selection
PASS = 256 * BLOCK                              # rows whose block results one pass of a one-workgroup kernel takes


def weight(order, length, count):
    """The 64-bit weight the list is ordered by (maxrep_step.h: mxr_weight)."""
    order = ORDERS.get(order, order)
    if order == 0:
        return (int(length) << 31) | int(count)
    if order == 1:
        return (int(count) << 13) | int(length)
    return int(length) * (int(count) - 1)


def rotation_order(text):
    """The rows of the sorted rotations of the circular text (rotations that are equal in the order of their positions), by prefix
    doubling on cyclic ranks."""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(a)
    rank = a.astype(np.int64)
    k = 1
    while True:
        key = rank * (max(n, 256) + 1) + np.roll(rank, -k)
        order = np.argsort(key, kind="stable")
        ks = key[order]
        new = np.empty(n, dtype=np.int64)
        new[order] = np.cumsum(np.concatenate(([0], (ks[1:] != ks[:-1]).astype(np.int64))))
        rank = new
        if rank.max() == n - 1 or k >= n:
            return order.astype(np.int64)
        k *= 2


def lcp_of_order(text, sa, L):
    """The capped LCP array of the rows sa (repeat_ref.capped_lcp's array, which no order of tied rows changes) without the n x L
    windows: all neighbouring pairs are compared byte by byte, and a pair leaves at its first difference."""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(a)
    sa = np.asarray(sa, dtype=np.int64)
    out = np.zeros(n, dtype=np.uint32)
    rows = np.arange(1, n)
    x, y = sa[:-1].copy(), sa[1:].copy()
    for j in range(L):
        if not len(rows):
            break
        same = a[(x + j) % n] == a[(y + j) % n]
        out[rows[~same]] = j
        rows, x, y = rows[same], x[same], y[same]
    out[rows] = L
    return out


def bwt_of(text, sa):
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    return a[(np.asarray(sa, dtype=np.int64) - 1) % len(a)]


def bwt_runs(bw):
    bw = np.asarray(bw)
    return 1 + int(np.count_nonzero(bw[1:] != bw[:-1]))


def intervals(lcp, bw):
    """Every left-maximal LCP interval of the words lcp (lcp[0] == 0) once, as (len, count, first row, representative row), in the
    order of the representatives: two passes with a stack of (value, row), values ascending from the bottom."""
    lcp = [int(v) for v in np.asarray(lcp)]
    n = len(lcp)
    bw = np.asarray(bw)
    D = np.concatenate(([0], np.cumsum(bw[1:] != bw[:-1]))).tolist() if n else []
    nxt = [n] * n                                # the nearest row below with a smaller value
    stack = []
    for r in range(n - 1, -1, -1):
        while stack and lcp[stack[-1]] >= lcp[r]:
            stack.pop()
        nxt[r] = stack[-1] if stack else n
        stack.append(r)
    out = []
    stack = [0] if n else []                     # rows whose values ascend; of equal values the lowest row stays
    for r in range(1, n):
        l = lcp[r]
        while lcp[stack[-1]] > l:
            stack.pop()
        top = stack[-1]
        if lcp[top] == l:                        # a row above carries l inside the same interval (or l == 0 == lcp[0])
            stack[-1] = r
            continue
        stack.append(r)
        p, q = top, nxt[r]
        if l >= 1 and l != 0xFFFFFFFF and D[q - 1] - D[p] > 0:
            out.append((l, q - p, p, r))
    return out


def of_arrays(lcp, sa, bw, min_len, max_len, order, limit):
    """What bce_hip_maxrep_of_arrays_device returns: (entries as (len, count, row, pos) tuples, info)."""
    n = len(lcp)
    found = [x for x in intervals(lcp, bw) if x[0] >= min_len]
    found.sort(key=lambda x: (-weight(order, x[0], x[1]), x[3]))
    info = {"total": len(found), "capped": sum(1 for x in found if x[0] == max_len), "bwt_runs": bwt_runs(bw) if n else 0,
            "found": min(limit, len(found))}
    sa = np.asarray(sa)
    return [(l, c, p, int(sa[p])) for l, c, p, _ in found[:limit]], info


def of_text(text, min_len, max_len, order, limit):
    """What bce_hip_maximal_repeats returns for the text, but for pos: (entries as (len, count, row) tuples, info)."""
    sa = rotation_order(text)
    lcp = repeat_ref.capped_lcp(text, max_len) if len(text) * max_len <= 1 << 22 else lcp_of_order(text, sa, max_len)
    ents, info = of_arrays(lcp, sa, bwt_of(text, sa), min_len, max_len, order, limit)
    return [e[:3] for e in ents], info


def brute_force(text, min_len, max_len):
    """The set of (len, count, row, bytes) from the definition: a Counter over all cyclic l-grams for every l, the bytes in front of
    and behind the occurrences, row = the rotations whose first l bytes are smaller."""
    text = bytes(text)
    n = len(text)
    out = set()
    for l in range(max(1, min_len), max_len + 1):
        grams = [bytes(text[(i + j) % n] for j in range(l)) for i in range(n)]
        occ = Counter(grams)
        left, right = defaultdict(set), defaultdict(set)
        for i, g in enumerate(grams):
            left[g].add(text[(i - 1) % n])
            right[g].add(text[(i + l) % n])
        for g, c in occ.items():
            if c < 2 or len(left[g]) < 2 or (l < max_len and len(right[g]) < 2):
                continue
            out.add((l, c, sum(1 for h in grams if h < g), g))
    return out


def select(weights, limit):
    """The selection as the device runs it on the weights of the repeats in row order (maxrep_step.h): 64 bins of floor(log2), the
    largest bin t with `want` weights at or above it, the candidates in row order, a stable sort by weight descending -> (t,
    candidates, the indices of the first min(limit, len) in list order)."""
    H = [0] * 64
    for w in weights:
        H[int(w).bit_length() - 1] += 1
    want = min(limit, len(weights))
    above, t = 0, 0
    for b in range(63, -1, -1):
        above += H[b]
        if above >= want:
            t = b
            break
    cand = [i for i, w in enumerate(weights) if w >> t]
    assert len(cand) == above
    cand.sort(key=lambda i: -weights[i])         # (stable)
    return t, above, cand[:want]
