"""The definition of the search within k edits (tests/test_edit_cpu.py, tests/test_gpu_edit.py, tests/test_gpu_cli_edit.py) in numpy
on the text itself, nothing of the index.

T: the text, n bytes, read circularly; P: a pattern of m bytes; 0 <= k <= 2.  For a string S of l bytes the ANCHORED edit distance
e(P, S) is the least number of substitutions, insertions and deletions that turn P into S among the alignments that put P's first
byte against S's first and P's last against S's last, each a match or a substitution:
    m == 0: e = 0 for l == 0, else infinite;  m == 1: e = [P[0] != S[0]] for l == 1, else infinite;
    m >= 2: infinite for l < 2, else [P[0] != S[0]] + Lev(P[1 .. m-1), S[1 .. l-1)) + [P[m-1] != S[l-1]].
S(i, l) = T[(i + j) mod n], j < l, for l in [max(0, m - k), m + k].  Cyclic: E(i) = min over l of e(P, S(i, l)), i is a hit when
E(i) <= k, at distance E(i) and length L(i) = the smallest l that attains it.  Linear: the same over the l with i + l <= n only.

table() is a banded DP (band 2 k + 1 around the diagonal) over all positions at once; everything else is read from it."""
import numpy as np

from count_ref import cyclic_cut  # noqa: F401
import near_ref

MAX_K = 2
BIG = 99


def table(text, pat):
    """E[i, j] = min(e(P, S(i, m - MAX_K + j)), BIG) for j in [0, 2 MAX_K]: exact wherever it is <= MAX_K (a distance <= MAX_K never
    leaves the band), BIG or more than MAX_K elsewhere, BIG for lengths that do not exist.  uint8, n rows."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    p = np.frombuffer(bytes(pat), dtype=np.uint8)
    n, m, k = len(t), len(p), MAX_K
    E = np.full((n, 2 * k + 1), BIG, dtype=np.uint8)
    ext = np.resize(t, n + m + k + 1)                                  # ext[i] = T[i mod n]

    def col(j):                                                        # T[(i + j) mod n] for every i
        return ext[j:j + n]

    if m == 0:
        E[:, k] = 0
        return E
    if m == 1:
        E[:, k] = col(0) != p[0]
        return E
    first = (col(0) != p[0]).astype(np.uint8)
    one = np.uint8(1)
    mi = m - 2                                                         # the inner pattern P[1 .. m-1)
    # cur[off][i] = Lev(P[1 .. 1 + a), T[i + 1 .. i + 1 + b)), b = a + off, capped at BIG
    cur = {off: np.full(n, off, dtype=np.uint8) for off in range(0, k + 1)}
    for a in range(1, mi + 1):
        new = {}
        for off in range(-k, k + 1):
            b = a + off
            if b < 0:
                continue
            if b == 0:
                new[off] = np.full(n, min(a, BIG), dtype=np.uint8)
                continue
            x = np.full(n, BIG, dtype=np.uint8)
            if off in cur:
                np.add(cur[off], col(b) != p[a], out=x)                # inner byte b - 1 of the text is T[i + 1 + b - 1]
            if off + 1 in cur:
                np.minimum(x, cur[off + 1] + one, out=x)
            if off - 1 in new:
                np.minimum(x, new[off - 1] + one, out=x)
            new[off] = np.minimum(x, BIG, out=x)
        cur = new
    for j in range(2 * k + 1):
        l = m - k + j
        if l >= 2 and (j - k) in cur:
            E[:, j] = np.minimum(first + cur[j - k] + (col(l - 1) != p[m - 1]), BIG)
    return E


def hits_of(E, m, n, k, cyclic=True):
    """(positions uint32 ascending, lens uint16, dists uint8) from table()'s E."""
    K = MAX_K
    key = np.full(n, 255, dtype=np.uint8)                               # 8 * distance + j of the best length so far
    at = np.arange(n, dtype=np.int64)
    for j in range(K - k, K + k + 1):
        l = m - K + j
        if l < 0:
            continue
        ok = E[:, j] <= k
        if not cyclic:
            ok &= at <= n - l
        np.minimum(key, np.where(ok, (E[:, j] & 3) * np.uint8(8) + np.uint8(j), np.uint8(255)), out=key)
    pos = np.flatnonzero(key < 255)
    return pos.astype(np.uint32), (m - K + (key[pos] & 7).astype(np.int64)).astype(np.uint16), (key[pos] >> 3).astype(np.uint8)


def hits(text, pat, k, cyclic=True):
    return hits_of(table(text, pat), len(pat), len(text), k, cyclic)


def counts_of(dists, k):
    return np.bincount(dists, minlength=k + 1)[:k + 1].astype(np.uint64)


def counts(text, pat, k, cyclic=True):
    """The hits at distance exactly 0 .. k: a uint64 array of k + 1."""
    return counts_of(hits(text, pat, k, cyclic)[2], k)


def candidate_lengths(E, k):
    """per position: at how many lengths it is within k edits (what the search finds as candidates, at the least)"""
    return (E[:, MAX_K - k:MAX_K + k + 1] <= k).sum(axis=1)


# ---- the definition in plain loops (tests/test_edit_cpu.py checks table() against it on tiny texts) ---------------------------------

def _lev(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def anchored(p, s):
    m, l = len(p), len(s)
    if m == 0:
        return 0 if l == 0 else None
    if m == 1:
        return int(p[0] != s[0]) if l == 1 else None
    if l < 2:
        return None
    return int(p[0] != s[0]) + _lev(p[1:m - 1], s[1:l - 1]) + int(p[m - 1] != s[l - 1])


def hits_by_loops(text, pat, k, cyclic=True):
    n, m = len(text), len(pat)
    out = []
    for i in range(n):
        best = None
        for l in range(max(0, m - k), m + k + 1):
            if not cyclic and i + l > n:
                continue
            e = anchored(pat, bytes(text[(i + j) % n] for j in range(l)))
            if e is not None and e <= k and (best is None or e < best[2]):
                best = (i, l, e)
        if best:
            out.append(best)
    return out


# ---- the cases of the CPU and GPU tests --------------------------------------------------------------------------------------------

def edited(pat, text):
    """`pat` with one and two bytes deleted, inserted (a byte of the text's alphabet, and one it lacks) and substituted: at the
    second byte, in the middle, at the second-to-last byte, and adjacent."""
    m = len(pat)
    if m < 3:
        return []
    have = sorted(set(bytes(text)))
    lacks = next(v for v in range(255, -1, -1) if v not in have) if len(have) < 256 else have[0]
    spots = sorted({1, m // 2, m - 2})
    out = []
    for at in spots:
        for v in (have[(have.index(pat[at]) + 1) % len(have)] if pat[at] in have else have[0], lacks):
            out.append(pat[:at] + bytes([v]) + pat[at:])               # one inserted
            out.append(pat[:at] + bytes([v]) + pat[at + 1:])           # one substituted
            out.append(pat[:at] + bytes([v, v]) + pat[at:])            # two inserted, adjacent
        out.append(pat[:at] + pat[at + 1:])                            # one deleted
        if m >= 5:
            out.append(pat[:at] + pat[at + 2:] if at + 2 <= m - 1 else pat[:at - 1] + pat[at + 1:])   # two deleted, adjacent
    if m >= 6:
        out.append(pat[:1] + pat[2:m - 2] + pat[m - 1:])               # two deleted, apart
        out.append(pat[:1] + bytes([have[0]]) + pat[1:m - 2] + pat[m - 1:])   # one in, one out
    return out


def patterns_for(text):
    """near_ref.patterns_for's cuts and alterations, and edited() of the cuts of 3, 5, 8 and n (<= 12) bytes at 0 and across the end."""
    base = near_ref.patterns_for(text)
    n = len(text)
    more = []
    for m in sorted({3, 5, 8, n} - {0, 1, 2}):
        if m > 12:
            continue
        for start in sorted({0, n - 1}):
            p = cyclic_cut(text, start, m)
            more.append(p)
            more += edited(p, text)
    return list(dict.fromkeys(base + more))


def planted(text, rs, count, m_lo, m_hi):
    """`count` patterns cut from the (linear) text at random, m in [m_lo, m_hi], in turn: as cut, one byte removed, one byte
    doubled, one substituted, one removed and one doubled."""
    t = bytes(text)
    n = len(t)
    out = []
    for i in range(count):
        m = int(rs.randint(m_lo, m_hi + 1))
        at = int(rs.randint(0, n - m))
        p = bytearray(t[at:at + m])
        kind = i % 5
        x = int(rs.randint(1, m - 1))                                   # an inner byte
        if kind in (1, 4) and m >= 4:
            del p[x]
        if kind in (2, 4):
            y = int(rs.randint(1, len(p) - 1))
            p[y:y] = p[y:y + 1]
        if kind == 3:
            p[x] = t[(at * 7 + 3) % n]
        out.append(bytes(p))
    return out


# ---- the larger cases of tests/test_gpu_edit.py; tests/test_edit_cpu.py asserts on the CPU what they are chosen for -----------------

def four_case():
    """(2^16 bytes over 4 symbols, 100 planted patterns of 3 .. 24 bytes): more than one workgroup, lengths that differ in a wave."""
    text = bytes(np.random.RandomState(7).randint(97, 101, 1 << 16).astype(np.uint8))
    return text, [text[500:503]] + planted(text, np.random.RandomState(11), 99, 4, 24)


def random_case():
    """(2^20 random bytes, 64 patterns of 8 bytes): 48 random, 8 cut with one byte removed, 8 cut with one byte doubled."""
    text = bytes(np.random.RandomState(3).randint(0, 256, 1 << 20).astype(np.uint8))
    rs = np.random.RandomState(4)
    pats = [bytes(rs.randint(0, 256, 8).astype(np.uint8)) for _ in range(48)]
    for i in range(8):
        at = 1000 + 100000 * i
        cut = text[at:at + 9]
        pats.append(cut[:3 + i % 4] + cut[4 + i % 4:])                 # nine bytes, one removed
        cut = text[at + 50:at + 57]
        pats.append(cut[:2 + i % 4] + cut[1 + i % 4:])                 # seven bytes, one doubled
    return text, pats


def scan_case():
    """(the four-symbol text, 2100 patterns, k = 1): one pattern with more than 10^4 hits next to patterns with none."""
    text = four_case()[0]
    return text, [b"abc", b"\x00\x01\x02", b"zzzz", text[-2:] + text[:1], text[-1:] + text[:2]] + [b"\x01\x02\x03\x04"] * 2095


def linear_case():
    """The header's example: P = abcd, a text that ends in abc and starts with d, k = 2."""
    body = bytes(np.random.RandomState(9).randint(120, 123, 500).astype(np.uint8))
    return b"d" + body + b"abc", b"abcd"
