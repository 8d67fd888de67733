"""Brute-force references for the searches with mismatches (tests/test_near_cpu.py, tests/test_gpu_near.py,
tests/test_gpu_cli_near.py): numpy on the text itself, nothing of the index.

T: the text, n bytes, read circularly; P: a pattern of m bytes; d(i) = #{ j < m : P[j] != T[(i + j) mod n] }, i in [0, n).  Cyclic
hits: the i with d(i) <= k; linear hits: those of them with i + m <= n."""
import numpy as np

from count_ref import cyclic_cut  # noqa: F401  (m bytes of the circular text from a position; m may exceed n)


def distances(text, pat):
    """d(i) for every i in [0, n): an int64 array.  Any m: the empty pattern is at distance 0 everywhere, m > n wraps."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    p = np.frombuffer(bytes(pat), dtype=np.uint8)
    n, m = len(t), len(p)
    ext = np.resize(t, n + m)                                        # (np.resize repeats the text: ext[i] = T[i mod n])
    d = np.zeros(n, dtype=np.int64)
    for j in range(m):
        d += ext[j:j + n] != p[j]
    return d


def _window(d, n, m, cyclic):
    return d if cyclic else d[:max(n - m + 1, 0)]


def counts(text, pat, k, cyclic=True):
    """The hits at distance exactly 0 .. k: a uint64 array of k + 1."""
    d = _window(distances(text, pat), len(text), len(pat), cyclic)
    return np.bincount(d[d <= k], minlength=k + 1)[:k + 1].astype(np.uint64)


def hits(text, pat, k, cyclic=True):
    """(the hits ascending as uint32, their distances as uint8)."""
    d = _window(distances(text, pat), len(text), len(pat), cyclic)
    at = np.flatnonzero(d <= k)
    return at.astype(np.uint32), d[at].astype(np.uint8)


def altered(pat, at, text):
    """`pat` with the bytes at the positions `at` replaced: by the next byte value of the text's alphabet where it has another, by
    the value + 1 otherwise -- a different byte in either case."""
    alphabet = sorted(set(bytes(text)))
    out = bytearray(pat)
    for j in at:
        v = out[j]
        nxt = alphabet[(alphabet.index(v) + 1) % len(alphabet)] if v in alphabet else v
        out[j] = nxt if nxt != v else (v + 1) % 256
    return bytes(out)


def bwt_and_order(text):
    """(BWT of the sorted cyclic rotations, the row of rotation 0, the order itself: a naive suffix array of the circular text,
    equal rotations in the order of their starts)."""
    text = bytes(text)
    n = len(text)
    dbl = text + text
    order = sorted(range(n), key=lambda i: dbl[i:i + n])
    return bytes(text[(i - 1) % n] for i in order), order.index(0), order


# ---- the cases of the CPU and GPU tests --------------------------------------------------------------------------------------------

SMALL = [b"a", b"ab", b"abab", b"aaaa", b"abracadabra", bytes(range(256)) * 3, b"\x00\xff" * 5]


def texts():
    """The 57 texts of test_count_cpu.py's generator, and one whose root interval has 256 different candidate bytes."""
    rs = np.random.RandomState(96)
    out = [b"a", b"ab", b"abab", b"aaaa", b"abracadabra", bytes(range(256)), b"\x00\xff" * 5]
    for i in range(50):
        sigma = (2, 3, 256)[i % 3]
        n = int(rs.randint(1, 41))
        out.append(bytes(int(v) for v in rs.randint(0, sigma, n)))
    return out + [bytes(range(256)) * 3]


def patterns_for(text):
    """Cut from the circular text at 0, n // 2 and n - 1 with m in {1, 2, 3, n - 1, n, n + 1, 2 n}; each of those with 1, 2 and 3
    bytes altered, at position 0, at position m - 1 and at adjacent positions in between; patterns with a byte the text lacks,
    first, last and in the middle; the empty pattern."""
    n = len(text)
    pats = [b""]
    for m in sorted({1, 2, 3, n - 1, n, n + 1, 2 * n} - {0}):
        for start in sorted({0, n // 2, n - 1}):
            p = cyclic_cut(text, start, m)
            pats.append(p)
            for a in (1, 2, 3):
                if a <= m:
                    pats += [altered(p, range(at, at + a), text) for at in sorted({0, m - a, (m - a) // 2})]
    for v in [v for v in range(256) if v not in set(text)][:1]:
        body = cyclic_cut(text, 0, min(n, 3) + 1)
        pats += [bytes([v]), bytes([v]) + body, body + bytes([v]), body[:2] + bytes([v]) + body[2:]]
    return list(dict.fromkeys(pats))
