"""Brute-force references for the searches by byte classes (tests/test_class_cpu.py, tests/test_gpu_classes.py,
tests/test_gpu_cli_classes.py): numpy on the text itself, nothing of the index.

T: the text, n bytes, read circularly; P: m classes S_0 .. S_(m-1) as an (m, 8) uint32 array, byte c in S iff bit c & 31 of word
c >> 5 is set.  Cyclic hits: the i in [0, n) with T[(i + j) mod n] in S_j for all j < m; linear hits: those with i + m <= n.
nodes(P) = #{ (j, s) : 1 <= j <= m, s a string of j bytes with s[t] in S_(m-j+t) for all t, s occurs in the circular text }."""
import numpy as np


def masks_of(sets):
    """[iterable of byte values, ...] -> the (m, 8) uint32 masks"""
    out = np.zeros((len(sets), 8), dtype=np.uint32)
    for j, members in enumerate(sets):
        for c in members:
            out[j, c >> 5] |= np.uint32(1 << (c & 31))
    return out


def exact(pat):
    """the pattern of one-member classes that is the byte string `pat`"""
    return masks_of([[c] for c in bytes(pat)])


ANY = list(range(256))


def inside(mask, c):
    """which of the bytes c (a uint8 array) lie in the class `mask` (8 words)"""
    return ((mask[c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


def matches(text, masks):
    """a bool array over i in [0, n): is i a cyclic hit?  Any m: the empty pattern is everywhere, m > n wraps."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(t)
    ok = np.ones(n, dtype=bool)
    for j in range(len(masks)):
        ok &= inside(masks[j], t[(np.arange(n) + j) % n])
    return ok


def hits(text, masks, cyclic=True):
    """the hits ascending, as uint32"""
    n, m = len(text), len(masks)
    at = np.flatnonzero(matches(text, masks))
    return (at if cyclic else at[at + m <= n]).astype(np.uint32)


def count(text, masks, cyclic=True):
    return len(hits(text, masks, cyclic))


def nodes(text, masks):
    """nodes(P): for j = 1 .. m the distinct strings among the cyclic windows of j bytes that match the pattern's last j classes.
    A window is named by the position e behind it; the windows of j bytes that match are those of j - 1 bytes that matched and whose
    byte at e - j lies in S_(m-j), and two of them are the same string iff that byte and the strings behind it are the same --
    np.unique over (byte, the number of the string of j - 1 bytes) per length."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n, m = len(t), len(masks)
    alive, ids, total = np.ones(n, dtype=bool), np.zeros(n, dtype=np.int64), 0
    for j in range(1, m + 1):
        c = t[(np.arange(n) - j) % n]
        alive &= inside(masks[m - j], c)
        if not alive.any():
            break
        _, inv = np.unique(c[alive].astype(np.int64) * n + ids[alive], return_inverse=True)
        ids[alive] = inv
        total += int(inv.max()) + 1
    return total


# ---- the cases of the CPU and GPU tests --------------------------------------------------------------------------------------------

def _cut(text, start, m):
    n = len(text)
    return bytes(text[(start + k) % n] for k in range(m))


def two_of(text, c):
    """a class of two members: c and the next byte value of the text's alphabet (c + 1 where the text has no other)"""
    alphabet = sorted(set(bytes(text)))
    nxt = alphabet[(alphabet.index(c) + 1) % len(alphabet)] if c in alphabet else c
    return sorted({c, nxt if nxt != c else (c + 1) % 256})


def wide_run(text, wide, tail=3):
    """`wide` two-member classes cut from the circular text at 0, then `tail` one-member ones: wide + tail classes"""
    p = _cut(text, 0, wide + tail)
    return masks_of([two_of(text, c) for c in p[:wide]] + [[c] for c in p[wide:]])


def cases_for(text):
    """The empty pattern; strings cut from the circular text at 0, n // 2 and n - 1 with m in {1, 2, 3, 5, n - 1, n, n + 1, 2 n} as
    one-member classes, and each of them with the class at the first, a middle and the last position replaced by a two-member
    class, the full class, the empty class and a class of one byte the text lacks; the full class at every position for m = 1, 2,
    3; exactly 64 two-member classes before three one-member ones, and 65 of them (refused).  Longer texts take fewer cuts."""
    n = len(text)
    absent = [v for v in range(256) if v not in set(text)][:1]
    out = [np.zeros((0, 8), dtype=np.uint32)]
    small = n <= 48
    for m in sorted(({1, 2, 3, 5, n - 1, n, n + 1, 2 * n} if small else {1, 2, 3, 5, n + 1}) - {0}):
        for start in sorted({0, n // 2, n - 1} if small else {n - 1}):
            p = _cut(text, start, m)
            sets = [[c] for c in p]
            out.append(masks_of(sets))
            for at in sorted({0, m // 2, m - 1}):
                for members in [two_of(text, p[at]), ANY, [], absent]:
                    out.append(masks_of(sets[:at] + [members] + sets[at + 1:]))
    out += [masks_of([ANY] * m) for m in (1, 2, 3)]
    return out + [wide_run(text, 64), wide_run(text, 65)]
