"""Brute-force references for the pattern counts (tests/test_count_cpu.py, tests/test_gpu_count.py): pure Python / numpy on the
text itself, nothing of the index."""
import numpy as np


def cyclic_count(text, pat) -> int:
    """The i in [0, n) with pat[k] == text[(i + k) mod n] for all k; the empty pattern: n."""
    text, pat = bytes(text), bytes(pat)
    n, m = len(text), len(pat)
    ext = text * (m // n + 2)
    return sum(1 for i in range(n) if ext[i:i + m] == pat)


def linear_count(text, pat) -> int:
    """What bytes.count would give if it counted overlapping matches (pat not empty)."""
    text, pat = bytes(text), bytes(pat)
    found, at = 0, text.find(pat)
    while at >= 0:
        found += 1
        at = text.find(pat, at + 1)
    return found


def cyclic_cut(text, start, m) -> bytes:
    """m bytes of the circular text from position start (m may exceed n)."""
    text = bytes(text)
    n = len(text)
    return bytes(text[(start + k) % n] for k in range(m))


def bwt_of_rotations(text):
    """(BWT of the sorted cyclic rotations, the row of rotation 0) -- what K1 computes, by sorting in Python."""
    text = bytes(text)
    n = len(text)
    dbl = text + text
    order = sorted(range(n), key=lambda i: dbl[i:i + n])
    return bytes(text[(i - 1) % n] for i in order), order.index(0)


def sliding_counts(text, pats, m):
    """Linear counts of equally long patterns (rows of a 2-D uint8 array) in a numpy text, by a sliding-window compare."""
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(text, dtype=np.uint8), m)
    out = []
    for p in pats:
        idx = np.flatnonzero(win[:, 0] == p[0])                      # the windows that start with the pattern's first byte
        out.append(int(np.count_nonzero((win[idx] == p).all(axis=1))))
    return np.array(out, dtype=np.uint64)
