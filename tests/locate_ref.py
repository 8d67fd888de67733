"""Brute-force references for the pattern positions (tests/test_locate_cpu.py, tests/test_gpu_locate.py): pure Python / numpy on
the text itself, nothing of the index."""
import numpy as np


def cyclic_hits(text, pat):
    """The i in [0, n) with pat[k] == text[(i + k) mod n] for all k, ascending; the empty pattern: every i."""
    text, pat = bytes(text), bytes(pat)
    n, m = len(text), len(pat)
    ext = text * (m // n + 2)
    out, at = [], ext.find(pat)
    while 0 <= at < n:
        out.append(at)
        at = ext.find(pat, at + 1)
    return out


def linear_hits(text, pat):
    """The starts of pat in text that an overlapping scan finds, ascending (pat not empty)."""
    text, pat = bytes(text), bytes(pat)
    out, at = [], text.find(pat)
    while at >= 0:
        out.append(at)
        at = text.find(pat, at + 1)
    return out


def suffix_array_of_rotations(text):
    """The starts of the sorted cyclic rotations -- what K1 leaves behind, by sorting in Python (tied rotations of a periodic text
    in ascending order of their starts; K1 may leave them in another)."""
    text = bytes(text)
    n = len(text)
    dbl = text + text
    return sorted(range(n), key=lambda i: dbl[i:i + n])


def as_arrays(lists):
    return [np.array(h, dtype=np.uint32) for h in lists]
