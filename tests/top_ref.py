"""References for the list of the most frequent cyclic k-grams (tests/test_top_cpu.py, tests/test_gpu_top*.py, the CLI tests): pure
Python and numpy on the text itself, nothing of the index; and the same list from an LCP array, for the scans' hook."""
from collections import Counter

import numpy as np


def cyclic_kgrams(text, k):
    """Counter of the n cyclic k-grams text[(i + j) mod n], j < k, as byte strings."""
    text = bytes(text)
    n = len(text)
    ext = text * (k // n + 2)
    return Counter(ext[i:i + k] for i in range(n))


def size_hist(sizes):
    """hist[b] = the sizes with floor(log2 size) = b, b < 32."""
    hist = [0] * 32
    for s in sizes:
        hist[int(s).bit_length() - 1] += 1
    return hist


def top_kgrams(text, k, limit):
    """(entries, distinct, size_hist): entries = the first `limit` of the distinct cyclic k-grams by (-count, gram) as (count, row,
    gram), row = the sum of the counts of the lexicographically smaller k-grams: the first row of the k-gram among the sorted
    rotations."""
    cnt = cyclic_kgrams(text, k)
    row, rows = 0, {}
    for g in sorted(cnt):
        rows[g] = row
        row += cnt[g]
    ents = sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))[:limit]
    return [(c, rows[g], g) for g, c in ents], len(cnt), size_hist(cnt.values())


def classes_of_lcp(lcp, k):
    """(starts, sizes) of the maximal runs of rows [s, e) with lcp[r] >= k for s < r < e, in row order (numpy int64)."""
    lcp = np.asarray(lcp, dtype=np.int64)
    starts = np.flatnonzero(np.concatenate([[True], lcp[1:] < k]))
    return starts, np.diff(np.concatenate([starts, [len(lcp)]]))


def top_of_lcp(lcp, k, limit):
    """(counts, rows, distinct, size_hist) of the first `limit` classes of an LCP array by size descending, first row ascending."""
    starts, sizes = classes_of_lcp(lcp, k)
    order = np.lexsort((starts, -sizes))[:limit]
    hist = np.bincount(np.frexp(sizes.astype(np.float64))[1] - 1, minlength=32)   # (size = m 2^e, 1/2 <= m < 1: floor(log2 size) = e - 1, exactly)
    return sizes[order], starts[order], len(starts), hist.tolist()


def escape(gram):
    """A k-gram as `bce -gf` prints it: printable ASCII other than backslash and space as it is, everything else as \\xHH."""
    return "".join(chr(b) if 0x20 < b < 0x7F and b != 0x5C else "\\x%02X" % b for b in bytes(gram))
