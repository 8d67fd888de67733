"""A plain numpy restatement of the GPU decoder's back end (kd_decode.hip: planes() and inverse_bwt()), for
tests/test_gpu_unbwt.py; checked on the CPU by tests/test_unbwt_ref_cpu.py.

Planes: the eight wavelet-matrix levels of the BWT bytes.  Level j holds bit j of every byte in the order the stable partitions
on bits 0 .. j - 1 left them (zeros first).  R_full[p][i] = the ones of level p in front of position i, i = 0 .. n.  The decoder
knows only some of those boundary ranks (kUnknown elsewhere) and relies on every gap between two known ones being constant.

Inverse BWT: LF by one stable sort on the byte, the walk from row 0 backwards through the text, the text's position i at
out[(i + off) % n]; a walk that closes after lc < n rows with lc | n is a periodic text, the cycle repeated n / lc times.
"""
import numpy as np

K_UNKNOWN = 0xFFFFFFFF
FG_CHUNK = 8192                                  # positions of R per workgroup of the fill kernels


def plane_words(n):
    return (n + 31) // 32 + 3


def fill_chunks(n):
    return (n + 1 + FG_CHUNK - 1) // FG_CHUNK


def walker_shift(rows):
    """lf_walk's stride: at most 2^19 walkers; at least 256 rows each while that leaves 4096 of them."""
    sh = 0
    while (rows >> sh) > (1 << 19):
        sh += 1
    while sh < 8 and (rows >> (sh + 1)) >= 4096:
        sh += 1
    return sh


def walkers(rows):
    return ((rows - 1) >> walker_shift(rows)) + 1


def pack_words(bits, R_full):
    """One level's bits and full ranks -> (words, rankw) in the kernel's layout: LSB first, plane_words(n) words, the rank at each
    word's first position where that is <= n, zero past it."""
    n = len(bits)
    W = plane_words(n)
    padded = np.zeros(W * 32, dtype=np.uint8)
    padded[:n] = bits
    words = np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)
    starts = np.arange(W, dtype=np.int64) * 32
    rankw = np.where(starts <= n, R_full[np.minimum(starts, n)], 0).astype(np.uint32)
    return words, rankw


def planes_of(bwt):
    """-> (bits u8 [8][n], zeros [8], R_full u32 [8][n + 1], words u32 [8][W], rankw u32 [8][W])."""
    cur = np.ascontiguousarray(bwt, dtype=np.uint8)
    n = len(cur)
    W = plane_words(n)
    bits = np.empty((8, n), dtype=np.uint8)
    R_full = np.zeros((8, n + 1), dtype=np.uint32)
    words, rankw = np.empty((8, W), dtype=np.uint32), np.empty((8, W), dtype=np.uint32)
    zeros = []
    for j in range(8):
        b = (cur >> j) & 1
        bits[j] = b
        np.cumsum(b, dtype=np.uint32, out=R_full[j, 1:])
        zeros.append(n - int(R_full[j, n]))
        words[j], rankw[j] = pack_words(b, R_full[j])
        one = b.astype(bool)
        cur = np.concatenate([cur[~one], cur[one]])              # the stable partition on bit j
    return bits, zeros, R_full, words, rankw


def access(bits, zeros, R_full):
    """The bytes back from the levels: position i followed through the eight partitions."""
    n = bits.shape[1]
    pos = np.arange(n, dtype=np.int64)
    out = np.zeros(n, dtype=np.uint8)
    for j in range(8):
        b = bits[j][pos]
        r1 = R_full[j][pos].astype(np.int64)
        out |= (b << j).astype(np.uint8)
        pos = np.where(b == 1, zeros[j] + r1, pos - r1)
    return out


def minimal_known(bits_p):
    """The boundaries a sparse rank array cannot do without: 0, n, and every i with bits[i - 1] != bits[i]."""
    n = len(bits_p)
    known = np.zeros(n + 1, dtype=bool)
    known[0] = known[n] = True
    if n > 1:
        known[1:n] = bits_p[1:] != bits_p[:-1]
    return known


def sparse_ranks(R_full, bits, keep=None):
    """R_full [8][n + 1], bits [8][n] -> u32 [8][n + 1] that knows the minimal boundaries of every level and those of `keep`
    (a bool mask [8][n + 1] or [n + 1], or an index array for all levels); K_UNKNOWN elsewhere."""
    n = bits.shape[1]
    R = np.full((8, n + 1), K_UNKNOWN, dtype=np.uint32)
    for p in range(8):
        known = minimal_known(bits[p])
        if keep is not None:
            k = np.asarray(keep)
            if k.dtype == bool:
                known |= k[p] if k.ndim == 2 else k
            else:
                known[k[(k >= 0) & (k <= n)]] = True
        R[p, known] = R_full[p, known]
    return R


def gaps_constant(R):
    """The fill kernels' precondition: both ends of every level known (R[p][0] = 0), ranks that never decrease, and between two
    neighbouring known boundaries either no ones or nothing but ones."""
    for p in range(R.shape[0]):
        idx = np.flatnonzero(R[p] != K_UNKNOWN)
        if len(idx) == 0 or idx[0] != 0 or idx[-1] != R.shape[1] - 1 or R[p, 0] != 0:
            return False
        r = R[p, idx].astype(np.int64)
        d, w = np.diff(r), np.diff(idx)
        if not np.all((d == 0) | (d == w)):
            return False
    return True


def lf_of(bwt):
    a = np.ascontiguousarray(bwt, dtype=np.uint8)
    order = np.argsort(a, kind="stable")                          # the stable counting sort: row order[k] is the k-th smallest
    lf = np.empty(len(a), dtype=np.int64)
    lf[order] = np.arange(len(a), dtype=np.int64)
    return lf


def walk_rows(lf, steps):
    """lf^t(0) for t = 0 .. >= steps, by doubling (the walk itself, 2^k steps at a time)."""
    seq, jump = np.zeros(1, dtype=np.int64), lf
    while len(seq) <= steps:
        seq = np.concatenate([seq, jump[seq]])
        jump = jump[jump]
    return seq


def inverse(bwt, off):
    """-> (text with position i at (i + off) % n, LF cycle length through row 0); the text is None when the cycle's length does
    not divide n."""
    a = np.ascontiguousarray(bwt, dtype=np.uint8)
    n = len(a)
    seq = walk_rows(lf_of(a), n)
    lc = int(np.flatnonzero(seq[1:n + 1] == 0)[0]) + 1             # lf is a permutation: the walk comes back to row 0
    if n % lc:
        return None, lc
    cycle = a[seq[:lc]][::-1]                                     # the walk meets the text's bytes last to first
    return np.roll(np.tile(cycle, n // lc), off % n), lc


def inverse_slow(bwt, off):
    """The same, one row at a time."""
    a = np.ascontiguousarray(bwt, dtype=np.uint8)
    n = len(a)
    lf = lf_of(a)
    rows, row = [], 0
    while True:
        rows.append(row)
        row = int(lf[row])
        if row == 0:
            break
    lc = len(rows)
    if n % lc:
        return None, lc
    text = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        text[(i + off) % n] = a[rows[lc - 1 - (i % lc)]]
    return text, lc


def seam_inverse(u, idx):
    """inverse_bw_transform(T = u, n, idx) as the GPU seam does it: the sentinel's row put back at `idx` (n + 1 rows, symbol 0 below
    every byte), LF, the walk from row 0.  -> the n text bytes, or None when the n + 1 rows are not one cycle."""
    a = np.ascontiguousarray(u, dtype=np.uint8)
    n = len(a)
    sym = np.insert(a.astype(np.int64) + 1, idx, 0)
    order = np.argsort(sym, kind="stable")
    lf = np.empty(n + 1, dtype=np.int64)
    lf[order] = np.arange(n + 1, dtype=np.int64)
    seq = walk_rows(lf, n + 1)
    lc = int(np.flatnonzero(seq[1:n + 2] == 0)[0]) + 1
    if lc != n + 1:
        return None
    text = (sym[seq[:lc]][::-1] - 1)                              # positions of $T, the sentinel first
    return np.roll(text, n)[:n].astype(np.uint8)
