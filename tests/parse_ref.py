"""Pure-Python reference of the delta parse and of the patch (tests/test_parse_cpu.py, tests/test_gpu_parse*.py): the chain of
include/bce_hip.h's definition walked one position at a time on the lengths of match_ref (linear mode), nothing of the index and
nothing of the block decomposition."""
import numpy as np

import match_ref

LITERAL = 0xFFFFFFFF


def _raw(b):
    return b.tobytes() if isinstance(b, np.ndarray) else bytes(b)


def chain(lens, min_len):
    """The phrases in ascending query order from the lengths by end position: [(start, length, is_copy)], literal bytes merged into
    maximal runs."""
    lens = np.asarray(lens).tolist()
    out = []
    e = len(lens) - 1
    while e >= 0:
        if lens[e] >= min_len:
            assert lens[e] <= e + 1
            out.append((e - lens[e] + 1, lens[e], True))
            e -= lens[e]
        else:
            if out and not out[-1][2] and out[-1][0] == e + 1:
                out[-1] = (e, out[-1][1] + 1, False)
            else:
                out.append((e, 1, False))
            e -= 1
    out.reverse()
    return out


def parse_of_lengths(lens, query, min_len):
    """-> (phrases, lits bytes, info dict) of the chain on these lengths"""
    query = bytes(query)
    ph = chain(lens, min_len)
    lits = b"".join(query[s:s + l] for s, l, cp in ph if not cp)
    ncop = sum(1 for p in ph if p[2])
    copied = sum(p[1] for p in ph if p[2])
    assert copied + len(lits) == len(query)
    return ph, lits, {"nops": len(ph), "nlits": len(lits), "ncopies": ncop, "copied": copied}


def parse(text, query, min_len, max_len):
    return parse_of_lengths(match_ref.match_lens(text, query, max_len), query, min_len)


def apply(text, ops, lits):
    """The bytes the (len, src) pairs and the literal bytes describe over the text."""
    text, lits = _raw(text), _raw(lits)
    out, at = [], 0
    for ln, src in np.asarray(ops, dtype=np.uint64).reshape(-1, 2).tolist():
        if src == LITERAL:
            out.append(lits[at:at + ln])
            at += ln
        else:
            assert src + ln <= len(text)
            out.append(text[src:src + ln])
    assert at == len(lits)
    return b"".join(out)


def pairs(ops):
    """ops as an (nops, 2) uint32 array, from a record array (len, src) or from pairs"""
    ops = np.asarray(ops)
    if ops.dtype.names:
        return np.stack([ops["len"], ops["src"]], axis=1).astype(np.uint32) if len(ops) else np.zeros((0, 2), dtype=np.uint32)
    return ops.astype(np.uint32).reshape(-1, 2)


def check(text, query, want, ops, lits, info, positions=True):
    """The structure is the reference's exactly -- op boundaries, kinds, lengths, the literal bytes, info -- and every copy is
    checked by content (text[src : src + len] == the query bytes it covers, src + len <= n); src values are never compared.
    positions=False: the copies carry src == 0 (the hook without positions) and are not read."""
    text, query = _raw(text), _raw(query)
    ph, wlits, winfo = want
    ops = pairs(ops)
    assert {k: int(v) for k, v in info.items()} == winfo, (info, winfo)
    assert len(ops) == len(ph)
    assert _raw(lits) == wlits
    want_ops = np.array([(p[1], p[2]) for p in ph], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(ops[:, 1] != LITERAL, want_ops[:, 1] == 1)
    assert np.array_equal(ops[:, 0].astype(np.int64), want_ops[:, 0])
    if not positions:
        assert not ops[ops[:, 1] != LITERAL, 1].any()
        return
    for (start, ln, cp), (oln, src) in zip(ph, ops.tolist()):
        if cp:
            assert src + ln <= len(text) and text[src:src + ln] == query[start:start + ln], (start, ln, src)
    assert apply(text, ops, lits) == query


def fewest_phrases(text, query, max_len):
    """The fewest phrases of any parse of the query into substrings of the text of at most max_len bytes and single literal bytes,
    every literal byte counted as one: a dynamic programme over the prefixes, best[i] = the fewest for query[:i]."""
    text, query = bytes(text), bytes(query)
    q = len(query)
    best = [0] + [q + 1] * q
    for i in range(1, q + 1):
        best[i] = best[i - 1] + 1                                     # a literal byte
        for l in range(1, min(max_len, i) + 1):
            if query[i - l:i] in text:
                best[i] = min(best[i], best[i - l] + 1)
            else:
                break                                                 # (substrings that end at i: a longer one contains the shorter)
    return best[q]
