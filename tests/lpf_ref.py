"""Reference for the self-index queries (bce_hip_lpf, bce_hip_self_parse, bce_hip_nsv_device), from the definitions alone: the
longest previous factor by search, all nearest smaller values with a stack, the greedy chain one position at a time, the fewest
phrases by a dynamic programme, and a decoder that sees the ops and the literal bytes and never the text."""
import numpy as np

NONE = 0xFFFFFFFF


def lpf_brute(text, max_len):
    """lpf[i] = the largest l <= min(max_len, n - i) with T[j:j+l] == T[i:i+l] for some j < i: every l tried, nothing assumed."""
    n, out = len(text), []
    for i in range(n):
        best = 0
        for l in range(1, min(max_len, n - i) + 1):
            if text.find(text[i:i + l], 0, i + l - 1) < 0:             # an occurrence that starts in front of i ends in front of i + l
                break
            best = l
        out.append(best)
    return out


def lpf(text, max_len):
    """The same for texts of any size: the search for position i starts at lpf[i - 1] - 1, which the uncapped array never
    undercuts (drop the first byte of i - 1's factor), so the whole array costs about 2 n searches."""
    n, out, prev = len(text), [], 0
    for i in range(n):
        cap = min(max_len, n - i)
        l = min(max(prev - 1, 0), cap)
        while l < cap and text.find(text[i:i + l + 1], 0, i + l) >= 0:
            l += 1
        out.append(l)
        prev = l                                                       # (capped at max_len it is still a lower bound)
    return out


def check_src(text, lpf_arr, src):
    """Every source by content and order; NONE exactly where the length is 0."""
    for i, (l, s) in enumerate(zip(np.asarray(lpf_arr).tolist(), np.asarray(src).tolist())):
        if l == 0:
            assert s == NONE, (i, s)
        else:
            assert s < i and text[s:s + l] == text[i:i + l], (i, l, s)


def ansv(vals):
    """psv, nsv with a stack; strict: an equal value is not smaller."""
    vals = np.asarray(vals).tolist()
    n = len(vals)
    psv, nsv, st = [NONE] * n, [NONE] * n, []
    for r, v in enumerate(vals):
        while st and vals[st[-1]] >= v:
            st.pop()
        if st:
            psv[r] = st[-1]
        st.append(r)
    st = []
    for r in range(n - 1, -1, -1):
        v = vals[r]
        while st and vals[st[-1]] >= v:
            st.pop()
        if st:
            nsv[r] = st[-1]
        st.append(r)
    return np.array(psv, dtype=np.uint32), np.array(nsv, dtype=np.uint32)


def chain(lpf_arr, text, min_len):
    """The self-parse from lengths: phrases (start, len, is_copy) in text order with literal runs merged, the literal bytes, info."""
    lens = np.asarray(lpf_arr).tolist()
    n, s, ph, lits, ncopies, copied = len(lens), 0, [], bytearray(), 0, 0
    while s < n:
        if lens[s] >= min_len:
            ph.append((s, lens[s], True))
            ncopies += 1
            copied += lens[s]
            s += lens[s]
        else:
            if ph and not ph[-1][2]:
                ph[-1] = (ph[-1][0], ph[-1][1] + 1, False)
            else:
                ph.append((s, 1, False))
            lits.append(text[s])
            s += 1
    return ph, bytes(lits), {"nops": len(ph), "nlits": len(lits), "ncopies": ncopies, "copied": copied}


def self_parse(text, min_len, max_len):
    return chain(lpf(text, max_len), text, min_len)


def pairs(ops):
    """(len, src) rows of an ops array, whether records (api.OP_DTYPE) or pairs of words."""
    a = np.asarray(ops)
    if a.dtype.names:
        return list(zip(a["len"].tolist(), a["src"].tolist()))
    return [tuple(r) for r in a.reshape(-1, 2).tolist()]


def decode(ops, lits):
    """Left to right, from the ops and the literal bytes alone.  A copy may overlap what it writes: byte by byte."""
    out, at, lits = bytearray(), 0, np.asarray(lits if not isinstance(lits, (bytes, bytearray)) else np.frombuffer(lits, dtype=np.uint8), dtype=np.uint8).tobytes()
    for l, s in pairs(ops):
        if s == NONE:
            out += lits[at:at + l]
            at += l
        else:
            assert s < len(out), "a copy from text that does not exist yet"
            for k in range(l):
                out.append(out[s + k])
    assert at == len(lits)
    return bytes(out)


def check(text, want, ops, lits, info):
    """ops / lits / info of a self-parse against chain()'s answer: structure, literal bytes, info, every copy by content and order."""
    ph, wl, winfo = want
    got = pairs(ops)
    assert len(got) == len(ph), (len(got), len(ph))
    for (start, ln, is_copy), (l, s) in zip(ph, got):
        assert l == ln, (start, l, ln)
        if is_copy:
            assert s != NONE and s < start and text[s:s + l] == text[start:start + l], (start, l, s)
        else:
            assert s == NONE, (start, s)
    assert bytes(lits) == wl
    assert {k: int(info[k]) for k in winfo} == winfo, (info, winfo)
    assert winfo["nlits"] + winfo["copied"] == len(text)


def fewest_phrases(text, max_len):
    """The fewest phrases of any parse of T into substrings of at most max_len bytes that occur earlier (start j < the phrase's
    start, overlap allowed) and single literal bytes."""
    n = len(text)
    best = [0] + [n + 1] * n
    for i in range(n):
        best[i + 1] = min(best[i + 1], best[i] + 1)
        for l in range(1, min(max_len, n - i) + 1):
            if text.find(text[i:i + l], 0, i + l - 1) < 0:
                break
            best[i + l] = min(best[i + l], best[i] + 1)
    return best[n]


def rotation_order(text, rs=None):
    """The sorted rotations; equal rotations (a periodic text) in shuffled order where rs is given."""
    n = len(text)
    idx = list(range(n))
    if rs is not None:
        rs.shuffle(idx)
    return sorted(idx, key=lambda i: text[i:] + text[:i])


def summary_line(text, min_len, max_len):
    """What `bce -gz` prints."""
    _ph, _lits, info = self_parse(text, min_len, max_len)
    return "%d copies of %d bytes, %d literal bytes in %d runs: %d phrases at bounds %d .. %d; %d of %d bytes repeat earlier text" % (
        info["ncopies"], info["copied"], info["nlits"], info["nops"] - info["ncopies"], info["ncopies"] + info["nlits"], min_len, max_len,
        info["copied"], len(text))
