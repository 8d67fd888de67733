"""Reference of `bce -s`'s symbol records, one by one: bce_core.h's scan_pack restated in numpy, the streams the eight ScanCoders
must be fed (from the oracle's trace), and the input families that reach each enumeration route in scan mode
(tests/test_scanrec_cpu.py checks all of it on the CPU; tests/test_gpu_scan_routes.py holds the kernels against it).
The builders of the tail inputs live here too; tests/test_gpu_tail.py imports them back."""
import functools

import numpy as np

import oracle
from conftest import edge_inputs

K_MAX = 31


# ---- the word -----------------------------------------------------------------------------------------------------------------
def scan_pack(sym, k, c1, c2, cs):
    """bce_core.h's scan_pack on arrays: [4:0] sym, [9:5] k (2..31), [17:10] (c1 << 8) / cs, [25:18] (c2 << 8) / cs, [30:26]
    escapes.  The k > 31 loop is ScanCoder's own: k = (k >> 1) + (~s & 1), s >>= 1 (not AdaptiveCoder's (k + (~s & 1)) >> 1);
    c << 8 is a uint32 shift and wraps from 2^24."""
    sym, k, c1, c2, cs = (np.array(v, dtype=np.uint32, ndmin=1) for v in (sym, k, c1, c2, cs))
    nesc = np.zeros(len(k), dtype=np.uint32)
    while True:
        m = k > K_MAX
        if not m.any():
            break
        nesc[m] += 1
        s0 = sym[m]
        k[m] = (k[m] >> np.uint32(1)) + (~s0 & np.uint32(1))
        sym[m] = s0 >> np.uint32(1)
    q1 = (c1 << np.uint32(8)) // cs                      # uint32 throughout: the shift drops the high byte
    q2 = (c2 << np.uint32(8)) // cs
    return sym | (k << np.uint32(5)) | (q1 << np.uint32(10)) | (q2 << np.uint32(18)) | (nesc << np.uint32(26))


def unpack(word):
    w = int(word)
    return {"sym": w & 31, "k": (w >> 5) & 31, "q1": (w >> 10) & 255, "q2": (w >> 18) & 255, "nesc": (w >> 26) & 31}


def trace_syms(data):
    """The oracle's symbol rows (plane, s, k, c1, c2, cs) in its call order."""
    bwt, off = oracle.bwt_stage(data)
    return np.ascontiguousarray(oracle.trace_encode_from_bwt(bwt, off)["syms"], dtype=np.uint32)


def streams_of(syms):
    """Plane p's rows in trace order, packed: what ScanCoder p is fed (the filter emul_scan applies, tests/core_emul.cpp)."""
    words = scan_pack(syms[:, 1], syms[:, 2], syms[:, 3], syms[:, 4], syms[:, 5]) if len(syms) else np.zeros(0, dtype=np.uint32)
    return [words[syms[:, 0] == p] for p in range(8)]


def expected_streams(data):
    return streams_of(trace_syms(data))


def first_mismatch(got, want):
    """None, or a sentence naming the first record that differs: the plane, the index and both words unpacked."""
    for p in range(8):
        g, w = got[p], want[p]
        m = min(len(g), len(w))
        bad = np.nonzero(g[:m] != w[:m])[0]
        if len(bad):
            i = int(bad[0])
            return "plane %d record %d of %d: got 0x%08x %r, want 0x%08x %r (%d of the plane's records differ)" % (
                p, i, len(w), int(g[i]), unpack(g[i]), int(w[i]), unpack(w[i]), len(bad))
        if len(g) != len(w):
            return "plane %d: %d records, want %d (the first %d agree)" % (p, len(g), len(w), m)
    return None


def is_primitive(data):
    """No rotation of the input equals it (then the enumeration visits 8n - 8 nodes)."""
    return len(data) == 1 or (data + data).find(data, 1) == len(data)


# ---- the tail inputs (tests/test_gpu_tail.py) -----------------------------------------------------------------------------------
def repeat_input(n, rep, seed=21):
    base = oracle.synth_text(seed, n)
    chunk = base[1000:1000 + rep]
    return base[:n // 2] + chunk + base[n // 2:]


def many_copies(copies, length, seed):
    """`copies` copies of one block, each followed by a different separator: chains of `copies` rows."""
    block = oracle.synth_text(seed, length)
    out = bytearray(oracle.synth_text(seed + 1, 20000))
    for i in range(copies):
        out += block + b"<%06d>" % (i * 7919 % 1000003)
    out += oracle.synth_text(seed + 2, 20000)
    return bytes(out)


def _region(unit, length):
    return (unit * (length // len(unit) + 1))[:length]


STAIRCASE_CASES = ["zeros", "ff", "period2", "period3", "period7-in-random", "two-regions", "at-start", "at-end",
                   "record-table", "period2-twice", "three-regions-phases", "many-zero-runs", "same-length-twice",
                   "whole-text-periodic", "two-tables-first-at-start"]


def staircase_input(case):
    """Long runs of one byte and periodic tables (executables): chains whose rows are equally spaced text positions."""
    rs = np.random.RandomState(5)
    text = oracle.synth_text(91, 60000)
    rnd = rs.randint(0, 256, 60000).astype(np.uint8).tobytes()
    if case == "zeros":
        return text[:30000] + bytes(9000) + text[30000:]
    if case == "ff":
        return text[:30000] + b"\xff" * 7000 + text[30000:] + b"\xff" * 100 + b"z"
    if case == "period2":
        return text[:20000] + _region(b"\x00\x02", 12001) + text[20000:]
    if case == "period3":
        return rnd[:20000] + _region(b"abc", 10000) + text[:20000] + _region(b"cab", 500) + rnd[20000:40000]
    if case == "period7-in-random":
        return rnd[:30000] + _region(b"\x01\x00\x00\x00\x00\x00\x80", 15000) + rnd[30000:]
    if case == "two-regions":     # the same pattern twice: the node is a staircase only below the shorter one
        return text[:20000] + bytes(6000) + text[20000:40000] + bytes(4000) + b"\x01" + bytes(300) + text[40000:]
    if case == "at-start":        # the region reaches position 0: the walkers must not take the shortcut blindly
        return bytes(5000) + text + _region(b"\x00\x07", 3000) + b"q"
    if case == "at-end":
        return text + _region(b"xy", 8000)
    if case == "period2-twice":   # the same table in two places, same bytes before it: two rows leave together
        return text[:20000] + b"\x00\x00" + _region(b"\x00\x02", 9001) + b"\x01" + text[20000:40000] + b"\x00\x00" + _region(b"\x00\x02", 7000) + text[40000:]
    if case == "three-regions-phases":   # three places, different phases at the start and different bytes before
        return (rnd[:10000] + b"Q" + _region(b"abc", 6000) + rnd[10000:20000] + b"R" + _region(b"bca", 5000) + b"a" + text[:20000] +
                b"Q" + _region(b"cab", 4001) + b"\xff" + rnd[20000:30000])
    if case == "many-zero-runs":  # more regions than the closed form takes at once: the walkers take over until few are left
        return b"".join(text[i * 3000:(i + 1) * 3000] + bytes(300 * (i + 1) + (i % 3)) for i in range(14)) + text[42000:]
    if case == "whole-text-periodic":   # the region IS the text up to its last byte: it starts at position 0, where the
        return b"ab" * 30000 + b"c"        # byte "before" is the last one (rotations)
    if case == "two-tables-first-at-start":
        return _region(b"\x00\x00\x01", 20000) + text[:30000] + b"\x07" + _region(b"\x00\x01\x00", 14000) + text[30000:]
    if case == "same-length-twice":
        return text[:20000] + b"A" + bytes(5000) + b"B" + text[20000:40000] + b"A" + bytes(5000) + b"C" + text[40000:]
    if case == "record-table":    # 16-byte records that differ in one counter byte, then identical ones
        return text[:10000] + b"".join(b"REC" + bytes([i & 255]) + bytes(12) for i in range(300)) + (b"REC\x00" + bytes(12)) * 400 + text[10000:]
    raise ValueError(case)


def _spine_input(kind, seed=5, runs=1500, text_bytes=120000):
    rng = np.random.RandomState(seed)
    text = oracle.synth_text(70 + seed, text_bytes)
    if kind == "zero-runs":            # runs of zeros of hundreds of different lengths between random bytes: the all-zero context keeps
        parts = []                     # thousands of rows for thousands of bytes, a few runs end at every length
        for _ in range(runs):
            parts.append(rng.bytes(int(rng.randint(1, 24))))
            parts.append(bytes(int(rng.randint(1, 3000))))
        return text[:60000] + b"".join(parts) + text[60000:]
    if kind == "equal-runs":           # hundreds of runs of the SAME length: the first rows of the chain all leave at once
        return text[:50000] + b"".join(rng.bytes(3) + bytes(2048) for _ in range(300)) + text[50000:] + b"".join(
            rng.bytes(5) + bytes(int(rng.randint(1500, 2500))) for _ in range(200))
    if kind == "u16-ramps":            # little-endian 16-bit arrays with small values: the context alternates between two bytes
        arrs = [np.minimum(rng.geometric(0.2, int(rng.randint(200, 4000))), 200).astype("<u2").tobytes() for _ in range(300)]
        return text[:30000] + b"".join(a + rng.bytes(2) for a in arrs) + text[30000:]
    if kind == "records":              # records of 12 bytes whose last 9 are constant, in tables of many lengths
        recs = [b"".join(rng.bytes(3) + b"\x00\x00\x00\x01\x00\x00\x00\xff\x10" for _ in range(int(rng.randint(50, 1500)))) for _ in range(200)]
        return text[:40000] + b"".join(r + rng.bytes(int(rng.randint(1, 9))) for r in recs) + text[40000:]
    raise ValueError(kind)


# ---- the families of the scan-mode tests ----------------------------------------------------------------------------------------
SPINE_RUNS, SPINE_TEXT = 25, 40000    # _spine_input("zero-runs") cut down from 1500 runs in 120 000 bytes of text; see test_gpu_scan_routes.py


def _half():
    return oracle.synth_text(8, 1 << 17)


FAMILIES = {}
for _name, _data in edge_inputs():
    FAMILIES["edge-" + _name] = (lambda d=_data: d)
FAMILIES.update({
    "nonode-a": lambda: b"a", "nonode-d2x14": lambda: b"\xd2" * 14, "nonode-zeros-1000": lambda: bytes(1000), "nonode-ab-x7": lambda: b"ab" * 7,
    "text-64k": lambda: oracle.synth_text(1, 65536), "rand-64k": lambda: oracle.synth_rand(1, 65536),
    "repeat": lambda: repeat_input(300000, 2500, seed=33),
    "copies": lambda: many_copies(60, 900, 71),
})
for _case in STAIRCASE_CASES:
    FAMILIES["stair-" + _case] = (lambda c=_case: staircase_input(c))
FAMILIES.update({
    "periodic-ab-c": lambda: b"ab" * 30000 + b"c",
    "periodic-halves": lambda: _half() + _half(),
    "periodic-halves-hash": lambda: _half() + _half() + b"#",
    "spine": lambda: _spine_input("zero-runs", runs=SPINE_RUNS, text_bytes=SPINE_TEXT),
})
# the same bytes through RankFile(bwt=, offset=): no text on the device, so no chain skip and no closed form
INJECTED = {"injected-zeros": "stair-zeros", "injected-repeat": "repeat"}
# the four that also run under every knob
KNOB_FAMILIES = ["repeat", "stair-period2-twice", "spine", "rand-64k"]


@functools.lru_cache(maxsize=None)
def family_input(name):
    return FAMILIES[INJECTED.get(name, name)]()


@functools.lru_cache(maxsize=None)
def family_reference(name):
    """-> (the eight expected streams, oracle.scan's table, oracle.scan's nine doubles) of a family; computed once, read-only."""
    name = INJECTED.get(name, name)
    data = family_input(name)
    streams = expected_streams(data)
    for s in streams:
        s.setflags(write=False)
    cfg, res = oracle.scan(data)
    return streams, cfg, tuple(res)
