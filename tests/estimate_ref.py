"""What tests/test_estimate_cpu.py and tests/test_gpu_estimate.py share: the inputs the issue names, the per-plane Q24 sums taken
from the oracle's trace of coder operations with the library's own cost function, and the size formula of bce_hip_estimate
written out a second time in Python (a 64-bit carry-less range coder for the header, bce.cpp:520-529, 610-615, 655-661)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "estimate_oracle.json")
Q24 = 1 << 24
WORD_Q24 = 16 * Q24            # one 16-bit word of a stream
FLUSH_WORDS = 1                # RangeCoder::flush (host_coder.cpp): its shift_out is a no-op behind encode(), then ONE word,
                               # which carries the up to 16 bits the coder still held: it IS the rounding up to whole words
M64 = (1 << 64) - 1


def inputs():
    """(name, bytes) of the inputs the accuracy of the method is measured on."""
    import oracle
    return [("abracadabra", b"abracadabra"), ("one-byte", b"a"), ("a-300", b"a" * 300),
            ("synth-text-4000", oracle.synth_text(1, 4000)), ("synth-text-1e5", oracle.synth_text(1, 10**5)),
            ("synth-text-1e6", oracle.synth_text(1, 10**6)),
            ("synth-rand-1e5", oracle.synth_rand(1, 10**5)), ("synth-rand-1e6", oracle.synth_rand(1, 10**6))]


def custom_config():
    """The 288-byte table tests/golden holds: the scanned config of oracle_fullsize.json's mixed-2e8-scanned vector."""
    with open(os.path.join(ROOT, "tests", "golden", "oracle_fullsize.json")) as f:
        v = [v for v in json.load(f)["vectors"] if "config_hex" in v][0]
    cfg = bytes.fromhex(v["config_hex"])
    assert len(cfg) == 288
    return cfg


DEFAULT_HEADER_ROW = bytes(32)      # row 8 of AdaptiveCoder<31>::init_ (bce.cpp:713-724), the header coder's: all zero


class _Log2:
    """L(x) = bce_hip_cost_q24(1, x), with the values below 8192 -- every total and freq of a model step -- looked up once."""

    def __init__(self):
        import bce_amd
        self.fn = bce_amd.load_library().bce_hip_cost_q24
        self.small = np.array([0] + [self.fn(1, x) for x in range(1, 8192)], dtype=np.int64)

    def __call__(self, x):
        x = np.asarray(x, dtype=np.int64)
        out = np.zeros(x.shape, dtype=np.int64)
        lo = x < 8192
        out[lo] = self.small[x[lo]]
        for i in np.flatnonzero(~lo):
            out[i] = self.fn(1, int(x[i]))
        return out


def oracle_sums(data, config=None):
    """-> (n, offset, plane_cost_q24[8], plane_steps[8]) from the oracle's trace.  The trace's ops hold every range-coder step in
    call order per coder -- the preamble, C[p], the k > 31 escape's uniform bits and the set(cum, freq, total) of every symbol --
    so nothing has to be derived from `syms`; the steps counted are the adaptive coder's calls, one row of `syms` each."""
    import oracle
    bwt, offset = oracle.bwt_stage(data)
    tr = oracle.trace_encode_from_bwt(bwt, offset, config)
    assert tr["archive"] == oracle.compress(data, config)
    ops, syms = tr["ops"].astype(np.int64), tr["syms"]
    L = _Log2()
    cost = L(ops[:, 3]) - L(ops[:, 2])
    assert (cost >= 0).all()
    plane_cost = [int(cost[ops[:, 0] == p].sum()) for p in range(8)]
    plane_steps = [int((syms[:, 0] == p).sum()) for p in range(8)]
    return len(data), int(offset), plane_cost, plane_steps


class RangeCoder:
    """AdaptiveCoder's range-coder half (bce.cpp:520-529, 538-553, 610-615, 655-661) for the archive's header."""

    def __init__(self):
        self.l, self.h, self.words = 0, M64, 0

    def encode(self, cum, freq, total):
        if self.h - self.l < total:
            self.words += 4
            self.l, self.h = 0, M64
        step = (self.h - self.l) // total
        self.l = (self.l + step * cum) & M64
        self.h = (self.l + step * freq - 1) & M64
        while not ((self.h ^ self.l) >> 48):
            self.words += 1
            self.l = (self.l << 16) & M64
            self.h = ((self.h << 16) & M64) | 0xFFFF

    def setv(self, s):                                           # VCoder::setv, bce.cpp:364-370
        while s:
            self.encode(s & 1, 1, 3)
            s >>= 1
        self.encode(2, 1, 3)

    def preamble(self, row):                                     # init(1, i), bce.cpp:682-691
        last = 0
        for bit in row:
            self.encode(int(bit != last), 1, 2)
            if bit != last:
                self.encode(bit, 1, 6)
            last = bit

    def flush(self):
        self.words += 1


def stream_words(cost_q24):
    return cost_q24 // WORD_Q24 + FLUSH_WORDS


def archive_bytes(n, offset, plane_cost_q24, config=None):
    """Exact framing + per plane the whole 16-bit words of its Q24 sum + the flush word (bce_cost.h: stream_words_q24)."""
    row8 = DEFAULT_HEADER_ROW if config is None else bytes(config)[8 * 32:9 * 32]
    words = [stream_words(c) for c in plane_cost_q24]
    size = sum(words)
    main = RangeCoder()                                          # BCE::encode :1141-1150 (HostCoder::rebuild_header)
    main.preamble(row8)
    main.setv(n)
    main.encode(offset, 1, n + 1)
    main.setv(size)
    s = size
    for i in range(7):
        main.encode(words[i], 1, s + 1)
        s -= words[i]
    main.flush()
    return 2 * (1 + main.words + size)                           # :1152-1157 (HostCoder::assemble)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# The bound on |estimate - real archive| the issue sets: twice the worst relative error recorded over the inputs above
# (estimate_oracle.json: measured by tools/make_estimate_golden.py, not chosen) plus what word rounding can cost -- 2 bytes per
# plane -- plus the flush words: one 2-byte word for each of the eight streams and for the header.
ROUNDING_BYTES = 2 * 8 + 2 * 9


def error_bound(real_bytes, worst_rel_error):
    return 2.0 * worst_rel_error * real_bytes + ROUNDING_BYTES


def tight_bound(records):
    """What the estimate can be off by when the model is right -- reasoned, not measured.  Word rounding and flush words as above;
    the cost function is within 2^-20 bit of log2 per call (tests/test_estimate_cpu.py checks exactly that), two calls per record,
    all errors taken with one sign; escape bits cost exactly one bit each.  What the coder itself loses to its truncated division
    (below total / 2^48 of the range per step) and to a range reset (four words, once per ~2^48 / total steps) is far below a byte
    at any n < 2^31.  At 1.4e8 records: 34 + 33 B."""
    return ROUNDING_BYTES + records * 2 * 2.0 ** -20 / 8
