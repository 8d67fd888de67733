"""Record streams for the K4 model kernels (bce_amd/csrc/k4_model.hip), built so that every route of a flush is taken on purpose.

A flush sorts its records (stable) on key bits 10..28 = plane | slot, so every slot's records become one run; which kernel
replays a run depends on its length (256 and more: the long route, k = 2 on a walker of its own) and on where in the 64-record
windows of the sorted array it starts and ends.  The generators here place runs at chosen lanes by putting filler runs on slots
that sort in front of them.  Every case carries `checks`: the properties it exists for, computed from its records and the
sequential reference alone (tests/test_model_cpu.py asserts them without a GPU), so that a generator that drifts cannot quietly
stop covering its case.  tests/test_gpu_model.py runs the same cases through bce_hip_model_flush.

Shared by the two test files; not a conftest.
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LONG = 256            # K4_LONG: runs at least this long take the long route
GW = 16               # K4_GW: windows per staged group of the general long walk
GW2 = 64              # windows per step of the k = 2 walker
LONG_WAVES = 1024 * 4  # waves k4_long_kernel launches; it strides over the queue of long runs

DEFAULT_CONFIG = np.array([
    [0, 0, 5, 5, 5] + [4] * 26 + [0],
    [0, 0, 5, 5, 5] + [4] * 26 + [0],
    [0, 0, 5, 5, 5] + [4] * 22 + [3] * 4 + [0],
    [0, 0, 5, 5, 5] + [4] * 17 + [3] * 9 + [0],
    [0, 0, 5, 5] + [4] * 8 + [3] * 19 + [0],
    [0, 0, 5, 5] + [4] * 8 + [3] * 19 + [0],
    [0, 0, 5] + [4] * 6 + [3] * 22 + [0],
    [0, 0] + [4] * 4 + [3] * 19 + [2] * 6 + [0],
    [0] * 32], dtype=np.uint8).tobytes()


def config_random():
    return np.random.RandomState(3).randint(0, 6, size=288).astype(np.uint8).tobytes()


def config_flat(bits):
    return bytes([bits]) * 288


# ---- the sequential reference (tests/core_emul.cpp: model_step in a loop) ----------------------------------------------------
_emul = None


def load_emul():
    global _emul
    if _emul is None:
        out = os.path.join(ROOT, "tests", "_build", "libcore_emul.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        srcs = [os.path.join(ROOT, "tests", "core_emul.cpp"), os.path.join(ROOT, "bce_amd", "csrc", "host_coder.cpp"),
                os.path.join(ROOT, "bce_amd", "csrc", "scan_coder.cpp")]
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out] + srcs + ["-lpthread"])
        L = C.CDLL(out)
        L.emul_model_state_bytes.argtypes = [C.c_void_p]
        L.emul_model_state_bytes.restype = C.c_uint64
        L.emul_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.emul_model.restype = C.c_int64
        _emul = L
    return _emul


class Reference:
    """emul_model with the counter state kept between calls, as K4 keeps it between flushes."""

    def __init__(self, config=None):
        self.L = load_emul()
        self.cfg = np.frombuffer(config or DEFAULT_CONFIG, dtype=np.uint8).copy()
        self.state = np.zeros(int(self.L.emul_model_state_bytes(self.cfg.ctypes.data)), dtype=np.uint8)

    def step(self, keys, escs):
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        escs = np.ascontiguousarray(escs, dtype=np.uint32)
        out = np.empty(len(keys), dtype=np.uint64)
        rc = self.L.emul_model(self.cfg.ctypes.data, keys.ctypes.data, escs.ctypes.data, len(keys), self.state.ctypes.data,
                               len(self.state), out.ctypes.data)
        if rc != 0:
            raise ValueError("emul_model refused record %d" % (rc - 1))
        return out


def out_freq(rec):
    return ((rec >> np.uint64(13)) & np.uint64(0xFF)).astype(np.int64) + 1


# ---- geometry of a config: which slots exist ---------------------------------------------------------------------------------
class Geometry:
    def __init__(self, config=None):
        cfg = np.frombuffer(config or DEFAULT_CONFIG, dtype=np.uint8).reshape(9, 32)
        self.bits = cfg[:8].astype(np.int64)
        self.nctx = np.zeros((8, 32), dtype=np.int64)
        self.ctxoff = np.zeros((8, 32), dtype=np.int64)
        self.off = np.zeros((8, 32), dtype=np.int64)
        self.stat_bytes = np.zeros(8, dtype=np.int64)
        for p in range(8):
            slots = start = 0
            for k in range(2, 32):
                self.ctxoff[p, k], self.off[p, k] = slots, start
                self.nctx[p, k] = 1 << (2 * self.bits[p, k])
                slots += self.nctx[p, k]
                start += k * self.nctx[p, k]
            self.stat_bytes[p] = start

    def all_slots(self, kmin=2, kmax=31):
        """(gid, k) of every slot with kmin <= k <= kmax; gid = plane << 16 | slot, the sort key of a record."""
        g, kk = [], []
        for p in range(8):
            for k in range(kmin, kmax + 1):
                lo = int(self.ctxoff[p, k])
                g.append((p << 16) + lo + np.arange(self.nctx[p, k], dtype=np.int64))
                kk.append(np.full(self.nctx[p, k], k, dtype=np.int64))
        return np.concatenate(g), np.concatenate(kk)

    def pick(self, rng, count, kmin=2, kmax=31):
        g, k = self.all_slots(kmin, kmax)
        sel = rng.choice(len(g), size=count, replace=False)
        return g[sel], k[sel]


def pack_keys(gid, k, sym):
    return (np.asarray(sym, dtype=np.uint32) | (np.uint32(k) << np.uint32(5)) | (np.uint32(gid) << np.uint32(10))).astype(np.uint32)


def esc_word(nesc, bits):
    return np.uint32((int(nesc) << 27) | (int(bits) & ((1 << int(nesc)) - 1)))


def make_stream(runs, rng, order="shuffle"):
    """runs: (gid, k, syms[, escs]) -> key and escape words in a stream order that keeps each run's own order.
    shuffle: the runs' records interleaved at random; reverse: run after run, the highest slot first."""
    if order == "reverse":
        runs = sorted(runs, key=lambda r: -r[0])
    keys = np.concatenate([pack_keys(r[0], r[1], r[2]) for r in runs]) if runs else np.zeros(0, np.uint32)
    escs = np.concatenate([np.asarray(r[3], dtype=np.uint32) if len(r) > 3 and r[3] is not None else np.zeros(len(r[2]), np.uint32)
                           for r in runs]) if runs else np.zeros(0, np.uint32)
    if order == "shuffle" and len(runs) > 1:
        label = np.repeat(np.arange(len(runs)), [len(r[2]) for r in runs])
        where = np.argsort(rng.permutation(label), kind="stable")       # run r's records go to its labels' places, in order
        k2, e2 = np.empty_like(keys), np.empty_like(escs)
        k2[where], e2[where] = keys, escs
        keys, escs = k2, e2
    return keys, escs


class Layout:
    """Runs in the order they will have in the sorted array: each new run takes the next free slot of its k."""

    def __init__(self, config=None):
        self.geo = Geometry(config)
        self.plane, self.slot, self.total, self.runs = 0, 0, 0, []

    def run(self, k, syms, escs=None, plane=None, slot=None):
        syms = np.asarray(syms, dtype=np.uint32)
        assert len(syms) and int(syms.max()) < k
        for p in range(self.plane if plane is None else plane, 8):
            lo = int(self.geo.ctxoff[p, k])
            hi = lo + int(self.geo.nctx[p, k])
            cand = max(lo, self.slot) if p == self.plane else lo
            if slot is not None:
                assert p == plane and lo <= slot < hi and slot >= cand
                cand = slot
            if cand < hi:
                assert (p, cand) >= (self.plane, self.slot)
                self.plane, self.slot = p, cand + 1
                self.runs.append(((p << 16) | cand, k, syms, escs))
                start = self.total
                self.total += len(syms)
                return start
            assert slot is None and plane is None
        raise AssertionError("no slot of k = %d left behind the cursor" % k)

    def _filler_k(self):
        """the smallest k that still has a slot behind the cursor in its plane (the next plane starts again at 2)"""
        for k in range(2, 32):
            if self.plane < 8 and self.geo.ctxoff[self.plane, k] + self.geo.nctx[self.plane, k] > self.slot:
                return k
        return 2

    def pad_to(self, lane):
        """a filler run, on a slot that sorts in front, so that the next run starts on `lane` of a window"""
        self.filler((lane - self.total) % 64)

    def filler(self, n):
        while n > 0:
            m, k = min(n, 200), self._filler_k()
            self.run(k, (np.arange(m) * 5 // 3) % k)
            n -= m

    def stream(self, seed, order="shuffle"):
        return make_stream(self.runs, np.random.RandomState(seed), order)


# ---- what a stream does, from its records and the reference's outputs --------------------------------------------------------
def run_table(keys):
    """One flush: (order, starts, lens, first key of each run) of the stable sort on bits 10..28."""
    gid = (keys >> np.uint32(10)) & np.uint32(0x7FFFF)
    order = np.argsort(gid, kind="stable")
    sg = gid[order]
    starts = np.flatnonzero(np.concatenate([[True], sg[1:] != sg[:-1]])) if len(sg) else np.zeros(0, np.int64)
    lens = np.diff(np.concatenate([starts, [len(sg)]]))
    return order, starts, lens, keys[order[starts]] if len(sg) else np.zeros(0, np.uint32)


def long_run_count(keys):
    return int((run_table(keys)[2] >= LONG).sum())


class Analysis:
    """Per flush of a case's own plan: the runs of the sorted array, and where the reference halves."""

    def __init__(self, case, ref):
        self.case = case
        edges = [0] + list(case.cuts) + [len(case.keys)]
        self.flush = []
        for lo, hi in zip(edges[:-1], edges[1:]):
            keys = case.keys[lo:hi]
            order, starts, lens, first = run_table(keys)
            pos = np.empty(len(keys), dtype=np.int64)
            pos[order] = np.arange(len(keys))
            hp = np.sort(pos[out_freq(ref[lo:hi]) == 0xFF])              # freq 0xFF: the counter was 0xFE, this record halves
            r = np.searchsorted(starts, hp, side="right") - 1
            self.flush.append(dict(
                n=hi - lo, starts=starts, lens=lens, k=(first.astype(np.int64) >> 5) & 31, first=first,
                h_pos=hp, h_run=r, h_lane=hp % 64, h_relwin=hp // 64 - starts[r] // 64 if len(hp) else hp,
                h_last=hp == starts[r] + lens[r] - 1 if len(hp) else hp.astype(bool),
                h_len=lens[r] if len(hp) else hp, h_k=((first.astype(np.int64) >> 5) & 31)[r] if len(hp) else hp))

    def f(self, i=-1):
        return self.flush[i]

    def runs(self, i=-1, k=None, long=None):
        """(start, length, k) rows of flush i"""
        f = self.flush[i]
        m = np.ones(len(f["starts"]), dtype=bool)
        if k is not None:
            m &= (f["k"] == 2) if k == 2 else (f["k"] > 2)
        if long is not None:
            m &= (f["lens"] >= LONG) == long
        return np.stack([f["starts"][m], f["lens"][m], f["k"][m]], axis=1)

    def halvings(self, i=-1, k=None, long=None):
        """boolean mask over flush i's halvings"""
        f = self.flush[i]
        m = np.ones(len(f["h_pos"]), dtype=bool)
        if k is not None:
            m &= (f["h_k"] == 2) if k == 2 else (f["h_k"] > 2)
        if long is not None:
            m &= (f["h_len"] >= LONG) == long
        return m


class Case:
    def __init__(self, name, keys, escs, config=None, cuts=(), checks=()):
        self.name, self.config = name, config
        self.keys = np.ascontiguousarray(keys, dtype=np.uint32)
        self.escs = np.ascontiguousarray(escs, dtype=np.uint32)
        self.cuts = [int(c) for c in cuts]          # the case's own flush plan: cut points inside the stream
        self.checks = list(checks)                  # (what, function of an Analysis -> bool)

    def probes(self):
        """k more records for every slot the stream touched, one per symbol: their freq fields spell the counters out."""
        slot = np.unique(self.keys >> np.uint32(5))                     # (gid, k) pairs
        k = (slot & np.uint32(31)).astype(np.int64)
        rep = np.repeat(slot, k)
        sym = np.arange(len(rep)) - np.repeat(np.cumsum(k) - k, k)
        return ((rep << np.uint32(5)) | sym.astype(np.uint32)).astype(np.uint32), np.zeros(len(rep), np.uint32)


MAX_SMALL_FLUSHES = 1000


def flush_plans(case, ref):
    """name -> cut points.  Fixed sizes 1, 64, 1000 (at most MAX_SMALL_FLUSHES flushes of the size, the rest of a longer stream
    in one: a flush costs a sort, four kernels and a copy whatever its size), random cut points from a fixed seed, the case's
    own plan, and a cut right behind every record that brings a counter to 0xFE (freq 0xFE in the reference; at most 64, spread
    evenly) -- the next flush then enters with that counter one event from halving."""
    n = len(case.keys)
    plans = {"one": []}
    if case.cuts:
        plans["own"] = list(case.cuts)
    for c in (1, 64, 1000):
        cuts = np.arange(c, min(n, c * MAX_SMALL_FLUSHES + 1), c)
        plans["cut%d" % c] = [int(x) for x in cuts if 0 < x < n]
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7FFFFFFF)
    if n > 1:
        plans["random"] = sorted(set(int(x) for x in rng.randint(1, n, size=min(12, n - 1))))
    fe = np.flatnonzero(out_freq(ref[:n]) == 0xFE) + 1
    fe = fe[fe < n]
    if len(fe) > 64:
        fe = fe[np.linspace(0, len(fe) - 1, 64).astype(np.int64)]
    if len(fe):
        plans["at0xFE"] = sorted(set(int(x) for x in fe))
    return {k: v for k, v in plans.items() if k == "one" or v}


def segments(n, cuts):
    edges = [0] + list(cuts) + [n]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


# ---- the families ---------------------------------------------------------------------------------------------------------------
def _sym(rng, k, n, dist):
    if dist == "const0":
        return np.zeros(n, np.uint32)
    if dist == "constlast":
        return np.full(n, k - 1, np.uint32)
    if dist == "uniform":
        return rng.randint(0, k, n).astype(np.uint32)
    if dist == "skew":                                                  # ~97 % one symbol
        return np.where(rng.random_sample(n) < 0.97, k // 2, rng.randint(0, k, n)).astype(np.uint32)
    if dist == "alt":
        return (np.arange(n) % k).astype(np.uint32)
    raise ValueError(dist)


def _bits(rng, n, pat):
    if pat == "zeros":
        return np.zeros(n, np.uint32)
    if pat == "ones":
        return np.ones(n, np.uint32)
    if pat == "alt":
        return (np.arange(n) & 1).astype(np.uint32)
    p = {"half": 0.5, "rare": 0.01}[pat]
    return (rng.random_sample(n) < p).astype(np.uint32)


def _sizes():
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257):
        def mixed(n=n):
            rng = np.random.RandomState(100 + n)
            geo = Geometry()
            lens = []
            while sum(lens) < n:
                lens.append(min(n - sum(lens), int(rng.randint(1, 40))))
            g, k = geo.pick(rng, len(lens))
            keys, escs = make_stream([(g[i], k[i], _sym(rng, k[i], lens[i], "uniform")) for i in range(len(lens))], rng)
            return Case("size-mixed-%d" % n, keys, escs, checks=[("nsym = %d" % n, lambda a: a.f()["n"] == n)])
        out.append(("size-mixed-%d" % n, mixed))
        for k in (2, 3):
            def one(n=n, k=k):
                L = Layout()
                L.run(k, np.zeros(n, np.uint32))
                keys, escs = L.stream(1)
                return Case("size-onerun-k%d-%d" % (k, n), keys, escs,
                            checks=[("one run of %d records alone in the array" % n,
                                     lambda a: a.f()["n"] == n and list(a.f()["lens"]) == [n])])
            out.append(("size-onerun-k%d-%d" % (k, n), one))
    # a long run last in the sorted array, the array a whole number of windows and not (the `probe < nsym` test, `win >= nwin`)
    for k in (2, 7):
        for tail, rag in ((256, 0), (300, 0), (256, 1), (1100, 37), (4096 + 64 + 30, 63)):
            name = "tail-long-k%d-%d-rag%d" % (k, tail, rag)

            def tl(k=k, tail=tail, rag=rag, name=name):
                L = Layout()
                L.filler(150)
                L.pad_to((rag - tail) % 64)
                L.run(k, _sym(np.random.RandomState(tail), k, tail, "uniform"), plane=7)
                keys, escs = L.stream(tail + rag)
                return Case(name, keys, escs, checks=[
                    ("the last run of the sorted array is long", lambda a: a.f()["lens"][-1] == tail),
                    ("nsym %% 64 == %d" % rag, lambda a: a.f()["n"] % 64 == rag)])
            out.append((name, tl))
    return out


def _short():
    def many():
        # two flushes of its own: the first leaves 100..254 events of one symbol in every slot, so that in the second the
        # halvings fall INSIDE runs that are all short (within one flush a short run can only halve on its 255th record)
        rng = np.random.RandomState(7)
        geo = Geometry()
        S = 3000
        g, k = geo.pick(rng, S)
        pre = rng.randint(100, 255, S)
        sym = rng.randint(0, 32, S) % k
        a = make_stream([(g[i], k[i], np.full(pre[i], sym[i], np.uint32)) for i in range(S)], rng)
        ln = rng.randint(1, 256, S)
        ln[:40] = 255
        ln[40:80] = 1
        b = make_stream([(g[i], k[i], np.full(ln[i], sym[i], np.uint32) if i % 4 else _sym(rng, k[i], ln[i], "uniform")) for i in range(S)], rng)
        return Case("short-runs-3000-slots", np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), cuts=[len(a[0])], checks=[
            ("thousands of slots, every run short, lengths 1 and 255 included",
             lambda an: len(an.f()["lens"]) >= 3000 and an.f()["lens"].max() == 255 and an.f()["lens"].min() == 1),
            (">= 1000 halvings inside short runs, not on their last record",
             lambda an: int((~an.f()["h_last"]).sum()) >= 1000),
            ("halvings on the last record of a short run", lambda an: int(an.f()["h_last"].sum()) >= 5)])

    def crowded():
        rng = np.random.RandomState(8)
        geo = Geometry()
        S = 4000
        g, k = geo.pick(rng, S)
        ln = rng.randint(1, 21, S)
        keys, escs = make_stream([(g[i], k[i], _sym(rng, k[i], ln[i], "uniform")) for i in range(S)], rng)

        def heads_per_window(an):
            st = an.f()["starts"]
            return np.bincount(st // 64).max()
        return Case("short-runs-crowded-windows", keys, escs, checks=[
            (">= 8 runs start inside one window", lambda an: heads_per_window(an) >= 8)])

    def const255():
        # 255 events of one symbol from zero counters: the halving is the run's 255th record, still on the short route
        L = Layout()
        for k in (2, 3, 16, 31):
            for lane in (0, 1, 63):
                L.pad_to(lane)
                L.run(k, np.full(255, k - 1, np.uint32))
        keys, escs = L.stream(9)
        return Case("short-runs-255-constant", keys, escs, checks=[
            ("12 short runs halve on their 255th record", lambda an: int((an.f()["h_last"] & (an.f()["h_len"] == 255)).sum()) == 12)])
    return [("short-runs-3000-slots", many), ("short-runs-crowded-windows", crowded), ("short-runs-255-constant", const255)]


def _threshold():
    out = []
    for k in (2, 5):
        name = "threshold-k%d" % k

        def th(k=k, name=name):
            L = Layout()
            want = []
            for ln in (255, 256, 257):
                for lane in (0, 63, 17):
                    L.pad_to(lane)
                    want.append((L.run(k, np.zeros(ln, np.uint32)), ln))
            L.pad_to(0)
            L.run(k, np.ones(40, np.uint32))             # another slot's run starts the window behind a run that ended on lane 63
            keys, escs = L.stream(11 + k)

            def has(an, ln, lane):
                f = an.f()
                return bool(((f["lens"] == ln) & (f["starts"] % 64 == lane)).any())

            def end_lane(an, lane, next_starts_window=False):
                f = an.f()
                end = (f["starts"] + f["lens"] - 1) % 64
                m = (f["lens"] >= LONG) & (end == lane)
                if next_starts_window:
                    nxt = np.isin(f["starts"] + f["lens"], f["starts"])
                    m &= nxt & ((f["starts"] + f["lens"]) % 64 == 0)
                return bool(m.any())
            checks = [("a run of %d starting on lane %d" % (ln, lane), lambda an, ln=ln, lane=lane: has(an, ln, lane))
                      for ln in (255, 256, 257) for lane in (0, 63, 17)]
            checks += [("a long run ends on lane 63 and another slot's run starts the next window", lambda an: end_lane(an, 63, True)),
                       ("a long run ends on lane 0", lambda an: end_lane(an, 0)),
                       ("long runs: exactly the six of 256 and 257", lambda an: int((an.f()["lens"] >= LONG).sum()) == 6)]
            return Case(name, keys, escs, checks=checks)
        out.append((name, th))
    return out


def _general_long():
    out = []

    def dist_case(dist, ks, lens, seed, extra=()):
        name = "long-%s" % dist

        def build():
            rng = np.random.RandomState(seed)
            L = Layout()
            for i, (k, ln) in enumerate(zip(ks, lens)):
                L.pad_to(int(rng.randint(0, 64)))
                L.run(k, _sym(rng, k, ln, dist))
            keys, escs = L.stream(seed)
            checks = [("k > 2 long runs from 256 to ~1e5 records",
                       lambda an: an.runs(k=3, long=True)[:, 1].min() == 256 and an.runs(k=3, long=True)[:, 1].max() >= 100000),
                      ("runs spanning several 16-window groups", lambda an: int((an.runs(k=3, long=True)[:, 1] > 3 * GW * 64).sum()) >= 3)]
            return Case(name, keys, escs, checks=checks + list(extra))
        return name, build
    halves = ("halvings inside general long runs", lambda an: int(an.halvings(k=3, long=True).sum()) >= 50)
    out.append(dist_case("const0", [3, 4, 7, 16, 31, 5, 9], [256, 300, 1000, 5000, 20000, 100000, 2500], 21, [halves]))
    out.append(dist_case("uniform", list(range(3, 32)) + [6, 12], [256, 257, 300, 383, 511, 512, 640, 1000, 1024, 1500, 2000, 3000, 4000, 5000,
                                                                   700, 900, 1100, 1300, 1700, 1900, 2100, 2300, 2900, 3100, 3300, 3700, 4100, 4300, 4700,
                                                                   100000, 30000], 22,
                         [("every k from 3 to 31 has a long run", lambda an: set(an.runs(k=3, long=True)[:, 2]) == set(range(3, 32))), halves]))
    out.append(dist_case("skew", [3, 5, 8, 13, 21, 31, 17], [256, 400, 3000, 9000, 40000, 100000, 1500], 23, [halves]))

    def k31():
        L = Layout()
        for lane, ln in ((0, 256), (5, 4000), (63, 100000), (31, 1337)):
            L.pad_to(lane)
            L.run(31, np.full(ln, 30, np.uint32), escs=np.zeros(ln, np.uint32))
        keys, escs = L.stream(24)
        return Case("long-k31-sym30", keys, escs, checks=[
            ("k = 31 runs of sym 30 only", lambda an: set(an.runs(long=True)[:, 2]) == {31} and
             bool(((an.case.keys & 31) == 30)[((an.case.keys >> np.uint32(5)) & 31) == 31].all())),
            ("halvings 128 events apart in the long runs", lambda an: int(an.halvings(k=3, long=True).sum()) >= 700)])
    out.append(("long-k31-sym30", k31))

    def group_edges():
        # the walk's groups start at the window behind the run's first: a run that ends exactly where a group ends has
        # (64 - start lane) + 1024 m records; one record less leaves the group's last window one short
        rng = np.random.RandomState(25)
        L = Layout()
        want = []
        for lane in (0, 37):
            for m in (1, 2):
                for short in (0, 1):
                    L.pad_to(lane)
                    ln = (64 - lane) + GW * 64 * m - short
                    want.append((L.run(4 + m, _sym(rng, 4 + m, ln, "skew")), ln))
        keys, escs = L.stream(25)

        def ends(an, short):
            f = an.f()
            lg = f["lens"] >= LONG
            head = 64 - f["starts"] % 64
            return int((lg & ((f["lens"] - head + short) % (GW * 64) == 0) & (f["lens"] > head + 64)).sum())
        return Case("long-group-boundary", keys, escs, checks=[
            ("4 runs end exactly on a 16-window group boundary (last window full)", lambda an: ends(an, 0) == 4),
            ("4 runs end one record short of it", lambda an: ends(an, 1) == 4)])
    out.append(("long-group-boundary", group_edges))

    def lanes():
        # one symbol from zero counters: the halvings are events 254, 382, 510, ... of the run, so a run that starts on lane 2
        # has every one of them on lane 0 of a window, one that starts on lane 1 on lane 63; 255 + 128 j records: the last halves
        L = Layout()
        for k, lane, ln in ((3, 2, 4000), (9, 1, 2000), (31, 2, 700), (6, 1, 5000), (5, 20, 255 + 128 * 3), (12, 0, 255 + 128)):
            L.pad_to(lane)
            L.run(k, np.full(ln, k // 2, np.uint32))
        keys, escs = L.stream(26)

        def on_lane(an, lane):
            f = an.f()
            return int((an.halvings(k=3, long=True) & (f["h_lane"] == lane) & (f["h_relwin"] > 0)).sum())
        return Case("long-halving-lanes", keys, escs, checks=[
            (">= 20 halvings on lane 0 of a window, behind the head fragment", lambda an: on_lane(an, 0) >= 20),
            (">= 20 halvings on lane 63", lambda an: on_lane(an, 63) >= 20),
            ("2 long runs halve on their last record", lambda an: int((an.halvings(k=3, long=True) & an.f()["h_last"]).sum()) == 2)])
    out.append(("long-halving-lanes", lanes))

    def head():
        # the first flush leaves counters of 200..254 behind, so the long runs of the second halve inside their head fragment
        rng = np.random.RandomState(27)
        L = Layout()
        pre = []
        for k, lane, c0 in ((3, 10, 230), (7, 0, 254), (31, 40, 250), (4, 63, 254), (16, 1, 200), (5, 30, 254)):
            L.pad_to(lane)
            L.run(k, np.full(1500, k - 1, np.uint32))
            pre.append((L.runs[-1][0], k, np.full(c0, k - 1, np.uint32)))
        a = make_stream(pre, rng)
        b = L.stream(27)
        return Case("long-halving-in-head", np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), cuts=[len(a[0])], checks=[
            ("6 long runs halve inside their head fragment", lambda an: int((an.halvings(k=3, long=True) & (an.f()["h_relwin"] == 0)).sum()) == 6),
            ("one of them on the run's first record, on lane 63", lambda an: bool((an.halvings(k=3, long=True) & (an.f()["h_relwin"] == 0) & (an.f()["h_lane"] == 63)).any()))])
    out.append(("long-halving-in-head", head))
    return out


def _k2():
    out = []
    for pat in ("zeros", "ones", "alt", "half", "rare"):
        name = "k2-%s" % pat

        def build(pat=pat, name=name):
            rng = np.random.RandomState(30 + len(pat))
            L = Layout()
            for lane, ln in ((0, 256), (9, 700), (63, 4096), (2, 4096 * 3 + 500), (33, 20000), (0, 64 * GW2 * 2 + 64)):
                L.pad_to(lane)
                L.run(2, _bits(rng, ln, pat))
            keys, escs = L.stream(31)
            return Case(name, keys, escs, checks=[
                ("k = 2 long runs up to several 64-window groups", lambda an: an.runs(k=2, long=True)[:, 1].max() > 4096 * 3 and len(an.runs(k=2, long=True)) == 6),
                ("halvings in them", lambda an: int(an.halvings(k=2, long=True).sum()) >= 100)])
        out.append((name, build))

    def edges():
        # the walker's groups: 64 windows from the window behind the run's first
        rng = np.random.RandomState(36)
        L = Layout()
        for lane in (0, 21):
            for m in (1, 2):
                for extra in (0, 64, -1, 1):
                    L.pad_to(lane)
                    L.run(2, _bits(rng, (64 - lane) + GW2 * 64 * m + extra, "half" if m == 1 else "rare"))
        keys, escs = L.stream(36)

        def ends(an, extra):
            f = an.f()
            head = 64 - f["starts"] % 64
            return int(((f["lens"] >= LONG) & (f["k"] == 2) & ((f["lens"] - head - extra) % (GW2 * 64) == 0)).sum())
        return Case("k2-group-boundary", keys, escs, checks=[
            ("4 runs end exactly on a 64-window group boundary", lambda an: ends(an, 0) == 4),
            ("4 runs end one window past it", lambda an: ends(an, 64) == 4),
            ("4 one record short, 4 one record past", lambda an: ends(an, -1) == 4 and ends(an, 1) == 4)])
    out.append(("k2-group-boundary", edges))

    def carried():
        # both counters one or two events from 0xFF when the long run's flush begins
        rng = np.random.RandomState(37)
        L = Layout()
        pre = []
        for lane, c0, c1, pat in ((0, 254, 254, "alt"), (5, 253, 253, "half"), (63, 254, 253, "ones"), (17, 253, 254, "zeros"), (40, 254, 254, "rare")):
            L.pad_to(lane)
            L.run(2, _bits(rng, 5000, pat))
            pre.append((L.runs[-1][0], 2, np.concatenate([np.zeros(c0, np.uint32), np.ones(c1, np.uint32)])))
        a = make_stream(pre, rng)
        b = L.stream(37)

        def entry(an):
            # counters at the second flush's start, from the first flush's records: no halving there, so they are the counts
            f0 = an.flush[0]
            return len(f0["h_pos"]) == 0 and f0["lens"].min() >= 506 and f0["lens"].max() <= 508
        return Case("k2-counters-carried-at-0xFE", np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), cuts=[len(a[0])], checks=[
            ("the first flush leaves both counters of 5 slots at 253 / 254 and halves nothing", entry),
            ("every long run of the second flush halves within its first 3 records", lambda an: int((an.halvings(k=2, long=True) & (an.f()["h_pos"] - an.f()["starts"][an.f()["h_run"]] < 3)).sum()) == 5)])
    out.append(("k2-counters-carried-at-0xFE", carried))

    def group_windows():
        # zeros from zero counters halve on events 254 + 128 j: a run starting on lane 0 halves in windows 3, 5, .., 65, .. of the
        # run (65 = the first window of the walker's second group), one starting on lane 2 in windows 4, 6, .., 64 (the last of the first)
        L = Layout()
        for lane in (0, 2):
            L.pad_to(lane)
            L.run(2, np.zeros(4096 * 3 + 200, np.uint32))
        L.pad_to(0)
        L.run(2, np.ones(4096 * 2 + 100, np.uint32))
        keys, escs = L.stream(38)

        def in_group_window(an, w):
            f = an.f()
            m = an.halvings(k=2, long=True) & (f["h_relwin"] >= 1)
            return int((m & ((f["h_relwin"] - 1) % GW2 == w)).sum())
        return Case("k2-halving-in-group-edge-windows", keys, escs, checks=[
            ("halvings in the first window of a group", lambda an: in_group_window(an, 0) >= 2),
            ("halvings in the last window of a group", lambda an: in_group_window(an, GW2 - 1) >= 2)])
    out.append(("k2-halving-in-group-edge-windows", group_windows))
    return out


def _many_long():
    def build():
        rng = np.random.RandomState(40)
        geo = Geometry()
        S = 5200
        g2, k2 = geo.pick(rng, S // 2, 2, 2)
        g3, k3 = geo.pick(rng, S - S // 2, 3, 31)
        g, k = np.concatenate([g2, g3]), np.concatenate([k2, k3])
        ln = rng.randint(256, 301, S)
        keys, escs = make_stream([(g[i], k[i], _sym(rng, k[i], ln[i], ("uniform", "const0", "skew")[i % 3])) for i in range(S)], rng)
        return Case("many-long-runs", keys, escs, checks=[
            ("more long runs than k4_long_kernel has waves", lambda an: len(an.runs(long=True)) >= 5000 > LONG_WAVES and len(an.runs(long=False)) == 0),
            ("all of 256..300 records, k = 2 and k > 2 mixed",
             lambda an: an.f()["lens"].min() >= 256 and an.f()["lens"].max() <= 300 and len(an.runs(k=2)) >= 2000 and len(an.runs(k=3)) >= 2000)])
    return [("many-long-runs", build)]


def _random_mix(name, config, seed, n, nslots):
    def build():
        rng = np.random.RandomState(seed)
        geo = Geometry(config)
        g_all, k_all = geo.all_slots()
        nsl = min(nslots, len(g_all))
        sel = rng.choice(len(g_all), size=nsl, replace=False)
        g, k = g_all[sel], k_all[sel]
        w = 1.0 / np.arange(1, nsl + 1) ** 1.1                          # a few slots take most of the records, the rest are short
        # half of the heaviest slots are binary ones, as in real streams
        heavy = np.argsort(k, kind="stable")[:max(2, nsl // 50)][::2]
        w[heavy], w[:len(heavy)] = w[:len(heavy)].copy(), w[heavy].copy()
        which = rng.choice(nsl, size=n, p=w / w.sum())
        expo = np.array([1.0, 1.0, 3.0, 12.0, 1e9])[rng.randint(0, 5, nsl)]   # uniform .. heavily skewed .. constant
        kk = k[which]
        sym = np.minimum((kk * rng.random_sample(n) ** expo[which]).astype(np.int64), kk - 1)
        flip = rng.random_sample(nsl) < 0.5                             # ... towards the last symbol for half of the slots
        sym = np.where(flip[which], kk - 1 - sym, sym)
        nesc = np.where((kk >= 16) & (rng.random_sample(n) < 0.3), rng.randint(1, 28, n), 0).astype(np.int64)
        ebits = rng.randint(0, 1 << 27, n).astype(np.int64) & ((np.int64(1) << nesc) - 1)
        keys = (sym | (kk << 5) | (g[which] << 10)).astype(np.uint32)
        escs = ((nesc << 27) | ebits).astype(np.uint32)
        return Case(name, keys, escs, config=config, checks=[
            ("%d records" % n, lambda an: an.f()["n"] == n),
            ("short and long runs of k = 2 and of k > 2; halvings in the long ones of both",
             lambda an: all(len(an.runs(k=kk_, long=lg)) > 0 for kk_ in (2, 3) for lg in (False, True)) and
             all(int(an.halvings(k=kk_, long=True).sum()) > 0 for kk_ in (2, 3)))])
    return name, build


def _configs():
    out = []
    for cname, cfg in (("default", None), ("random", config_random()), ("bits0", config_flat(0)), ("bits5", config_flat(5))):
        name = "planes-%s" % cname

        def build(cfg=cfg, name=name):
            rng = np.random.RandomState(50)
            geo = Geometry(cfg)
            runs = []
            for p in range(8):
                first = (p << 16) | int(geo.ctxoff[p, 2])
                last = (p << 16) | int(geo.ctxoff[p, 31] + geo.nctx[p, 31] - 1)
                runs.append((first, 2, _bits(rng, 100 + 300 * (p & 1), "half")))
                runs.append((last, 31, np.concatenate([_sym(rng, 31, 100 + 300 * (~p & 1), "skew"), [30, 0, 30]])))
                mid_k = 2 + (p * 3) % 29
                mid = (p << 16) | int(geo.ctxoff[p, mid_k] + geo.nctx[p, mid_k] - 1)
                if mid not in (first, last):
                    runs.append((mid, mid_k, _sym(rng, mid_k, 777, "uniform")))
            keys, escs = make_stream(runs, rng)

            def edges(an):
                gid = (an.case.keys >> np.uint32(10)).astype(np.int64)
                kk = (an.case.keys.astype(np.int64) >> 5) & 31
                ok = True
                for p in range(8):
                    ok &= bool(((gid == (p << 16)) & (kk == 2)).any())                       # slot 0 = the first counter of the plane
                    ok &= bool((gid == ((p << 16) | int(geo.ctxoff[p, 31] + geo.nctx[p, 31] - 1))).any())
                # the last counter byte of the last plane: sym 30 of its last k = 31 slot
                top = (7 << 16) | int(geo.ctxoff[7, 31] + geo.nctx[7, 31] - 1)
                ok &= int(geo.off[7, 31] + (geo.nctx[7, 31] - 1) * 31 + 30) == int(geo.stat_bytes[7]) - 1
                return ok and bool(((gid == top) & ((an.case.keys & 31) == 30)).any())
            return Case(name, keys, escs, config=cfg, checks=[
                ("all eight planes, each one's first and last slot, plane 7's highest counter offset", edges),
                ("both routes", lambda an: len(an.runs(long=True)) >= 8 and len(an.runs(long=False)) >= 8)])
        out.append((name, build))
    out.append(_random_mix("mix-config-random", config_random(), 60, 400000, 3000))
    out.append(_random_mix("mix-config-bits5", config_flat(5), 61, 400000, 3000))

    def bits0():
        # one slot per (plane, k): uniform records over the 240 slots make every k = 3..31 a long run in every flush
        rng = np.random.RandomState(62)
        n = 300000
        p = rng.randint(0, 8, n).astype(np.int64)
        k = rng.randint(2, 32, n).astype(np.int64)
        sym = np.minimum((k * rng.random_sample(n) ** 2.0).astype(np.int64), k - 1)
        nesc = np.where((k >= 16) & (rng.random_sample(n) < 0.2), rng.randint(1, 28, n), 0).astype(np.int64)
        keys = (sym | (k << 5) | ((k - 2) << 10) | (p << 26)).astype(np.uint32)
        escs = ((nesc << 27) | (rng.randint(0, 1 << 27, n).astype(np.int64) & ((np.int64(1) << nesc) - 1))).astype(np.uint32)
        return Case("mix-config-bits0", keys, escs, config=config_flat(0), checks=[
            ("240 slots, all long: every k = 3..31 on the general long route in every plane",
             lambda an: len(an.runs(long=True)) == 240 and len(an.runs(long=False)) == 0)])
    out.append(("mix-config-bits0", bits0))
    return out


def _escapes():
    def build():
        rng = np.random.RandomState(70)
        geo = Geometry()
        runs = []
        g, k = geo.pick(rng, 60, 16, 31)
        for i in range(60):
            ln = (40, 300, 2000)[i % 3]
            nesc = np.where(rng.random_sample(ln) < 0.5, 1 + (np.arange(ln) + i) % 27, 0).astype(np.int64)
            eb = rng.randint(0, 1 << 27, ln).astype(np.int64) & ((np.int64(1) << nesc) - 1)
            eb |= np.where(nesc > 0, np.int64(1) << np.maximum(nesc - 1, 0), 0)          # (the highest escape bit set: the sentinel sits right above it)
            runs.append((g[i], k[i], _sym(rng, k[i], ln, "skew"), ((nesc << 27) | eb).astype(np.uint32)))
        g, k = geo.pick(rng, 30, 2, 15)
        for i in range(30):
            runs.append((g[i], k[i], _sym(rng, k[i], (40, 300, 2000)[i % 3], "uniform")))
        keys, escs = make_stream(runs, rng)

        def ok(an):
            kk = (an.case.keys.astype(np.int64) >> 5) & 31
            ne = an.case.escs.astype(np.int64) >> 27
            return (set(ne[kk >= 16]) == set(range(0, 28)) and bool((an.case.escs[kk < 16] == 0).all()) and int((kk < 16).sum()) > 1000
                    and len(an.runs(long=True)) >= 40 and len(an.runs(long=False)) >= 20)
        return Case("escape-words", keys, escs, checks=[("nesc 0..27 on k >= 16 in short and long runs; k < 16 with an all-zero escape word", ok)])
    return [("escape-words", build)]


def _mixes():
    return [_random_mix("mix-default-1M", None, 80, 1000000, 20000),
            _random_mix("mix-default-2M", None, 81, 2000000, 40000),
            _random_mix("mix-default-4M", None, 82, 4000000, 60000)]


def all_cases():
    """[(name, builder)]: the builder makes the Case (streams of up to 4 M records are not kept around)."""
    out = []
    for fam in (_sizes, _short, _threshold, _general_long, _k2, _many_long, _configs, _escapes, _mixes):
        out += fam()
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


# ---- the rule itself, in plain Python (from the reference coder's text, not from bce_core.h) ---------------------------------
def python_model(keys, escs, slots=None):
    """Counters are bytes, one list of k per slot, zero at the start.  For symbol s of k: cum = sum of the counters below s, plus s;
    total = sum of all, plus k; freq = counter + 1; the counter goes up by one and when it reaches 0xFF all k are halved.
    -> the packed records ([12:0] cum, [20:13] freq - 1, [33:21] total, [61:34] escape bits under a sentinel bit)."""
    slots = {} if slots is None else slots
    out = []
    for kw, ew in zip(keys.tolist(), escs.tolist()):
        s, k, where = kw & 31, (kw >> 5) & 31, kw >> 10
        c = slots.setdefault(where, [0] * k)
        assert len(c) == k
        cum, total, freq = sum(c[:s]) + s, sum(c) + k, c[s] + 1
        c[s] += 1
        if c[s] == 0xFF:
            c[:] = [v >> 1 for v in c]
        sentinel = (ew & 0x7FFFFFF) | (1 << (ew >> 27))
        out.append(cum | ((freq - 1) << 13) | (total << 21) | (sentinel << 34))
    return np.array(out, dtype=np.uint64), slots
